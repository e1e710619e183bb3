"""K2's register rasteriser (pk_render.h render_line_regs) against the documented PPU.

tests/test_k2_frames.py and tests/test_ppu_spec.py hold the broad evidence (the 264 PyBoy frames and
every state of tests/ppu_cases.py).  Here are the states a word-wise decode can get wrong that those
reach only by chance: waves whose lanes all differ, under the three image interleaves; a sweep of
scroll, window and object edges built with tests/ppu_cases.make; the latch flags K2 consumes; and the
termination flags K2 writes in the place of pk_done_kernel.  The expected screens come from
tests/ppu_spec.py alone.  Every check runs on the CPU through the host-simulation build of the
unmodified kernel source and, marked gpu, on the gfx950 build.

The C ABI has no call that clears single latch flags, so the latch test holds the two whole-handle
states (every flag set, every flag clear); a frame whose flags K1 cleared in part is what the
vram_midframe_rom and raster_fx_rom cases of tests/test_gpu_parity.py and
tests/test_hostsim_parity.py run."""
import ctypes

import numpy as np
import pytest

from tests import ppu_cases, ppu_spec
from tests.ppu_cases import BG_OBJ, BG_OBJ16, SOLID, Y, make, solid_columns_vram

GREY = np.array([0xFF, 0x99, 0x55, 0x00], np.uint8)
SENTINEL = 0xA5      # no grey shade
NOOP = 8             # an action id that presses nothing


def _dummy_rom() -> bytes:
    rom = bytearray(0x8000)
    rom[0x147] = 0x13
    return bytes(rom)


# ------------------------------------------------------------------------------------------------
# the two backends behind one small interface
class _Sim:
    def __init__(self, n, frame_skip=24, render=True):
        from tests.hostsim.sim import SimEmulator, lib
        self.L = lib()
        self.emu = SimEmulator(_dummy_rom(), n, render=render, frame_skip=frame_skip)
        self.n = n

    def load(self, e, state):
        self.emu.load_env(e, state)

    def render_latched(self):
        self.emu.render_latched()

    def screen(self):
        return self.emu.screen()

    def fill_screen(self, v):
        p = self.L.pk_screen_ptr(self.emu.h)
        np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), shape=(self.n, 144, 160))[:] = v

    def step(self):
        self.emu.step(np.full(self.n, NOOP, np.uint8))

    def close(self):
        self.emu.close()


class _Gpu:
    def __init__(self, n, frame_skip=24, render=True):
        from pokegym_amd.emulator import BatchedEmulator
        self.emu = BatchedEmulator(_dummy_rom(), n, render=render, frame_skip=frame_skip)
        self.n = n

    def load(self, e, state):
        self.emu.load_env(e, state)

    def render_latched(self):
        self.emu.render_latched()

    def screen(self):
        import torch
        torch.cuda.synchronize()
        return self.emu.screen.cpu().numpy()

    def fill_screen(self, v):
        self.emu.screen.fill_(v)

    def step(self):
        import torch
        self.emu.step(torch.full((self.n,), NOOP, dtype=torch.uint8, device=self.emu.device))

    def close(self):
        self.emu.close()


BACKENDS = [pytest.param(_Sim, id="hostsim"), pytest.param(_Gpu, id="gpu", marks=pytest.mark.gpu)]


def _bad(names, got, want):
    return [(names[i], int((got[i] != want[i]).sum())) for i in range(len(names)) if not np.array_equal(got[i], want[i])]


# ------------------------------------------------------------------------------------------------
# 1. mixed waves
N_MIXED = 128


def _mixed_rounds():
    """Two loads of 128 envs that together hold every case of tests/ppu_cases.py, directed and random
    shuffled with a fixed seed: no two lanes of a wave hold the same state."""
    n = len(ppu_cases.all_cases())
    order = np.random.default_rng(0x4B32).permutation(n)
    assert N_MIXED < n <= 2 * N_MIXED
    return [order[:N_MIXED], order[n - N_MIXED:]]


@pytest.mark.parametrize("ilv", ["16", "32", "64"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_mixed_wave_equals_spec(backend, ilv, monkeypatch):
    monkeypatch.setenv("PK_ILV", ilv)
    cases = ppu_cases.all_cases()
    want = GREY[ppu_cases.expected()]
    rounds = _mixed_rounds()
    assert set(np.concatenate(rounds)) == set(range(len(cases)))
    for r in rounds:
        kinds = [cases[i][0].startswith("random_") for i in r[:64]]
        assert 8 <= sum(kinds) <= 56           # a wave mixes directed and random states
    b = backend(N_MIXED)
    try:
        for r in rounds:
            for e, i in enumerate(r):
                b.load(e, ppu_cases.full_state(cases[i][1]))
            b.render_latched()
            bad = _bad([cases[i][0] for i in r], b.screen(), want[r])
            assert not bad, bad[:10]
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------
# 2. edge sweep
def _sweep_cases():
    c = []

    def add(name, lcdc, **kw):
        c.append((name, make(lcdc, **kw)))

    # fine scroll 0..7 at the map's start and across its wrap (248..255), a new value every line;
    # SCY so that y + SCY passes 255 -> 0 inside the frame; unsigned and signed tile ids, both maps
    scx = np.where((Y // 8) & 1, 248 + (Y & 7), Y & 7)
    for nm, lcdc in (("unsigned_9800", 0x91), ("signed_9800", 0x81), ("unsigned_9c00", 0x99), ("signed_9c00", 0x89)):
        add(f"scx_fine_and_wrap_{nm}", lcdc, scx=scx, scy=250)
        add(f"scx_wrap_scy_wrap_{nm}", lcdc, scx=255 - (Y & 15), scy=184 + (Y & 1) * 7)
    # the window's first column: WX below 7, at 7, mid-tile, at the last column and past it; WY = 70
    # is above, on and below lines of the frame; the BG under it scrolls by a fine offset
    for wx in (0, 3, 6, 7, 8, 13, 159, 166, 167):
        add(f"wx_{wx}_unsigned", 0xF1, wx=wx, wy=70, scx=5, scy=3)
        add(f"wx_{wx}_signed", 0xE1, wx=wx, wy=70, scx=250, scy=251)
    add("wx_per_line_all_edges", 0xE1, wx=np.array((0, 3, 6, 7, 8, 13, 159, 166, 167))[Y % 9], wy=2, scx=Y & 7)
    # objects at both screen edges, plain and X-flipped
    xs = (0, 1, 7, 8, 9, 160, 161, 167, 168)
    add("obj_x_edges", BG_OBJ, oam=[(20 + 12 * k, x, 2 * k + 1, 0) for k, x in enumerate(xs)])
    add("obj_x_edges_xflip", BG_OBJ, oam=[(20 + 12 * k, x, 2 * k + 1, 0x20) for k, x in enumerate(xs)], scx=3)
    add("obj16_x_edges_yflip", BG_OBJ16, oam=[(18 + 14 * k, x, 2 * k + 1, 0x40 | (0x20 if k & 1 else 0)) for k, x in enumerate(xs)])
    # eleven on a line: the 11th in OAM order has the smallest X and would cover the others
    add("obj_11_on_a_line", BG_OBJ, oam=[(60, 30 + 5 * k, 2 * k + 1, 0) for k in range(10)] + [(60, 28, 0xF3, 0)])
    add("obj16_11_on_a_line", BG_OBJ16, oam=[(60, 80 - 5 * k, 2 * k + 1, 0x10 if k & 1 else 0) for k in range(10)] + [(60, 40, 0xF2, 0)])
    # equal X: the lower OAM index is on top, whatever the palettes
    add("obj_equal_x", BG_OBJ, oam=[(50, 40, 5, 0x10), (50, 40, 7, 0), (52, 44, 9, 0), (52, 40, 11, 0x10), (90, 100, SOLID + 3, 0), (90, 100, SOLID + 1, 0)])
    # attribute bit 7 over BG colour 0 and over the other colours, with BGP mapping colour 0 to
    # shade 0 and to another shade, alone and over an object drawn before
    behind = [(30 + 18 * (k // 6), 14 + 26 * (k % 6) + k // 6, 2 * k + 1, 0x80 | (0x10 if k & 1 else 0)) for k in range(24)]
    for bgp in (0xE4, 0x1B, 0x55):
        add(f"behind_bg_bgp_{bgp:02x}", BG_OBJ, vram=solid_columns_vram(), oam=behind, bgp=bgp, scx=2)
    add("behind_over_drawn_object", BG_OBJ, vram=solid_columns_vram(),
        oam=[(40, 20 + 36 * k, 2 * k + 1, 0x80) for k in range(4)] + [(42, 23 + 36 * k, 2 * k + 9, 0x10) for k in range(4)])
    # 8x16 objects Y-flipped: odd ids, both halves, clipped at the top and the bottom
    add("obj16_yflip", BG_OBJ16, oam=[(yy, 12 + 14 * k, 2 * k + 3, 0x40) for k, yy in enumerate((2, 9, 16, 17, 80, 87, 144, 152, 159))])
    # LCDC bits 0, 1 and 5 each off, over a frame that has window and objects
    pal = [(30 + 14 * (k // 6), 16 + 22 * (k % 6), 2 * k + 1, 0x10 if k & 1 else 0) for k in range(24)]
    for nm, lcdc in (("all_on", 0xF3), ("bg_off", 0xF2), ("obj_off", 0xF1), ("win_off", 0xD3)):
        add(f"lcdc_{nm}", lcdc, oam=pal, wx=90, wy=40, scx=4, bgp=0x1B)
    assert len(c) <= 64 and len({n for n, _ in c}) == len(c)
    return c


_sweep = None


def _sweep_expected():
    global _sweep
    if _sweep is None:
        cases = _sweep_cases()
        want = np.stack([ppu_spec.render_prefix(p) for _, p in cases])
        want.setflags(write=False)
        _sweep = (cases, want)
    return _sweep


def test_sweep_states_differ_where_the_rule_matters():
    """The sweep's pairs show different screens, so each of them can see its rule broken."""
    cases, want = _sweep_expected()
    idx = {n: i for i, (n, _) in enumerate(cases)}
    for a, b in (("scx_fine_and_wrap_unsigned_9800", "scx_fine_and_wrap_signed_9800"), ("wx_6_unsigned", "wx_7_unsigned"),
                 ("wx_166_unsigned", "wx_167_unsigned"), ("obj_x_edges", "obj_x_edges_xflip"),
                 ("behind_bg_bgp_e4", "behind_bg_bgp_1b"), ("lcdc_all_on", "lcdc_bg_off"), ("lcdc_all_on", "lcdc_obj_off"),
                 ("lcdc_all_on", "lcdc_win_off")):
        assert not np.array_equal(want[idx[a]], want[idx[b]]), (a, b)
    # the 11th object and the higher OAM index of an equal-X pair leave no pixel
    for name, dropped in (("obj_11_on_a_line", 10), ("obj16_11_on_a_line", 10)):
        p = cases[idx[name]][1].copy()
        p[ppu_spec.O_OAM + 4 * dropped:ppu_spec.O_OAM + 4 * dropped + 4] = 0
        assert np.array_equal(ppu_spec.render_prefix(p), want[idx[name]])


@pytest.mark.parametrize("backend", BACKENDS)
def test_edge_sweep_equals_spec(backend):
    cases, want = _sweep_expected()
    b = backend(64)
    try:
        for e, (_, p) in enumerate(cases):
            b.load(e, ppu_cases.full_state(p))
        b.render_latched()
        bad = _bad([n for n, _ in cases], b.screen()[:len(cases)], GREY[want])
        assert not bad, bad[:10]
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------
# 3. latch protocol
@pytest.mark.parametrize("backend", BACKENDS)
def test_latch_flags_are_consumed_once(backend):
    """A handle with frame_skip 0 steps without emulating: its pk_step is K2 on the flags as they
    are.  After pk_render_latched every flag K2 found set is clear, so that K2 launch and a second
    one leave a sentinel in every row; arming again draws every row again."""
    cases, want = _sweep_expected()
    b = backend(64, frame_skip=0)
    try:
        for e in range(64):
            b.load(e, ppu_cases.full_state(cases[e % len(cases)][1]))
        grey = GREY[want][[e % len(cases) for e in range(64)]]
        b.render_latched()
        assert np.array_equal(b.screen(), grey)
        for _ in range(2):                      # K2 with every flag clear, twice: no row is touched
            b.fill_screen(SENTINEL)
            b.step()
            assert (b.screen() == SENTINEL).all()
        b.render_latched()                      # flags set again: every row is drawn, none twice
        assert np.array_equal(b.screen(), grey)
        b.fill_screen(SENTINEL)
        b.step()
        assert (b.screen() == SENTINEL).all()
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------
# 4. termination flags written by K2
def _done_hostsim(render, ranges):
    """term / trunc / rew of five steps (max_episode_steps 3, no reset) through the C ABI."""
    from tests.hostsim.sim import SimEmulator, lib
    L = lib()
    vp = ctypes.c_void_p
    L.pk_step_range.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp, vp, vp]
    L.pk_set_episode_params.argtypes = [vp, ctypes.c_uint32, ctypes.c_double]
    n = 128
    emu = SimEmulator(_dummy_rom(), n, render=render, frame_skip=0)
    assert L.pk_set_episode_params(emu.h, 3, 4.0) == 0
    act = np.full(n, NOOP, np.uint8)
    out = []
    try:
        for t in range(5):
            term, trunc, rew = np.full(n, 0xCC, np.uint8), np.full(n, 0xCC, np.uint8), np.full(n, np.nan)
            if ranges:
                for e0, cnt in ((64, 64), (0, 64)):
                    assert L.pk_step_range(emu.h, e0, cnt, act.ctypes.data, rew.ctypes.data, term.ctypes.data, trunc.ctypes.data, None) == 0
            else:
                assert L.pk_step(emu.h, act.ctypes.data, None, rew.ctypes.data, term.ctypes.data, trunc.ctypes.data, None) == 0
            out.append((term, trunc, rew))
    finally:
        emu.close()
    return out


@pytest.mark.parametrize("ranges", [False, True], ids=["pk_step", "pk_step_range"])
def test_hostsim_fused_done_equals_done_kernel(ranges):
    fused, plain = _done_hostsim(True, ranges), _done_hostsim(False, ranges)
    for t in range(5):
        for a, b in zip(fused[t], plain[t]):
            assert np.array_equal(a, b)
        assert (fused[t][0] == (1 if t >= 2 else 0)).all() and (fused[t][1] == fused[t][0]).all()
        assert (fused[t][2] == 0.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [None, 64], ids=["pk_step", "pk_step_range"])
def test_gpu_vecenv_fused_done_equals_done_kernel(batch):
    """A screen-obs VecEnv with max_episode_steps 3 over a rendering emulator (K2 writes the flags) and
    over a headless one (pk_done_kernel does): the same term / trunc / rew in every step."""
    import torch
    from pokegym_amd.emulator import BatchedEmulator
    from pokegym_amd.env import VecEnv
    from pokegym_amd.testrom.game import game_rom
    n = 64 if batch is None else 128
    rom = game_rom()
    runs = []
    for render in (True, False):
        emu = BatchedEmulator(rom, n, render=render, max_episode_steps=3)
        env = VecEnv(n, emulator=emu, reward=False, max_episode_steps=3, log_interval=0, batch_size=batch)
        if batch is None:
            env.reset()
        else:
            env.async_reset()
        act = torch.full((n if batch is None else batch,), NOOP, dtype=torch.uint8, device=env.device)
        seq = []
        for t in range(7 * (1 if batch is None else 2)):
            if batch is None:
                _, rew, term, trunc, _ = env.step(act)
            else:
                _, rew, term, trunc, _, ids, _ = env.recv()
                env.send(act)
                seq.append(ids.cpu().numpy().copy())
            seq.append((term.cpu().numpy().copy(), trunc.cpu().numpy().copy(), rew.cpu().numpy().copy()))
        env.close()
        runs.append(seq)
    seen = set()
    for a, b in zip(*runs):
        if isinstance(a, tuple):
            for x, y in zip(a, b):
                assert np.array_equal(x, y)
            assert np.array_equal(a[0], a[1]) and (a[2] == 0.0).all()
            seen |= set(np.unique(a[0]).tolist())
        else:
            assert np.array_equal(a, b)
    assert seen == {0, 1}
