"""Shared scenarios of the tile-view tests (pk_tiles_*): test_hostsim_tiles.py runs them on the
host-simulation build, test_gpu_tiles.py on the gfx950 build.  The oracle is the model of
include/pokegym_amd.h as pokegym_amd/tiles.py states it in numpy (tiles.model, tiles.key_model), which
check_model_equals_pixels pins to tests/ppu_spec.py, the project's statement of Pan Docs.
make(n, **kw) builds an emulator (frame_skip etc. as the runner chooses, make(n, rom=..., state=...)
overrides the cartridge), dev(values, dtype) a tensor on its device."""
import functools
import itertools
import os

import numpy as np

from pokegym_amd import _native
from pokegym_amd import tiles as T
from tests import ppu_cases, ppu_spec
from tests.ppu_cases import BG_OBJ, BG_OBJ16, make as state

HERE = os.path.dirname(os.path.abspath(__file__))
N = 130                 # two full 64-env groups and a part of a third
SENTINEL = 0x1234       # no id (<= 383) and, with a key of 0x5A5A..., no value a test expects
KEY_SENTINEL = 0x5A5A5A5A5A5A5A5A
MODES = [("id", 12), ("hash", 8), ("hash", 15)]


# ------------------------------------------------------------------------------------------------
# 1. the model against the independent pixel statement (CPU only)
def paint(plane, vram, bgp):
    """Plane 0 of an id-mode view painted back to 144 x 160 shade ids through the tile data and BGP;
    "nothing" is shade 0."""
    ids = np.repeat(np.repeat(plane.astype(np.int64), 8, axis=0), 8, axis=1)
    none = ids == T.NONE
    y, x = np.arange(144)[:, None], np.arange(160)[None, :]
    a = np.where(none, 0, ids) * 16 + 2 * (y & 7)
    v = np.asarray(vram, np.uint8).astype(np.int64)
    bit = 7 - (x & 7)
    colour = ((v[a] >> bit) & 1) | (((v[a + 1] >> bit) & 1) << 1)
    return np.where(none, 0, (int(bgp) >> (2 * colour)) & 3).astype(np.uint8)


def aligned_cases():
    """(name, prefix): no objects, per-line parameters constant, SCX, SCY, WY and WX - 7 multiples of 8:
    both tile-data modes, both maps for both layers, window on and off, WX = 7 and above, the wrap at
    map column and row 31; LCDC.0 = 0 (window off: tests/ppu_spec.py keeps PyBoy's window without a
    background) and the LCD off with no layer enabled (ppu_spec does not model LCDC.7)."""
    out = []
    scrolls = ((0, 0, 7, 0), (200, 136, 87, 40), (248, 248, 7 + 8 * 19, 8 * 17), (8, 16, 7, 72))
    for td, bgmap, winmap, win in itertools.product((0, 1), repeat=4):
        lcdc = 0x83 | td << 4 | bgmap << 3 | winmap << 6 | win << 5
        for scx, scy, wx, wy in scrolls:
            out.append((f"lcdc_{lcdc:02x}_scx{scx}_scy{scy}_wx{wx}_wy{wy}",
                        state(lcdc, scx=scx, scy=scy, wx=wx, wy=wy, bgp=0x1B if td else 0xE4)))
    out.append(("bg_off", state(0x92, scx=16, scy=8)))
    out.append(("bg_off_map_bits", state(0xDA, scx=16, scy=8, wx=47, wy=8)))
    out.append(("lcd_off_no_layer", state(0x58, scx=16, scy=8)))
    return out


def check_model_equals_pixels():
    """Plane 0 of tiles.model (id mode), painted through the tile data and BGP, is tests/ppu_spec.py's
    frame on every pixel, for every aligned case; a window case differs from its window-off twin, so
    the layer rule is seen.  LCD off with every layer enabled is all "nothing"."""
    seen_window = seen_signed = 0
    for name, p in aligned_cases():
        vram, oam, lcdc, bgp, obp0, obp1, params = ppu_spec.split_prefix(p)
        scx, scy, wx, wy = (int(params[0, k]) for k in range(4))
        view = T.model(vram, oam, lcdc, scy, scx, wy, wx, mode="id", obj=False)
        assert view.shape == (1, 18, 20) and view.dtype == np.uint16
        want = ppu_spec.render(vram, oam, lcdc, bgp, obp0, obp1, params)
        got = paint(view[0], vram, bgp)
        assert np.array_equal(got, want), (name, int((got != want).sum()))
        if lcdc & 1:
            assert (view != T.NONE).all() and int(view.max()) <= 383
            seen_signed += int((view >= 256).any())
            if lcdc & 0x20 and wy < 144:
                off = T.model(vram, oam, lcdc & ~0x20, scy, scx, wy, wx, mode="id", obj=False)
                seen_window += int(not np.array_equal(off, view))
        else:
            assert (view == T.NONE).all(), name
    assert seen_window >= 16 and seen_signed >= 16
    p = state(0x7F, scx=8)
    vram, oam, lcdc, _, _, _, params = ppu_spec.split_prefix(p)
    assert (T.model(vram, oam, lcdc, 0, 8, 0, 7) == T.NONE).all()


# ------------------------------------------------------------------------------------------------
# 2. the states of the kernel-vs-model comparison
OBJ_YS = (0, 4, 8, 12, 16, 152, 159, 160)
OBJ_XS = (0, 4, 8, 164, 167, 168)


def edge_cases():
    """States beyond tests/ppu_cases.py: arbitrary (unaligned) scroll and window positions with random
    objects; WX in {0, 6, 7, 166, 167} x WY in {0, 143, 144}; objects on every (Y, X) of OBJ_YS x OBJ_XS,
    8 x 8 and 8 x 16 with and without Y flip (a half on the grid and a half off at Y = 4, 8, 152);
    several objects in one cell, with equal X and with the smaller X later in OAM."""
    c = []

    def add(name, lcdc, **kw):
        c.append((name, state(lcdc, **kw)))

    for k in range(28):
        rng = np.random.default_rng(0x711E + k)
        scx, scy, wx, wy = (int(v) for v in rng.integers(0, 256, 4))
        if k & 1:
            wx, wy = int(rng.integers(0, 168)), int(rng.integers(0, 144))
        add(f"unaligned_{k:02d}", 0x80 | int(rng.integers(0, 128)), vram=rng.integers(0, 256, 8192, dtype=np.uint8),
            oam=ppu_cases._random_oam(rng), scx=scx, scy=scy, wx=wx, wy=wy)
    for (wx, wy), lcdc in zip(itertools.product((0, 6, 7, 166, 167), (0, 143, 144)), itertools.cycle((0xF3, 0xE3, 0xB3))):
        add(f"wx_{wx}_wy_{wy}", lcdc, wx=wx, wy=wy, scx=5, scy=3)
    spots = [(y, x) for y in OBJ_YS for x in OBJ_XS]
    for nm, lcdc, attr in (("obj8", BG_OBJ, 0x00), ("obj16", BG_OBJ16, 0x00), ("obj16_yflip", BG_OBJ16, 0x40),
                           ("obj16_mixed_flip", BG_OBJ16, None)):
        for half, part in (("a", spots[:40]), ("b", spots[-40:])):
            add(f"{nm}_edges_{half}", lcdc, scx=3,
                oam=[(y, x, (7 * i + 2) & 0xFF, (0x40 if i % 3 == 0 else 0x20) if attr is None else attr)
                     for i, (y, x) in enumerate(part)])
    crowd = [(50, 64, 5, 0), (50, 60, 9, 0), (50, 60, 7, 0), (52, 67, 11, 0x40), (100, 30, 0x21, 0), (100, 30, 0x32, 0x40),
             (96, 31, 0x43, 0), (101, 28, 0x54, 0x40), (100, 28, 0x65, 0)]
    add("obj8_one_cell", BG_OBJ, oam=crowd)
    add("obj16_one_cell", BG_OBJ16, oam=crowd)
    add("obj16_one_cell_reversed", BG_OBJ16, oam=crowd[::-1])
    add("obj_on_lcd_off", 0x13, oam=crowd)
    add("obj_off", 0x91, oam=crowd)
    assert len({n for n, _ in c}) == len(c)
    return c


@functools.lru_cache(maxsize=None)
def all_states():
    """(names, prefixes uint8 (k, PREFIX)): tests/ppu_cases.py's directed and random cases, then edge_cases()."""
    cases = list(ppu_cases.all_cases()) + edge_cases()
    pre = np.stack([p for _, p in cases])
    pre.setflags(write=False)
    return tuple(n for n, _ in cases), pre


def _regs(pre):
    """(vram, oam, lcdc, scy, scx, wy, wx) of state prefixes, as load_env installs them."""
    r = pre[:, ppu_spec.O_REGS:ppu_spec.O_REGS + 11].astype(np.int64)
    return (pre[:, ppu_spec.O_VRAM:ppu_spec.O_VRAM + 8192], pre[:, ppu_spec.O_OAM:ppu_spec.O_OAM + 160],
            r[:, 0], r[:, 7], r[:, 8], r[:, 9], r[:, 10])


@functools.lru_cache(maxsize=None)
def expected(mode, bits, obj=True):
    """The model's view of every state of all_states(), computed once a process."""
    v = T.model(*_regs(all_states()[1]), mode=mode, bits=bits, obj=obj)
    v.setflags(write=False)
    return v


def check_states_reach_the_rules():
    """With the model alone: the states tell each single rule from its nearest wrong version — the window
    column's + 7, the signed-addressing fold, the Y flip of 8 x 16 objects and priority by X before the
    index — which is what the mutation check of DESIGN.md 7m relies on."""
    names, pre = all_states()
    vram, oam, lcdc, scy, scx, wy, wx = _regs(pre)
    want = expected("id", 12)
    assert len(names) == len(want) and want.shape[1:] == (2, 18, 20)
    win = ((lcdc & 0xA1) == 0xA1) & (wx <= 166) & (wy < 144)
    assert (win & (wx % 8 != 7)).sum() >= 20
    assert (((lcdc & 0x91) == 0x81) & (want[:, 0] >= 256).any(axis=(1, 2))).sum() >= 20
    unflipped = T.model(vram, oam & np.tile(np.array([0xFF, 0xFF, 0xFF, 0xBF], np.uint8), 40), lcdc, scy, scx, wy, wx)
    assert (unflipped != want).any(axis=(1, 2, 3)).sum() >= 10
    by_index = 0
    for e in np.nonzero((lcdc & 0x82) == 0x82)[0]:
        o = oam[e].reshape(40, 4).astype(np.int64)
        first = {}
        for i in range(40):
            r, c = (o[i, 0] - 12) >> 3, (o[i, 1] - 4) >> 3
            for rr in ((r, r + 1) if lcdc[e] & 4 else (r,)):
                if 0 <= rr < 18 and 0 <= c < 20:
                    first.setdefault((rr, c), []).append((o[i, 1], i))
        by_index += any(min(v) != v[0] for v in first.values())
    assert by_index >= 20
    assert (want[:, 1] != T.NONE).any(axis=(1, 2)).sum() >= 100


def load_round(emu, ids, rev):
    """State ids[i] into env i (rev: env n - 1 - i), so a state meets different lanes and interleave rows."""
    _, pre = all_states()
    for i, s in enumerate(ids):
        emu.load_env(emu.n - 1 - i if rev else i, ppu_cases.full_state(pre[s]))


def keys_of(t):
    return t.cpu().numpy().view(np.uint64)


def view_of(emu):
    return emu.tiles.cpu().numpy().view(np.uint16)


def check_kernel_equals_model(make, dev, mode, bits):
    """Every state of all_states(), N envs at a time with no two lanes alike, a second time in reversed
    env order: every u16 of both planes and every key, unsalted and salted, is the model's, bit for bit."""
    names, pre = all_states()
    want = expected(mode, bits)
    emu = make(N)
    emu.tiles_create(mode, bits, True)
    assert emu.tile_planes == 2 and tuple(emu.tiles.shape) == (N, 2, 18, 20)
    assert (view_of(emu) == T.NONE).all()
    order = np.random.default_rng(0x7153).permutation(len(names))
    rounds = [order[i:i + N] for i in range(0, len(order), N)]
    rounds[-1] = order[-N:]
    rng = np.random.default_rng(9)
    for k, ids in enumerate(rounds):
        rev = bool(k & 1)
        load_round(emu, ids, rev)
        at = ids[::-1] if rev else ids
        keys = dev(np.full(N, KEY_SENTINEL, np.uint64).view(np.int64), np.int64)
        emu.tiles_eval(keys=keys)
        got = view_of(emu)
        bad = [(names[s], int((got[e] != want[s]).sum())) for e, s in enumerate(at) if not np.array_equal(got[e], want[s])]
        assert not bad, bad[:10]
        assert np.array_equal(keys_of(keys), T.key_model(want[at]))
        salt = rng.integers(0, 1 << 63, N, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        salt[::17] = np.uint64(0xFFFFFFFFFFFFFFFF)                       # "no cell" passes through
        salt[1::17] = 0
        keys = dev(salt.copy().view(np.int64), np.int64)                 # a copy: on the host build dev() wraps the array
        emu.tiles_eval(salt=keys, keys=keys)                             # in place: salt_dev may be keys_dev
        assert np.array_equal(keys_of(keys), T.key_model(want[at], salt))
    emu.close()
    one = make(64)                                                       # one plane: the key covers 360 values
    one.tiles_create(mode, bits, False)
    assert one.tile_planes == 1 and tuple(one.tiles.shape) == (64, 1, 18, 20)
    load_round(one, order[:64], False)
    keys = dev(np.zeros(64, np.int64), np.int64)
    one.tiles_eval(keys=keys)
    assert np.array_equal(view_of(one)[:, 0], want[order[:64], 0])
    assert np.array_equal(keys_of(keys), T.key_model(want[order[:64], :1]))
    one.close()


# ------------------------------------------------------------------------------------------------
# 3. ranges and masks
def check_ranges_and_masks(make, dev, n=192):
    """Output and keys prefilled with a sentinel: a call over [64, 128) with a random mask changes the
    participants only; an all-zero mask and count = 0 (refused, as for every ranged call) write nothing;
    a last partial range works."""
    names, pre = all_states()
    want = expected("id", 12)
    emu = make(n)
    emu.tiles_create("id", 12, True)
    ids = np.random.default_rng(77).permutation(len(names))[:n]
    load_round(emu, ids, False)
    L, h = emu._L, emu._h

    def prefill():
        emu.tiles.fill_(SENTINEL)
        return dev(np.full(n, KEY_SENTINEL, np.uint64).view(np.int64), np.int64)

    def same(keys, took):
        got, k = view_of(emu), keys_of(keys)
        assert np.array_equal(got[took], want[ids][took]) and (got[~took] == SENTINEL).all()
        assert np.array_equal(k[took], T.key_model(want[ids])[took]) and (k[~took] == KEY_SENTINEL).all()

    rng = np.random.default_rng(5)
    mask = rng.integers(0, 2, n).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)
    took = np.zeros(n, bool)
    took[64:128] = mask[64:128] != 0
    assert 8 < took.sum() < 56
    keys = prefill()
    emu.tiles_eval(dev(mask, np.uint8), keys=keys, env0=64, count=64)
    same(keys, took)
    keys = prefill()
    emu.tiles_eval(dev(np.zeros(n, np.uint8), np.uint8), keys=keys)
    same(keys, np.zeros(n, bool))
    assert L.pk_tiles_eval(h, None, None, keys.data_ptr(), 0, 0, None) < 0
    assert "env range [0, +0)" in L.pk_last_error().decode(errors="replace")
    same(keys, np.zeros(n, bool))
    emu.tiles_eval(keys=keys, env0=128, count=n - 128 - 7)               # ends inside a 16-env workgroup
    took[:] = False
    took[128:n - 7] = True
    same(keys, took)
    emu.tiles_eval(env0=0, count=64)                                     # without keys
    took[:64] = True
    assert np.array_equal(view_of(emu)[took], want[ids][took]) and (view_of(emu)[~took] == SENTINEL).all()
    emu.close()


def actions(steps, n, seed):
    return np.random.default_rng(seed).integers(0, 9, size=(steps, n), dtype=np.uint8)


def model_of(emu, mode, bits, obj=True, env0=0, count=None):
    """The model applied to the machine state read back through snapshot."""
    return T.from_states(emu.snapshot_range(env0, emu.n - env0 if count is None else count), mode=mode, bits=bits, obj=obj)


def check_headless_equals_reward_handle(make, dev, n=64):
    """A headless handle (render=False) and a reward-stack handle fed the same actions show the same
    view, which is the model's of their state."""
    a, b = make(n, render=False), make(n, reward=True)
    acts = actions(3, n, 23)
    for emu in (a, b):
        emu.tiles_create("hash", 12, True)
        emu.reset()
        for t in range(3):
            emu.step(dev(acts[t], np.uint8))
        emu.tiles_eval()
    va, vb = view_of(a), view_of(b)
    assert np.array_equal(va, vb) and np.array_equal(va, model_of(a, "hash", 12))
    assert (va[:, 0] != T.NONE).any()
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------
# 4. the view follows the game
def warp_case(n):
    """The door-warp fixture: its state and six env-steps of actions, columns 0..n/2-1 the recorded ones
    (they walk through a door: a map load with the LCD off), the rest seeded random."""
    d = np.load(os.path.join(HERE, "golden", "warp_state.npz"))
    acts = actions(len(d["actions"]), n, 5)
    acts[:, :n // 2] = d["actions"][:, None]
    return d["state"].tobytes(), acts


def check_follows_the_game(make_game, dev, oracle_states=None, n=64):
    """pkbench from the warp fixture, 64 envs, six env-steps: after every step `tiles` (id mode, with
    keys) is the model of the state read back through snapshot; the walking envs' views change, the
    door's LCD-off step shows "nothing", and the view after it is another map's.  oracle_states(rom,
    state, acts): the oracle's v9 states after the same actions, compared as well (the GPU runner)."""
    from pokegym_amd.testrom.game import game_rom
    start, acts = warp_case(n)
    emu = make_game(n, start)
    emu.tiles_create("id", 12, True)
    keys = dev(np.zeros(n, np.int64), np.int64)
    views = []
    for t in range(len(acts)):
        emu.step(dev(acts[t], np.uint8))
        emu.tiles_eval(keys=keys)
        want = model_of(emu, "id", 12)
        assert np.array_equal(view_of(emu), want), t
        assert np.array_equal(keys_of(keys), T.key_model(want)), t
        views.append(want)
    assert len({v[0].tobytes() for v in views}) >= 3                     # the recorded env's view moves
    assert (views[-1][:, 0] != T.NONE).all() and (views[-1][:, 1] != T.NONE).any()
    assert len({v.tobytes() for v in views[-1]}) > 4                     # the random envs diverge
    if oracle_states is not None:
        ref = oracle_states(game_rom(), start, acts)
        assert np.array_equal(views[-1], T.from_states(ref))
    emu.close()


def check_vecenv(make_env, dev, pipeline, n=64):
    """VecEnv(n, batch_size=n/2, tile_view="hash") on a headless emulator: tile_obs() after step(), and
    after every recv() of the pipeline, is the model of the envs' states; reset() and load_state()
    evaluate the envs they replace."""
    env = make_env(n, reward=False, render=False, tile_view="hash", tile_bits=10)
    emu = env.emu
    assert emu.tile_planes == 2 and tuple(env.tile_space.shape) == (2, 18, 20)
    acts = actions(5, n, 31)

    def want(sl=slice(None)):
        full = model_of(emu, "hash", 10)
        return full[env.phys(np.arange(n))][sl]

    if pipeline:
        env.async_reset()
        assert np.array_equal(env.tile_obs().cpu().numpy().view(np.uint16), want())
        for t in range(5):
            for _ in range(env.num_batches):
                env.recv()
                sl = env.current_envs()
                got = env.tile_obs().cpu().numpy().view(np.uint16)
                assert got.shape[0] == n // 2 and np.array_equal(got, want(sl)), t
                env.send(dev(acts[t, sl], np.uint8))
        env._join_streams()
    else:
        env.reset()
        assert np.array_equal(env.tile_obs().cpu().numpy().view(np.uint16), want())
        for t in range(5):
            env.step(dev(acts[t], np.uint8))
            assert np.array_equal(env.tile_obs().cpu().numpy().view(np.uint16), want()), t
        first = env.tile_obs().cpu().numpy().copy()
        assert len({v.tobytes() for v in first}) > 1
        env.load_state(n - 1, env.save_state(0))
        got = env.tile_obs().cpu().numpy()
        assert np.array_equal(got[n - 1], first[0]) and np.array_equal(got[:n - 1], first[:n - 1])
        env.reset()
        assert np.array_equal(env.tile_obs().cpu().numpy().view(np.uint16), want())
    emu.close()


def check_archive_key(make_env, dev, n=64):
    """archive_key="tiles": envs with equal views share a cell, an env whose background has scrolled by
    8 pixels gets another; resume_from_bank re-evaluates the env it replaced."""
    env = make_env(n, reward=True, tile_view="id", bank_episodes=True, bank_slots=1, archive_cells=4,
                   archive_key="tiles", novelty_log2=10, novelty_key="tiles")
    env.reset()
    for _ in range(6):                                                   # the same machine in every env, its map loaded
        env.step(dev(np.full(n, 8, np.uint8), np.uint8))
    st = bytearray(env.save_state(0))
    scx = 8375 + 8
    st[scx] = (st[scx] + 8) & 0xFF
    env.load_state(2, bytes(st))
    view = env.tile_obs().cpu().numpy()
    assert np.array_equal(view[0], view[1]) and not np.array_equal(view[0, 0], view[2, 0])
    assert np.array_equal(view[2, 0, :, :-1], view[0, 0, :, 1:])        # one tile column to the left
    keys = env.cell_keys().cpu().numpy().view(np.uint64)
    assert np.array_equal(keys, T.key_model(view.view(np.uint16)))
    assert keys[0] == keys[1] and keys[2] != keys[0] and len(np.unique(keys)) == 2
    won = env.archive_update().cpu().numpy()
    cells = env.emu.archive_read()
    assert cells["used"] == 2 and set(cells["keys"][:2].tolist()) == {int(keys[0]), int(keys[2])}
    assert (won >= 0).sum() == 2 and won[2] >= 0
    env.checkpoint_to_bank([2], [0])
    env.resume_from_bank([5], [0])
    got = env.tile_obs().cpu().numpy()
    assert np.array_equal(got[5], view[2]) and np.array_equal(got[4], view[0])
    env.step(dev(np.full(n, 8, np.uint8), np.uint8))                     # the novelty key is the tile key
    nk = env.novelty_keys.cpu().numpy().view(np.uint64)
    assert nk[0] == nk[1] and nk[2] != nk[0]
    env.emu.close()


# ------------------------------------------------------------------------------------------------
# 5. lifecycle
def check_lifecycle(make, dev, n=64):
    """Every rejected call is a negative code with its own message and changes nothing; a handle on
    which creates failed still takes a correct one."""
    emu = make(n)
    L, h = emu._L, emu._h

    def said(text):
        return text in L.pk_last_error().decode(errors="replace")

    assert L.pk_tiles_planes(h) == 0 and not L.pk_tiles_ptr(h) and emu.tiles is None and emu.tile_planes == 0
    assert L.pk_tiles_eval(h, None, None, None, 0, n, None) < 0 and said("no tile view")
    assert L.pk_tiles_create(h, 2, 12, 1) < 0 and said("unknown tile view mode 2")
    for bits in (0, 7, 16, 64):
        assert L.pk_tiles_create(h, _native.PK_TILES_HASH, bits, 1) < 0 and said("bits in 8..15, not %u" % bits)
    assert L.pk_tiles_create(h, _native.PK_TILES_ID, 12, 2) < 0 and said("unknown flags 0x2")
    assert L.pk_tiles_create(None, 0, 12, 1) < 0 and said("null handle")
    assert L.pk_tiles_planes(h) == 0 and not L.pk_tiles_ptr(h)
    for bad in (dict(mode="ids"), dict(mode="hash", bits=7), dict(mode="hash", bits=16)):
        try:
            emu.tiles_create(**bad)
        except (ValueError, _native.PkError):
            pass
        else:
            raise AssertionError(bad)
    assert emu.tile_planes == 0
    emu.tiles_create("id", 0, False)                                     # id mode ignores bits
    assert L.pk_tiles_planes(h) == 1 and L.pk_tiles_ptr(h)
    assert L.pk_tiles_create(h, 0, 12, 1) < 0 and said("already has a tile view of 1 planes")
    assert L.pk_tiles_planes(h) == 1
    for env0, count in ((32, 8), (0, n + 1), (n, 1), (0, 0)):
        assert L.pk_tiles_eval(h, None, None, None, env0, count, None) < 0 and said("env range [%u, +%u)" % (env0, count))
    assert (view_of(emu) == T.NONE).all()
    emu.reset()
    emu.tiles_eval()
    assert np.array_equal(view_of(emu), model_of(emu, "id", 12, obj=False))
    emu.close()


BAD_KEYWORDS = ({"tile_view": "ids"}, {"tile_view": "hash", "tile_bits": 7}, {"tile_view": "hash", "tile_bits": 16},
                {"archive_key": "tiles"}, {"novelty_key": "tiles", "novelty_log2": 10})


def check_vecenv_off(make_env, dev, n=64):
    """tile_view=None: no view, no calls."""
    env = make_env(n, reward=False)
    assert env.emu.tile_planes == 0 and env.tile_view is None and env.tile_space is None

    def forbidden(*a, **k):
        raise AssertionError("tile_view=None must not call the tile entry points")

    env.emu.tiles_eval = env.emu.tiles_create = forbidden
    try:
        env.tile_obs()
    except RuntimeError:
        pass
    else:
        raise AssertionError("tile_obs() without tile_view")
    env.reset()
    env.step(dev(np.full(n, 8, np.uint8), np.uint8))
    env.emu.close()
