"""Where a frame ends: PyBoy's own frame-end facts, the oracle and K1 at every frame boundary.

The oracle (oracle/gbcore.c) and K1 (pk_step.hip) were written by the same hand, so their parity
says nothing about the convention both follow for where `tick()` returns.  The only evidence of
that convention that is independent of both is in tests/golden/ppu_states.npz: the first 9125
bytes of the 264 savestates PyBoy itself wrote for the reference, each saved at a frame end.  They
hold the CPU block (v9 bytes 5-22) and the LCD timing block (8375-8404), and in all 264:

    LY = 144, STAT mode = 1, next_stat_mode = 1, IF bit 0 (VBlank) set;
    with d = clock_target - clock and o = 456 - d (how far the last instruction ran past the
    start of line 144): o = 0 in the 202 halted states (HALT fast-forwards onto the boundary),
    o in {0, 4, 8, 12, 16} in the 62 running ones.

`check_frame_end` states this once: the four register facts; halted => o == 0; running =>
0 <= o <= Cmax - 1, Cmax the longest instruction of the documented opcode table
(tests/sm83_spec.py: 24 T-states, CALL) — the frame ends with the instruction that crosses the
boundary, which started before it.  The tests hold the fixture, the oracle, the host-simulated K1
(here) and the gfx950 K1 (tests/test_gpu_parity.py) to it at every frame end, by stepping with
frame_skip=1 so that every frame is a step end and is rendered.

A frame end with the LCD off (the frame ends on the clock alone) or off VBlank (the frame
watchdog) has no PyBoy evidence: it is skipped and counted, and at most SKIP_CAP of a ROM's
sampled frame ends may be skipped.

o % 4 == 0 (every documented instruction takes a multiple of 4 T-states, and so does the line)
is asserted on pkbench, the warp fixture, dma_wait_rom and vram_midframe_rom.  It is NOT asserted
on the fuzz ROMs: their HALT fast-forward lands on STAT mode boundaries, and the one at 250 cycles
into a line is 2 (mod 4), so the instruction stream that resumes there is offset by 2 — the oracle
shows o in {2, 6, 10, 18, 22} on fuzz_rom(3).
"""
from __future__ import annotations

import functools
import os
from collections import Counter
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import oracle

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GREY = np.array([0xFF, 0x99, 0x55, 0x00], np.uint8)

# v9 savestate offsets (oracle/gbcore.c gb_save_state)
V9_IME, V9_HALT, V9_IE, V9_IF = 17, 18, 20, 22
V9_LCDC, V9_STAT, V9_LY = 8375, 8379, 8380
V9_CLOCK, V9_TARGET, V9_NEXT_MODE = 8388, 8396, 8404
LINE_CYCLES = 456
SKIP_CAP = 0.10


@functools.lru_cache(maxsize=None)
def cmax() -> int:
    """T-states of the longest instruction in the documented opcode table (taken branches count)."""
    from tests import sm83_spec as S
    base = [S.cycles(op) for op in range(256)]
    return max(max(c[1] for c in base if c is not None), max(S.cb_cycles(op) for op in range(256)))


def frame_end_facts(state_bytes) -> dict:
    """The frame-end fields of a v9 state (or of its first 9125 bytes)."""
    s = np.frombuffer(state_bytes, np.uint8) if isinstance(state_bytes, (bytes, bytearray)) else np.asarray(state_bytes)
    le64 = lambda o: int.from_bytes(s[o:o + 8].tobytes(), "little", signed=True)
    d = le64(V9_TARGET) - le64(V9_CLOCK)
    return {"ly": int(s[V9_LY]), "stat_mode": int(s[V9_STAT]) & 3, "next_mode": int(s[V9_NEXT_MODE]),
            "if": int(s[V9_IF]), "ie": int(s[V9_IE]), "ime": int(s[V9_IME]), "halted": int(s[V9_HALT]),
            "lcd_on": bool(s[V9_LCDC] & 0x80), "d": d, "o": LINE_CYCLES - d}


def check_frame_end(facts: dict) -> list:
    """The frame-end invariants `facts` violates (empty = none)."""
    bad = []
    if facts["ly"] != 144:
        bad.append(f"LY {facts['ly']} != 144")
    if facts["stat_mode"] != 1:
        bad.append(f"STAT mode {facts['stat_mode']} != 1")
    if facts["next_mode"] != 1:
        bad.append(f"next_stat_mode {facts['next_mode']} != 1")
    if not facts["if"] & 1:
        bad.append(f"IF {facts['if']:#04x}: VBlank bit clear")
    o = facts["o"]
    if facts["halted"]:
        if o != 0:
            bad.append(f"halted with overshoot {o} != 0")
    elif not 0 <= o <= cmax() - 1:
        bad.append(f"running with overshoot {o} outside [0, {cmax() - 1}]")
    return bad


def has_evidence(facts: dict) -> bool:
    """A frame end PyBoy's states speak about: LCD on, ended by VBlank (not by the watchdog)."""
    return facts["lcd_on"] and facts["ly"] == 144


class FrameEndTally:
    """check_frame_end over many frame ends: violations, the skipped share, halted / running counts
    and the overshoot histogram of the running ones."""

    def __init__(self):
        self.sampled = self.skipped = self.halted = 0
        self.overshoot = Counter()
        self.bad = []

    def add(self, states, where):
        for e, s in enumerate(states):
            f = frame_end_facts(s)
            self.sampled += 1
            if not has_evidence(f):
                self.skipped += 1
                continue
            v = check_frame_end(f)
            if v:
                self.bad.append((where, e, v))
            if f["halted"]:
                self.halted += 1
            else:
                self.overshoot[f["o"]] += 1

    def report(self) -> str:
        return (f"sampled {self.sampled} skipped {self.skipped} ({100.0 * self.skipped / max(self.sampled, 1):.2f} %) "
                f"halted {self.halted} running {sum(self.overshoot.values())} overshoot {dict(sorted(self.overshoot.items()))}")

    def assert_ok(self, multiple_of_4: bool):
        assert not self.bad, self.bad[:4]
        assert self.sampled > 0 and self.skipped <= SKIP_CAP * self.sampled, self.report()
        if multiple_of_4:
            assert all(o % 4 == 0 for o in self.overshoot), self.report()


class OracleBatch:
    """n oracle emulators stepped in lockstep with a device (or host-simulated) batch, so that
    every step end can be compared, with any (frame_skip, release_frame)."""

    def __init__(self, rom: bytes, n: int, state: bytes | None = None):
        base = oracle.GB(rom, state)
        if state is None:
            base.power_on()
        self.gbs = [base.clone() for _ in range(n)]
        k = max(1, min(oracle.threads(), n // 8))
        self.cuts = [n * i // k for i in range(k + 1)]
        self.pool = ThreadPoolExecutor(k) if k > 1 else None

    def step(self, actions, frame_skip: int, release_frame: int):
        """One env-step of every env; returns (v9 states (n, 142610), shade screens (n, 144, 160))."""
        n = len(self.gbs)
        st = np.zeros((n, oracle.STATE_SIZE), np.uint8)
        sc = np.zeros((n, oracle.ROWS, oracle.COLS), np.uint8)

        def run(e0, e1):
            for e in range(e0, e1):
                gb = self.gbs[e]
                gb.run_action(int(actions[e]), frame_skip, release_frame)
                st[e] = np.frombuffer(gb.save_state(), np.uint8)
                sc[e] = gb.screen()

        if self.pool is None:
            run(0, n)
        else:
            for f in [self.pool.submit(run, a, b) for a, b in zip(self.cuts, self.cuts[1:])]:
                f.result()
        return st, sc

    def close(self):
        if self.pool is not None:
            self.pool.shutdown()
            self.pool = None


def warp_frame_actions(n: int, seed: int = 5):
    """The warp fixture's state and per-frame actions (144, n): the layout of the env-step tests
    (columns 0..n/2-1 the recorded actions, which walk through a door — pkbench's map load with
    the LCD off for ~5 frames — the rest seeded random), each action held for 24 one-frame steps."""
    d = np.load(os.path.join(GOLD, "warp_state.npz"))
    acts = np.random.default_rng(seed).integers(0, 9, size=(len(d["actions"]), n), dtype=np.uint8)
    acts[:, :n // 2] = d["actions"][:, None]
    return d["state"].tobytes(), np.repeat(acts, 24, axis=0)


def frame_case(name: str, n: int, frames: int | None = None):
    """(rom, start state or None, per-frame actions (frames, n), whether o % 4 == 0 is asserted)."""
    from pokegym_amd.testrom import fuzz
    from pokegym_amd.testrom.game import game_rom
    if name == "warp":
        state, acts = warp_frame_actions(n)
        return game_rom(), state, acts if frames is None else acts[:frames], True
    rom, default, seed = {"pkbench": (game_rom, 240, 40), "fuzz3": (lambda: fuzz.fuzz_rom(3), 100, 41),
                          "dma_wait": (fuzz.dma_wait_rom, 100, 42),
                          "vram_midframe": (fuzz.vram_midframe_rom, 100, 43),
                          "raster_fx": (fuzz.raster_fx_rom, 100, 44)}[name]
    acts = np.random.default_rng(seed).integers(0, 9, size=(frames or default, n), dtype=np.uint8)
    return rom(), None, acts, name != "fuzz3"


def _diff(a, b):
    return np.nonzero(np.asarray(a) != np.asarray(b))[0][:8].tolist()


# ------------------------------------------------------------------ the fixture itself ----------
def test_cmax_is_the_documented_longest_instruction():
    assert cmax() == 24


def test_pyboy_states_satisfy_the_frame_end_invariants():
    """All 264 PyBoy-written states pass check_frame_end; 202 halted / 62 running; the running ones'
    overshoots are exactly {0, 4, 8, 12, 16}; IME = 1 and IE = 0x0D in all of them, so the VBlank
    bit they hold in IF is one the CPU has yet to dispatch: tick() returns before the dispatch."""
    prefix = np.load(os.path.join(GOLD, "ppu_states.npz"))["prefix"]
    assert prefix.shape == (264, 9125)
    t = FrameEndTally()
    t.add(prefix, "fixture")
    print(t.report())
    assert t.bad == [] and t.skipped == 0
    assert (t.sampled, t.halted, sum(t.overshoot.values())) == (264, 202, 62)
    assert set(t.overshoot) == {0, 4, 8, 12, 16}
    facts = [frame_end_facts(p) for p in prefix]
    assert all(f["d"] == LINE_CYCLES for f in facts if f["halted"])
    assert all(f["ie"] == 0x0D and f["ime"] == 1 for f in facts)


def test_check_frame_end_sees_each_violation():
    """One field moved at a time on a passing state: every invariant reports."""
    prefix = np.load(os.path.join(GOLD, "ppu_states.npz"))["prefix"]
    halted = next(frame_end_facts(p) for p in prefix if p[V9_HALT])
    running = next(frame_end_facts(p) for p in prefix if not p[V9_HALT])
    assert check_frame_end(halted) == [] and check_frame_end(running) == []
    for base, change in [(halted, {"ly": 143}), (halted, {"ly": 145}), (halted, {"stat_mode": 0}),
                         (halted, {"next_mode": 2}), (halted, {"if": halted["if"] & ~1}), (halted, {"o": 4}),
                         (running, {"o": -4}), (running, {"o": cmax()})]:
        assert len(check_frame_end({**base, **change})) == 1, change
    assert check_frame_end({**running, "o": cmax() - 1}) == []


# ------------------------------------------------------------------ oracle and host-sim K1 ------
CASES = ["pkbench", "warp", "fuzz3", "dma_wait", "vram_midframe", "raster_fx"]


@functools.lru_cache(maxsize=None)
def _run_hostsim_case(name: str):
    """Oracle and host-simulated K1, 4 envs, frame_skip=1: (oracle tally, K1 tally, mismatches)."""
    from tests.hostsim.sim import SimEmulator
    n = 4
    rom, state, acts, mult4 = frame_case(name, n)
    ob = OracleBatch(rom, n, state)
    emu = SimEmulator(rom, n, state=state, frame_skip=1, release_frame=8)
    t_ref, t_k1, bad = FrameEndTally(), FrameEndTally(), []
    for t in range(len(acts)):
        ref, ref_scr = ob.step(acts[t], 1, 8)
        emu.step(acts[t])
        got, scr = emu.snapshot_range(0, n), emu.screen()
        t_ref.add(ref, t)
        t_k1.add(got, t)
        for e in range(n):
            if not np.array_equal(got[e], ref[e]) or not np.array_equal(scr[e], GREY[ref_scr[e]]):
                bad.append((t, e, _diff(got[e], ref[e])))
        if bad:
            break
    emu.close()
    ob.close()
    return t_ref, t_k1, bad, mult4


@pytest.mark.parametrize("name", CASES)
def test_every_frame_end_oracle_and_hostsim(name):
    """Every frame end of 4 envs (frame_skip=1: each frame is a step end and is rasterised, so K1
    enters with s.render set and the pend_hit / flush_lines filter and K2 run on every frame, the
    LCD-off frames of the door warp included): host-simulated K1 == oracle byte for byte and screen
    for screen, both satisfy the PyBoy frame-end invariants, at most 10 % of the frame ends lack
    evidence; o % 4 == 0 except on the fuzz ROM (module docstring)."""
    t_ref, t_k1, bad, mult4 = _run_hostsim_case(name)
    print("oracle", t_ref.report())
    print("k1    ", t_k1.report())
    assert not bad, bad[:4]
    t_ref.assert_ok(mult4)
    t_k1.assert_ok(mult4)


def test_frame_end_cases_cover_halted_and_overshooting_ends():
    """Across the ROM list both kinds of frame end are checked: halted ones, and running ones whose
    last instruction ran past the boundary (o > 0)."""
    for who in (0, 1):
        tallies = [_run_hostsim_case(name)[who] for name in CASES]
        assert sum(t.halted for t in tallies) > 0
        assert sum(c for t in tallies for o, c in t.overshoot.items() if o > 0) > 0


# ------------------------------------------------------------------ release_frame >= frame_skip -
@pytest.mark.parametrize("frame_skip,release_frame", [(1, 8), (1, 0), (2, 1), (8, 8), (9, 8), (24, 0), (24, 23),
                                                      (24, 24), (8, 200)])
def test_hostsim_frame_skip_release_frame(frame_skip, release_frame):
    """pkbench, 8 envs, random actions, host-simulated K1 vs the oracle after every step.  The
    reference releases the button at the top of loop pass i == release_frame
    (pyboy_binding.py:79-81), a pass that does not exist when release_frame >= frame_skip: the
    button then stays down into the next step."""
    from pokegym_amd.testrom.game import game_rom
    from tests.hostsim.sim import SimEmulator
    n, steps = 8, 6 if frame_skip > 2 else 24
    rom = game_rom()
    acts = np.random.default_rng(7).integers(0, 9, size=(steps, n), dtype=np.uint8)
    ob = OracleBatch(rom, n)
    emu = SimEmulator(rom, n, frame_skip=frame_skip, release_frame=release_frame)
    bad = []
    for t in range(steps):
        ref, ref_scr = ob.step(acts[t], frame_skip, release_frame)
        emu.step(acts[t])
        got, scr = emu.snapshot_range(0, n), emu.screen()
        bad += [(t, e, _diff(got[e], ref[e])) for e in range(n)
                if not np.array_equal(got[e], ref[e]) or not np.array_equal(scr[e], GREY[ref_scr[e]])]
        if bad:
            break
    emu.close()
    ob.close()
    assert not bad, bad[:4]
