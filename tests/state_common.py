"""Shared runner of the injected-state cases (tests/state_cases.py) — TEST INFRASTRUCTURE ONLY.

Case i of a launch is loaded into env i; K1 (host-simulated in tests/test_hostsim_states.py, the
gfx950 build in tests/test_gpu_states.py) and a per-case oracle.GB are stepped side by side:
3 steps of one rendered frame each (frame_skip 1, release 0), then from fresh loads 2 steps of 24
frames (release 8).  After every step the whole v9 state and the screen must be equal, bit for bit;
the oracle side is computed once per process and kept as digests (about 1,500 cases x 5 snapshots).
"""
from __future__ import annotations

import functools
import hashlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from pokegym_amd.testrom import stage as ST
from tests import state_cases as SC

RUNS = ((1, 0, 3), (24, 8, 2))      # (frame_skip, release_frame, steps)
MAX_ENVS = 512
GREY = np.array([0xFF, 0x99, 0x55, 0x00], np.uint8)


def _digest(state: bytes, screen: np.ndarray) -> bytes:
    h = hashlib.blake2b(state, digest_size=16)
    h.update(np.ascontiguousarray(screen).tobytes())
    return h.digest()


def oracle_run(case, run):
    """[(state, grey screen)] after every step of RUNS[run] from the case's state."""
    from oracle import oracle as O
    name, n_banks, state, action, _ = case
    fs, rel, steps = RUNS[run]
    gb = O.GB(ST.stage_rom(n_banks).rom, state)
    out = []
    for _ in range(steps):
        gb.run_action(action, fs, rel)
        out.append((gb.save_state(), GREY[gb.screen()]))
    return out


@functools.lru_cache(maxsize=None)
def reference() -> dict:
    """{case name: (digests of run 0's steps, digests of run 1's steps)}"""
    cases = SC.all_cases()

    def one(c):
        return c[0], tuple(tuple(_digest(s, scr) for s, scr in oracle_run(c, r)) for r in range(len(RUNS)))

    with ThreadPoolExecutor(8) as ex:
        return dict(ex.map(one, cases))


def launches(cases, n_banks, reverse=False):
    """The cases of one ROM variant in launches of at most MAX_ENVS envs (reverse: env order reversed,
    so that the neighbours of a wave differ)."""
    sel = [c for c in cases if c[1] == n_banks]
    if reverse:
        sel = sel[::-1]
    return [sel[i:i + MAX_ENVS] for i in range(0, len(sel), MAX_ENVS)]


def run_launch(make, batch, after_step=None):
    """make(rom, n, frame_skip, release_frame) -> an emulator adapter with load(states), step(actions),
    snapshots() -> (n, V9) uint8, screens() -> (n, 144, 160), close(); after_step(run, step) is called
    after every step.  Returns the failures:
    (case name, run, step, first differing v9 offsets)."""
    ref = reference()
    rom = ST.stage_rom(batch[0][1]).rom
    acts = np.array([c[3] for c in batch], np.uint8)
    bad = []
    for r, (fs, rel, steps) in enumerate(RUNS):
        emu = make(rom, len(batch), fs, rel)
        try:
            emu.load([c[2] for c in batch])
            alive = np.ones(len(batch), bool)
            for t in range(steps):
                emu.step(acts)
                if after_step:
                    after_step(r, t)
                snaps, scr = emu.snapshots(), emu.screens()
                for i, c in enumerate(batch):
                    if alive[i] and _digest(snaps[i].tobytes(), scr[i]) != ref[c[0]][r][t]:
                        alive[i] = False
                        want, wscr = oracle_run(c, r)[t]
                        idx = np.nonzero(snaps[i] != np.frombuffer(want, np.uint8))[0]
                        bad.append((c[0], r, t, idx[:6].tolist(), int((scr[i] != wscr).sum())))
        finally:
            emu.close()
    return bad


# ---- adapters ----
class SimAdapter:
    def __init__(self, rom, n, fs, rel):
        from tests.hostsim.sim import SimEmulator
        self.emu = SimEmulator(rom, n, frame_skip=fs, release_frame=rel)
        self.n = n

    def load(self, states):
        for i, s in enumerate(states):
            self.emu.load_env(i, s)

    def step(self, acts):
        self.emu.step(acts)

    def snapshots(self):
        return self.emu.snapshot_range(0, self.n)

    def screens(self):
        return self.emu.screen()

    def close(self):
        self.emu.close()


class GpuAdapter:
    """The product's BatchedEmulator; states go in through the savestate bank (one slot per env)."""

    def __init__(self, rom, n, fs, rel):
        import torch
        from pokegym_amd.emulator import BatchedEmulator
        self.torch = torch
        self.emu = BatchedEmulator(rom, n, frame_skip=fs, release_frame=rel, render=True)
        self.n = n

    def load(self, states):
        self.emu.bank_create(self.n)
        for i, s in enumerate(states):
            self.emu.bank_put(i, s)
        self.emu.bank_load(self.torch.arange(self.n, dtype=self.torch.int32, device=self.emu.device))

    def step(self, acts):
        self.emu.step(self.torch.from_numpy(acts).to(self.emu.device))

    def snapshots(self):
        return self.emu.snapshot_range(0, self.n)

    def screens(self):
        self.torch.cuda.synchronize()
        return self.emu.screen.cpu().numpy()

    def close(self):
        self.emu.close()
