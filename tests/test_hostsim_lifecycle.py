"""The host layer's lifecycle on the CPU (tests/hostsim): who owns device memory, what a failed
allocation leaves behind, and which launches a reset or a bank call issues.

Three scripts of C ABI calls build a handle with every feature that allocates.  For every call of
every script, and for every k below the number of hipMalloc calls it makes on a clean run, the
k-th allocation is made to fail: the call must fail with a message, free everything it allocated,
leave its feature absent (or, for the grow of pk_set_episode_params, unchanged), succeed when it
is made again, and the rest of the script must run; after pk_destroy nothing is live.

The launch pin records the kernel name, grid and block of every launch and the byte count of
every hipMemsetAsync of the reset and bank entry points and compares them with
tests/golden/capi_launch_sequences.json (`python tests/test_hostsim_lifecycle.py --record`
rewrites it)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hostsim"))
sys.path.insert(0, HERE)
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))

import sim  # noqa: E402
from pokegym_amd import _native  # noqa: E402
from pokegym_amd.testrom.game import game_rom  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "capi_launch_sequences.json")
N, MAX_STEPS, SLOTS = 64, 100, 4
GROW_TO = 800          # cap_log2 10 -> 11: (1 << 10) * 3 < (800 + 2) * 4
F_RENDER, F_REWARD = _native.PK_F_RENDER, _native.PK_F_REWARD


def lib():
    L = sim.lib()
    _native.bind(L)
    L.pk_sim_alloc_live.restype = ctypes.c_int64
    L.pk_sim_alloc_calls.restype = ctypes.c_int64
    L.pk_sim_alloc_fail_at.argtypes = [ctypes.c_int64]
    L.pk_sim_alloc_fail_at.restype = None
    L.pk_sim_record_enable.argtypes = [ctypes.c_int]
    L.pk_sim_record_enable.restype = None
    L.pk_sim_record_get.argtypes = [ctypes.c_char_p, ctypes.c_uint64]
    L.pk_sim_record_get.restype = ctypes.c_uint64
    return L


class Ctx:
    """One handle and the host arrays its calls read and write (device memory is host memory)."""

    def __init__(self, reward, n=N):
        self.L, self.reward, self.n = lib(), reward, n
        self.h = ctypes.c_void_p()
        self.rom = np.frombuffer(game_rom(), np.uint8).copy()
        self.rew, self.term, self.trunc = np.zeros(n), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        self.t = 0

    def traj(self):
        cap = self.L.pk_traj_capacity(self.h)
        origin, length = np.zeros(self.n, np.int32), np.zeros(self.n, np.uint32)
        flags, acts = np.zeros(self.n, np.uint8), np.zeros((self.n, cap), np.uint8)
        assert acts.ctypes.data % 16 == 0
        rc = self.L.pk_traj_get(self.h, 0, self.n, origin.ctypes.data, length.ctypes.data, flags.ctypes.data,
                                acts.ctypes.data, None)
        assert rc == 0, self.L.pk_last_error()
        return origin, length, flags, acts


def slots_of(c, mapping):
    s = np.full(c.n, -1, np.int32)
    for e, k in mapping.items():
        s[e] = k
    return s


def create(c):
    cfg = _native.PkConfig()
    cfg.n_envs = c.n
    cfg.rom = c.rom.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    cfg.rom_len = len(c.rom)
    cfg.frame_skip, cfg.release_frame, cfg.max_episode_steps = 2, 1, MAX_STEPS
    cfg.flags = F_RENDER | (F_REWARD if c.reward else 0)
    cfg.reward_scale = 4.0
    c.h = ctypes.c_void_p(1)                 # a failed pk_create must null it
    return c.L.pk_create(ctypes.byref(cfg), ctypes.byref(c.h))


def step(c):
    acts = ((np.arange(c.n) * 5 + c.t * 3) % 8).astype(np.uint8)
    c.t += 1
    return c.L.pk_step(c.h, acts.ctypes.data, None, c.rew.ctypes.data, c.term.ctypes.data, c.trunc.ctypes.data, None)


def steps(c):
    """A few steps with a checkpoint of envs 3 and 20 and a resume of them in envs 9 and 21 (the first
    32 envs: one sub-block of the bank's image mover, the simulation's slowest launch here)."""
    save, load = slots_of(c, {3: 0, 20: 1}), slots_of(c, {9: 0, 21: 1})
    rc = step(c) or c.L.pk_bank_checkpoint(c.h, save.ctypes.data, 0, 32, None)
    rc = rc or step(c) or c.L.pk_bank_resume(c.h, load.ctypes.data, 0, 32, None)
    return rc or step(c)


def probes(c):
    prog = (_native.PkProbe * 2)()
    for j, (addr, op) in enumerate(((0xD361, 1), (0xFF80, 3))):       # a delta and a change probe
        p = prog[j]
        p.addr, p.len, p.count, p.stride, p.kind, p.reduce, p.op, p.cmp, p.arg, p.weight = addr, 1, 1, 0, 0, 0, op, 0, 0, 1.0
    return c.L.pk_probe_create(c.h, prog, 2)


def destroy(c):
    c.L.pk_destroy(c.h)
    c.h = ctypes.c_void_p()
    return 0


def grow_probe(c):
    """What a failed grow must leave alone: the rows pk_traj_get returns, and a step."""
    before = c.traj()

    def check():
        for a, b in zip(before, c.traj()):
            assert np.array_equal(a, b)
        assert step(c) == 0, c.L.pk_last_error()
    return check


def absent(query, value=0):
    return lambda c: (lambda: _same(getattr(c.L, query)(c.h), value, query))


def _same(got, want, what):
    assert got == want, (what, got, want)


# a call of a script: its name, the call (returns the ABI's code), and a function that, called before
# the armed call, returns the check to make after it has failed
CALLS = {
    "create": (create, lambda c: (lambda: _same(c.h.value, None, "*out"))),
    "bank": (lambda c: c.L.pk_bank_create(c.h, SLOTS), absent("pk_bank_slots")),
    "traj": (lambda c: c.L.pk_traj_enable(c.h), absent("pk_traj_capacity")),
    "episodes": (lambda c: c.L.pk_bank_enable_episodes(c.h), absent("pk_bank_has_episodes")),
    "generic": (lambda c: c.L.pk_bank_enable_generic_episodes(c.h, _native.PK_GEP_PROBES | _native.PK_GEP_STACK),
                absent("pk_bank_generic_parts")),
    "archive": (lambda c: c.L.pk_archive_create(c.h, 1, SLOTS - 1, 7), absent("pk_archive_cells")),
    "exchange": (lambda c: c.L.pk_archive_exchange_enable(c.h), absent("pk_archive_payload_bytes")),
    "counts": (lambda c: c.L.pk_counts_create(c.h, 10), absent("pk_counts_limit")),
    "fstack": (lambda c: c.L.pk_fstack_create(c.h, 4, 2, 0, 0), absent("pk_fstack_depth")),
    "probes": (probes, absent("pk_probe_count")),
    "first_steps": (step, None),
    "grow": (lambda c: c.L.pk_set_episode_params(c.h, GROW_TO, 4.0), grow_probe),
    "steps": (steps, None),
    "destroy": (destroy, None),
}
SCRIPTS = {
    "reward": (True, ["create", "bank", "traj", "episodes", "archive", "exchange", "counts", "fstack", "first_steps", "grow",
                      "steps", "destroy"]),
    "reward_episodes_first": (True, ["create", "bank", "episodes", "traj", "archive", "exchange", "counts", "fstack",
                                     "first_steps", "grow", "steps", "destroy"]),
    "generic": (False, ["create", "probes", "fstack", "bank", "traj", "generic", "archive", "counts", "first_steps", "grow",
                        "steps", "destroy"]),
}


def run(c, names):
    for name in names:
        rc = CALLS[name][0](c)
        assert rc == 0, (name, rc, c.L.pk_last_error())


def clean_allocs(script):
    """hipMalloc calls of every call of a script on a clean run."""
    reward, names = SCRIPTS[script]
    c, out = Ctx(reward), []
    for name in names:
        before = c.L.pk_sim_alloc_calls()
        run(c, [name])
        out.append(c.L.pk_sim_alloc_calls() - before)
    return out


_allocs = {}


@pytest.mark.parametrize("script,index", [(s, i) for s, (_, names) in SCRIPTS.items() for i in range(len(names))],
                         ids=lambda v: str(v))
def test_failed_allocation_leaves_nothing_behind(script, index):
    reward, names = SCRIPTS[script]
    if script not in _allocs:
        _allocs[script] = clean_allocs(script)
    name, count = names[index], _allocs[script][index]
    call, probe = CALLS[name]
    if name in ("create", "bank", "traj", "episodes", "generic", "archive", "exchange", "counts", "fstack", "probes", "grow"):
        assert count > 0, "the sweep must cover %s" % name
    for k in range(count):
        c = Ctx(reward)
        baseline = c.L.pk_sim_alloc_live()
        run(c, names[:index])
        live = c.L.pk_sim_alloc_live()
        check = probe(c)
        c.L.pk_sim_alloc_fail_at(k)
        rc = call(c)
        c.L.pk_sim_alloc_fail_at(-1)
        assert rc < 0 and c.L.pk_last_error(), (name, k, rc)
        assert c.L.pk_sim_alloc_live() == live, (name, k)
        check()
        run(c, names[index:])
        assert c.L.pk_sim_alloc_live() == baseline, (name, k)


@pytest.mark.parametrize("script", list(SCRIPTS))
def test_clean_script_frees_everything(script):
    reward, names = SCRIPTS[script]
    c = Ctx(reward)
    baseline = c.L.pk_sim_alloc_live()
    run(c, names)
    assert c.L.pk_sim_alloc_live() == baseline


# ---- launch sequence pin ----------------------------------------------------------------------------

def sequences():
    """{kind/entry point/env0: the recorded lines} of the reset and bank entry points, on a handle
    of each kind at 128 envs in two 64-env ranges."""
    out = {}
    for kind in ("reward", "generic"):
        reward, names = SCRIPTS[kind]
        c = Ctx(reward, 128)
        run(c, names[:names.index("first_steps") + 1])
        L, h = c.L, c.h
        mask = np.zeros(c.n, np.uint8)
        mask[[1, 5, 64, 100]] = 1
        slots = slots_of(c, {1: 0, 5: 1, 64: 2, 100: 3, 7: 0, 70: 1})
        m, s = mask.ctypes.data, slots.ctypes.data
        entries = [
            ("pk_bank_save", lambda e0: L.pk_bank_save(h, s, e0, 64, None)),
            ("pk_bank_checkpoint", lambda e0: L.pk_bank_checkpoint(h, s, e0, 64, None)),
            ("pk_reset_range", lambda e0: L.pk_reset_range(h, e0, 64, m, None)),
            ("pk_reset_range/all", lambda e0: L.pk_reset_range(h, e0, 64, None, None)),
            ("pk_reset_from/slots", lambda e0: L.pk_reset_from(h, e0, 64, m, s, None)),
            ("pk_reset_from/no_slots", lambda e0: L.pk_reset_from(h, e0, 64, m, None, None)),
            ("pk_bank_load", lambda e0: L.pk_bank_load(h, s, e0, 64, None)),
            ("pk_bank_resume", lambda e0: L.pk_bank_resume(h, s, e0, 64, None)),
        ]
        buf = ctypes.create_string_buffer(1 << 16)
        for name, call in entries:
            for e0 in (0, 64):
                L.pk_sim_record_enable(1)
                rc = call(e0)
                assert L.pk_sim_record_get(buf, len(buf)) < len(buf)
                L.pk_sim_record_enable(0)
                assert rc == 0, (kind, name, e0, L.pk_last_error())
                out["%s/%s/%d" % (kind, name, e0)] = buf.value.decode().splitlines()
        destroy(c)
    return out


def test_launch_sequences_are_pinned():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = sequences()
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key


if __name__ == "__main__":
    if sys.argv[1:] == ["--record"]:
        with open(GOLDEN, "w") as f:
            json.dump(sequences(), f, indent=0, sort_keys=True)
            f.write("\n")
        print("wrote", GOLDEN)
