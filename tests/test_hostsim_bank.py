"""The savestate bank (pk_bank_* / pk_reset_from, ABI v7) on the CPU: the unmodified kernels and C
ABI in the host-simulation build (tests/hostsim), driven through BatchedEmulator's bank methods.
The oracle throughout is existing code: pk_load_env, pk_snapshot, a handle created with state=,
and the 6 reference v9 states of tests/golden/states.npz.  The gfx950 build runs the same checks
in test_gpu_bank.py (-m gpu)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hostsim"))

from emulator import HostsimEmulator  # noqa: E402
from pokegym_amd.testrom.fuzz import fuzz_rom  # noqa: E402
from pokegym_amd.testrom.game import game_rom  # noqa: E402

N = 70   # two 64-env groups, the second partial


@pytest.fixture(scope="module")
def pool():
    z = np.load(os.path.join(HERE, "golden", "states.npz"))
    return [s.tobytes() for s in z["states"]]


@pytest.fixture(scope="module")
def pkbench_pool():
    """pkbench states after 0, 5 and 11 steps from its power-on state."""
    rom = game_rom()
    emu = HostsimEmulator(rom, 1)
    acts = np.random.default_rng(3).integers(0, 8, 11, dtype=np.uint8)
    out = [emu.snapshot(0)]
    for t in range(11):
        emu.step(torch.tensor([acts[t]], dtype=torch.uint8))
        if t + 1 in (5, 11):
            out.append(emu.snapshot(0))
    emu.close()
    return rom, out


def slots_tensor(values):
    return torch.tensor(np.asarray(values, np.int32))


def rows(a):
    return [bytes(r) for r in a]


def test_bank_put_get_round_trip(pool):
    emu = HostsimEmulator(fuzz_rom(2), 4)
    emu.bank_create(9)
    assert emu.bank_slots == 9
    for i, st in enumerate(pool):
        emu.bank_put(i, st)
    for i, st in enumerate(pool):
        assert emu.bank_get(i) == st, i
    out = np.zeros(142610, np.uint8)
    p = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    assert emu._L.pk_bank_get(emu._h, 7, p, out.size) < 0      # empty slot
    assert emu._L.pk_bank_get(emu._h, 9, p, out.size) < 0      # no such slot
    assert emu._L.pk_bank_put(emu._h, 0, p, 100) < 0           # not a v9 state
    emu.close()


@pytest.mark.parametrize("ilv", ["64", "32", "16", "1"])
def test_bank_load_equals_load_env(pool, ilv, monkeypatch):
    monkeypatch.setenv("PK_ILV", ilv)
    rom = fuzz_rom(2)
    a, b = HostsimEmulator(rom, N), HostsimEmulator(rom, N)
    b.bank_create(9)
    for i, st in enumerate(pool):
        b.bank_put(i, st)
    slot = np.arange(N, dtype=np.int32) % 6       # every slot named by 11 or 12 envs
    skipped, rejected = (3, 63, 64, 69), (10, 40)
    slot[list(skipped)] = -1
    slot[10] = 9                                  # out of range
    slot[40] = 7                                  # empty
    pre = b.snapshot_range(0, N)
    for i in range(N):
        if i not in skipped + rejected:
            a.load_env(i, pool[i % 6])
    b.bank_load(slots_tensor(slot))
    sa, sb = a.snapshot_range(0, N), b.snapshot_range(0, N)
    bad = [i for i in range(N) if bytes(sa[i]) != bytes(sb[i])]
    assert not bad, bad
    for i in skipped + rejected:
        assert bytes(sb[i]) == bytes(pre[i]), i
    assert torch.equal(a.screen, b.screen)
    assert b.bank_rejects() == 2
    assert b.bank_rejects() == 0
    acts = torch.from_numpy(np.random.default_rng(5).integers(0, 8, (4, N), dtype=np.uint8))
    for t in range(4):
        a.step(acts[t])
        b.step(acts[t])
    sa, sb = a.snapshot_range(0, N), b.snapshot_range(0, N)
    bad = [i for i in range(N) if bytes(sa[i]) != bytes(sb[i])]
    assert not bad, bad
    assert torch.equal(a.screen, b.screen)
    a.close()
    b.close()


def test_bank_load_range_form(pool):
    emu = HostsimEmulator(fuzz_rom(2), N)
    emu.bank_create(2)
    emu.bank_put(0, pool[1])
    slot = slots_tensor(np.zeros(N, np.int32))     # envs below 64 name a slot too
    pre = emu.snapshot_range(0, N)
    emu.bank_load(slot, 64, 6)
    post = emu.snapshot_range(0, N)
    assert rows(post[:64]) == rows(pre[:64])
    assert all(bytes(r) == pool[1] for r in post[64:])
    assert emu._L.pk_bank_load(emu._h, slot.data_ptr(), 32, 6, None) < 0      # env0 not a multiple of 64
    assert emu._L.pk_bank_load(emu._h, slot.data_ptr(), 64, 7, None) < 0      # end past n
    assert emu._L.pk_bank_save(emu._h, slot.data_ptr(), 32, 6, None) < 0
    assert emu._L.pk_reset_from(emu._h, 32, 6, None, slot.data_ptr(), None) < 0
    assert rows(emu.snapshot_range(0, N)) == rows(post)
    emu.close()


@pytest.mark.parametrize("ilv", ["64", "32", "16", "1"])
def test_bank_save_then_load(ilv, monkeypatch):
    monkeypatch.setenv("PK_ILV", ilv)
    rom = game_rom()
    emu = HostsimEmulator(rom, N, max_episode_steps=7)
    twin = HostsimEmulator(rom, N, max_episode_steps=7)
    emu.bank_create(8)
    acts = torch.from_numpy(np.random.default_rng(9).integers(0, 8, (9, N), dtype=np.uint8))
    for t in range(3):
        emu.step(acts[t])
    src = (0, 31, 32, 63, 64, 69)
    slot = np.full(N, -1, np.int32)
    slot[list(src)] = np.arange(6)
    snap = {e: emu.snapshot(e) for e in src}
    emu.bank_save(slots_tensor(slot))
    for k, e in enumerate(src):
        assert emu.bank_get(k) == snap[e], e
    unsaved = np.zeros(142610, np.uint8)
    assert emu._L.pk_bank_get(emu._h, 6, unsaved.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), unsaved.size) < 0
    for t in range(3, 6):
        emu.step(acts[t])
    # into other envs, across sub-blocks and groups; slot 0 twice
    dst = {5: 0, 33: 1, 62: 2, 65: 3, 1: 4, 40: 5, 68: 0}
    slot = np.full(N, -1, np.int32)
    for e, k in dst.items():
        slot[e] = k
    others = [e for e in range(N) if e not in dst]
    pre = emu.snapshot_range(0, N)
    emu.bank_load(slots_tensor(slot))
    post = emu.snapshot_range(0, N)
    for e, k in dst.items():
        assert bytes(post[e]) == snap[src[k]], e
        twin.load_env(e, snap[src[k]])
    assert rows(post[others]) == rows(pre[others])
    assert emu.bank_rejects() == 0
    for t in range(6, 9):
        emu.step(acts[t])
        twin.step(acts[t])
        if t == 6:   # a load leaves PK_R_TIME alone: the 7th step ends every env's episode
            assert bool(emu.terminals.all())
    se, st = emu.snapshot_range(0, N), twin.snapshot_range(0, N)
    for e in dst:
        assert bytes(se[e]) == bytes(st[e]), e
        assert torch.equal(emu.screen[e], twin.screen[e]), e
    emu.close()
    twin.close()


def test_reset_from_without_reward(pool):
    rom = fuzz_rom(2)
    emu = HostsimEmulator(rom, N)
    emu.bank_create(6)
    for i, st in enumerate(pool):
        emu.bank_put(i, st)
    acts = torch.from_numpy(np.random.default_rng(2).integers(0, 8, (2, N), dtype=np.uint8))
    for t in range(2):
        emu.step(acts[t])
    mask = np.zeros(N, np.uint8)
    masked = (0, 1, 2, 30, 33, 63, 64, 66, 69)
    mask[list(masked)] = 1
    slot = (np.arange(N, dtype=np.int32) * 5) % 6
    slot[[2, 66]] = -1                               # the handle's own template
    pre = emu.snapshot_range(0, N)
    emu.reset_from(slots_tensor(slot), torch.from_numpy(mask))
    post = emu.snapshot_range(0, N)
    want = {}
    for s in sorted(set(int(slot[e]) for e in masked)):
        t = HostsimEmulator(rom, 1, state=pool[s] if s >= 0 else None)
        t.reset()
        want[s] = (t.snapshot(0), t.screen[0].clone())
        t.close()
    for e in range(N):
        if e in masked:
            snap, screen = want[int(slot[e])]
            assert bytes(post[e]) == snap, e
            assert torch.equal(emu.screen[e], screen), e
        else:
            assert bytes(post[e]) == bytes(pre[e]), e
    # a reset zeroes the step counter whichever source it reloads: with max_episode_steps = 20480
    # no env is done after one more step, and slot_of_env NULL is pk_reset_range
    assert emu._L.pk_reset_from(emu._h, 0, N, None, None, None) == 0
    assert rows(emu.snapshot_range(0, N)) == [want[-1][0]] * N
    assert emu.bank_rejects() == 0
    emu.close()


def test_reset_from_counts_rejects_and_falls_back(pool):
    rom = fuzz_rom(2)
    emu = HostsimEmulator(rom, N)
    emu.bank_create(4)
    emu.bank_put(1, pool[3])
    emu.step(torch.full((N,), 4, dtype=torch.uint8))
    slot = np.full(N, 1, np.int32)
    slot[7], slot[65] = 4, 2                         # out of range, empty
    emu.reset_from(slots_tensor(slot))
    t = HostsimEmulator(rom, 1)
    t.reset()
    tmpl = t.snapshot(0)
    t.close()
    post = emu.snapshot_range(0, N)
    for e in range(N):
        assert bytes(post[e]) == (tmpl if e in (7, 65) else pool[3]), e
    assert emu.bank_rejects() == 2
    emu.close()


@pytest.mark.parametrize("reload_on_reset", [True, False])
def test_reset_from_with_reward(pkbench_pool, reload_on_reset):
    rom, states = pkbench_pool
    n = 6
    kw = dict(reward=True, reload_on_reset=reload_on_reset, max_episode_steps=3)
    emu = HostsimEmulator(rom, n, state=states[0], **kw)
    emu.bank_create(3)
    for i, st in enumerate(states):
        emu.bank_put(i, st)
    twins = [HostsimEmulator(rom, n, state=st, **kw) for st in states]
    slot = np.array([2, 1, 0, 1, 2, -1], np.int32)
    src = [int(s) if s >= 0 else 0 for s in slot]    # -1: the handle's template, states[0]
    acts = torch.from_numpy(np.random.default_rng(4).integers(0, 8, (3, n), dtype=np.uint8))

    def same(what):
        for e in range(n):
            t = twins[src[e]]
            assert torch.equal(emu.obs[e], t.obs[e]), (what, e)
            assert emu.rewards[e] == t.rewards[e] and emu.terminals[e] == t.terminals[e], (what, e)
            assert emu.snapshot(e) == t.snapshot(e), (what, e)

    emu.reset_from(slots_tensor(slot))
    for t in twins:
        t.reset()
    same("reset")
    for k in range(3):
        emu.step(acts[k])
        for t in twins:
            t.step(acts[k])
        same(k)
    assert bool(emu.terminals.all())
    # the second reset: a reload with PK_F_RELOAD_ON_RESET, none without it (first reset only)
    emu.reset_from(slots_tensor(slot))
    for t in twins:
        t.reset()
    same("second reset")
    if reload_on_reset:
        assert [emu.snapshot(e) for e in range(n)] == [states[s] for s in src]
    else:
        assert all(emu.snapshot(e) != states[src[e]] for e in range(n))
    emu.step(acts[0])
    for t in twins:
        t.step(acts[0])
    same("step after the second reset")
    assert emu.bank_rejects() == 0
    emu.close()
    for t in twins:
        t.close()


def test_bank_guards(pool):
    emu = HostsimEmulator(fuzz_rom(2), N)
    L, h = emu._L, emu._h
    slot = slots_tensor(np.zeros(N, np.int32))
    buf = np.frombuffer(pool[0], np.uint8).copy()
    p = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    v = ctypes.c_uint64()
    assert L.pk_bank_slots(h) == 0
    assert L.pk_bank_put(h, 0, p, buf.size) < 0
    assert L.pk_bank_get(h, 0, p, buf.size) < 0
    assert L.pk_bank_save(h, slot.data_ptr(), 0, N, None) < 0
    assert L.pk_bank_load(h, slot.data_ptr(), 0, N, None) < 0
    assert L.pk_reset_from(h, 0, N, None, slot.data_ptr(), None) < 0
    assert L.pk_bank_rejects(h, ctypes.byref(v)) < 0
    assert L.pk_last_error()
    assert L.pk_bank_create(h, 0) < 0
    assert L.pk_bank_create(h, 65537) < 0
    assert L.pk_bank_slots(h) == 0
    assert L.pk_bank_create(h, 3) == 0
    assert L.pk_bank_create(h, 3) < 0
    assert L.pk_bank_slots(h) == 3
    assert L.pk_bank_load(h, None, 0, N, None) < 0
    pre = emu.snapshot(5)
    emu.step(torch.full((N,), 2, dtype=torch.uint8))
    assert emu.snapshot(5) != pre
    emu.close()


class _NoStream:
    """CPU stand-in for the HIP streams/events of VecEnv's sub-batch pipeline."""
    def __init__(self, *a, **k):
        pass

    def wait_stream(self, other):
        pass

    def wait_event(self, ev):
        pass

    def record(self, stream=None):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def test_vecenv_state_pool_sub_batches(pool, monkeypatch):
    """VecEnv(48, batch_size=24, state_pool=...) over the host-simulation emulator: resets and
    auto-resets start every env from its drawn slot, padding envs are never written, and
    save_to_bank / load_from_bank address envs by env index."""
    from pokegym_amd.env import VecEnv
    for name in ("Stream", "Event", "current_stream", "stream"):
        monkeypatch.setattr(torch.cuda, name, _NoStream)
    rom = fuzz_rom(2)
    emu = HostsimEmulator(rom, 128, reload_on_reset=True, max_episode_steps=2)
    pad = emu.snapshot(30)
    env = VecEnv(48, emulator=emu, batch_size=24, log_interval=0, state_pool=pool, pool_seed=7, bank_slots=4)
    assert emu.bank_slots == 10 and env.pool_size == 6
    env.reset()
    first = env.start_slots
    assert first.shape == (48,) and int(first.min()) >= 0 and int(first.max()) < 6
    assert len(set(first.tolist())) > 1
    for e in range(48):
        assert env.save_state(e) == pool[int(first[e])], e
    for p in (24, 63, 64 + 24, 127):
        assert emu.snapshot(p) == pad, p
    acts = torch.zeros(48, dtype=torch.uint8)
    env.step(acts)
    assert torch.equal(env.start_slots, first)            # nobody finished: nobody drew
    assert env.save_state(0) != pool[int(first[0])]
    *_, term, _, _ = env.step(acts)                        # max_episode_steps = 2: all auto-reset
    assert bool(term.all())
    second = env.start_slots
    assert not torch.equal(second, first)
    for e in range(48):
        assert env.save_state(e) == pool[int(second[e])], e
    # swarm: copy envs of the first sub-batch over envs of the second through the free slots
    env.step(acts)
    srcs, dsts, free = [0, 5, 23], [24, 30, 47], [6, 7, 9]
    want = [env.save_state(e) for e in srcs]
    env.save_to_bank(srcs, free)
    env.load_from_bank(torch.tensor(dsts), torch.tensor(free))
    assert [env.save_state(e) for e in dsts] == want
    for p in (24, 63, 64 + 24, 127):
        assert emu.snapshot(p) == pad, p
    with pytest.raises(ValueError):
        env.save_to_bank([0, 1], [6, 6])
    assert emu.bank_rejects() == 0
    emu.close()


def test_vecenv_without_pool_makes_no_bank():
    from pokegym_amd.env import VecEnv
    emu = HostsimEmulator(fuzz_rom(2), 4)
    env = VecEnv(4, emulator=emu, log_interval=0)
    env.reset()
    env.step(torch.zeros(4, dtype=torch.uint8))
    assert emu.bank_slots == 0
    with pytest.raises(RuntimeError):
        env.start_slots
    with pytest.raises(RuntimeError):
        env.save_to_bank([0], [0])
    env.close()
