"""The savestate bank (pk_bank_* / pk_reset_from, ABI v7) on the MI355X, through BatchedEmulator
and VecEnv.  The oracle is existing code: load_env, snapshot, an emulator created with state=,
and the 6 reference v9 states of tests/golden/states.npz; the same checks run on the CPU in
test_hostsim_bank.py.  The tests only copy state and step known-good ROMs."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
N = 70   # two 64-env groups, the second partial


@pytest.fixture(scope="module")
def pool():
    z = np.load(os.path.join(HERE, "golden", "states.npz"))
    return [s.tobytes() for s in z["states"]]


@pytest.fixture(scope="module")
def pkbench_pool():
    """pkbench states after 0, 5 and 11 steps from its power-on state."""
    import torch
    from pokegym_amd.emulator import BatchedEmulator
    from pokegym_amd.testrom.game import game_rom
    rom = game_rom()
    emu = BatchedEmulator(rom, 1)
    acts = np.random.default_rng(3).integers(0, 8, 11, dtype=np.uint8)
    out = [emu.snapshot(0)]
    for t in range(11):
        emu.step(torch.tensor([acts[t]], dtype=torch.uint8, device=emu.device))
        if t + 1 in (5, 11):
            out.append(emu.snapshot(0))
    emu.close()
    return rom, out


def dev(values, dtype=np.int32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(values, dtype)).cuda()


def rows(a):
    return [bytes(r) for r in a]


@pytest.mark.parametrize("ilv", ["32", "16"])
def test_bank_load_equals_load_env(pool, ilv, monkeypatch):
    import torch
    from pokegym_amd.emulator import BatchedEmulator
    from pokegym_amd.testrom.fuzz import fuzz_rom
    monkeypatch.setenv("PK_ILV", ilv)
    rom = fuzz_rom(2)
    a, b = BatchedEmulator(rom, N), BatchedEmulator(rom, N)
    b.bank_create(9)
    for i, st in enumerate(pool):
        b.bank_put(i, st)
        assert b.bank_get(i) == st
    slot = np.arange(N, dtype=np.int32) % 6
    skipped, rejected = (3, 63, 64, 69), (10, 40)
    slot[list(skipped)] = -1
    slot[10] = 9                                  # out of range
    slot[40] = 7                                  # empty
    pre = b.snapshot_range(0, N)
    for i in range(N):
        if i not in skipped + rejected:
            a.load_env(i, pool[i % 6])
    b.bank_load(dev(slot))
    sa, sb = a.snapshot_range(0, N), b.snapshot_range(0, N)
    bad = [i for i in range(N) if bytes(sa[i]) != bytes(sb[i])]
    assert not bad, bad
    for i in skipped + rejected:
        assert bytes(sb[i]) == bytes(pre[i]), i
    assert torch.equal(a.screen, b.screen)
    assert b.bank_rejects() == 2
    assert b.bank_rejects() == 0
    acts = dev(np.random.default_rng(5).integers(0, 8, (4, N)), np.uint8)
    for t in range(4):
        a.step(acts[t])
        b.step(acts[t])
    sa, sb = a.snapshot_range(0, N), b.snapshot_range(0, N)
    bad = [i for i in range(N) if bytes(sa[i]) != bytes(sb[i])]
    assert not bad, bad
    assert torch.equal(a.screen, b.screen)
    a.close()
    b.close()


@pytest.mark.parametrize("ilv", ["32", "16"])
def test_bank_save_then_load(ilv, monkeypatch):
    import torch
    from pokegym_amd.emulator import BatchedEmulator
    from pokegym_amd.testrom.game import game_rom
    monkeypatch.setenv("PK_ILV", ilv)
    rom = game_rom()
    emu = BatchedEmulator(rom, N, max_episode_steps=7)
    twin = BatchedEmulator(rom, N, max_episode_steps=7)
    emu.bank_create(8)
    acts = dev(np.random.default_rng(9).integers(0, 8, (9, N)), np.uint8)
    for t in range(3):
        emu.step(acts[t])
    src = (0, 31, 32, 63, 64, 69)
    slot = np.full(N, -1, np.int32)
    slot[list(src)] = np.arange(6)
    snap = {e: emu.snapshot(e) for e in src}
    emu.bank_save(dev(slot))
    for k, e in enumerate(src):
        assert emu.bank_get(k) == snap[e], e
    for t in range(3, 6):
        emu.step(acts[t])
    dst = {5: 0, 33: 1, 62: 2, 65: 3, 1: 4, 40: 5, 68: 0}
    slot = np.full(N, -1, np.int32)
    for e, k in dst.items():
        slot[e] = k
    others = [e for e in range(N) if e not in dst]
    pre = emu.snapshot_range(0, N)
    emu.bank_load(dev(slot))
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


@pytest.mark.parametrize("ilv", ["32", "16"])
@pytest.mark.parametrize("reload_on_reset", [True, False])
def test_reset_from_with_reward(pkbench_pool, reload_on_reset, ilv, monkeypatch):
    import torch
    from pokegym_amd.emulator import BatchedEmulator
    monkeypatch.setenv("PK_ILV", ilv)
    rom, states = pkbench_pool
    kw = dict(reward=True, reload_on_reset=reload_on_reset, max_episode_steps=3)
    emu = BatchedEmulator(rom, N, state=states[0], **kw)
    emu.bank_create(3)
    for i, st in enumerate(states):
        emu.bank_put(i, st)
    twins = [BatchedEmulator(rom, N, state=st, **kw) for st in states]
    slot = (np.arange(N, dtype=np.int32) * 2) % 3
    slot[[4, 64]] = -1                               # the emulator's template, states[0]
    src = np.where(slot >= 0, slot, 0)
    sel = [torch.from_numpy(src == s).cuda() for s in range(3)]
    acts = dev(np.random.default_rng(4).integers(0, 8, (3, N)), np.uint8)

    def same(what):
        snap = emu.snapshot_range(0, N)
        for s, t in enumerate(twins):
            m = sel[s]
            assert torch.equal(emu.obs[m], t.obs[m]), (what, s)
            assert torch.equal(emu.rewards[m], t.rewards[m]), (what, s)
            assert torch.equal(emu.terminals[m], t.terminals[m]), (what, s)
            ts = t.snapshot_range(0, N)
            assert all(bytes(snap[e]) == bytes(ts[e]) for e in np.flatnonzero(src == s)), (what, s)
        return snap

    emu.reset_from(dev(slot))
    for t in twins:
        t.reset()
    same("reset")
    for k in range(3):
        emu.step(acts[k])
        for t in twins:
            t.step(acts[k])
        same(k)
    assert bool(emu.terminals.all())
    emu.reset_from(dev(slot))
    for t in twins:
        t.reset()
    snap = same("second reset")
    reloaded = [bytes(snap[e]) == states[src[e]] for e in range(N)]
    assert all(reloaded) if reload_on_reset else not any(reloaded)
    assert emu.bank_rejects() == 0
    emu.close()
    for t in twins:
        t.close()


def test_vecenv_state_pool_sub_batches(pool):
    """VecEnv(48, batch_size=24) in padded 64-env slots, its sub-batches on their own streams: every
    reset and auto-reset starts each env from its drawn slot, padding envs are never written, and
    save_to_bank / load_from_bank move states between the sub-batches mid-pipeline."""
    import torch
    from pokegym_amd.env import VecEnv
    from pokegym_amd.testrom.fuzz import fuzz_rom
    env = VecEnv(48, rom=fuzz_rom(2), power_on=True, batch_size=24, reward=False, reload_on_reset=True,
                 max_episode_steps=2, log_interval=0, state_pool=pool, pool_seed=7, bank_slots=4)
    emu = env.emu
    assert emu.n == 128 and emu.bank_slots == 10
    pads = (24, 63, 64 + 24, 127)
    pad = emu.snapshot(30)
    env.async_reset()
    first = env.start_slots.cpu()
    assert len(set(first.tolist())) > 1 and int(first.min()) >= 0 and int(first.max()) < 6
    for e in range(48):
        assert env.save_state(e) == pool[int(first[e])], e
    acts = torch.zeros(24, dtype=torch.uint8, device=env.device)
    for _ in range(4):               # two steps of each sub-batch: every env finishes and restarts
        env.recv()
        env.send(acts)
    torch.cuda.synchronize()
    second = env.start_slots.cpu()
    assert not torch.equal(second, first)
    for e in range(48):
        assert env.save_state(e) == pool[int(second[e])], e
    # mid-pipeline: both sub-batches have a step in flight when the states are copied across
    for _ in range(2):
        env.recv()
        env.send(acts)
    srcs, dsts, free = [0, 5, 23, 24], [30, 47, 25, 1], [6, 7, 9, 8]
    env.save_to_bank(srcs, free, check=False)
    env.load_from_bank(torch.tensor(dsts, device=env.device), torch.tensor(free, device=env.device))
    torch.cuda.synchronize()
    assert [env.save_state(e) for e in dsts] == [env.save_state(e) for e in srcs]
    assert [emu.bank_get(k) for k in free] == [env.save_state(e) for e in srcs]
    assert env.save_state(0) != pool[int(second[0])]
    for p in pads:
        assert emu.snapshot(p) == pad, p
    with pytest.raises(ValueError):
        env.save_to_bank([0, 1], [6, 6])
    assert emu.bank_rejects() == 0
    env.close()
