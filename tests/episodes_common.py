"""Shared scenarios of the episode-checkpoint tests (pk_bank_checkpoint / pk_bank_resume, ABI v8):
test_hostsim_episodes.py runs them on the host-simulation build, test_gpu_episodes.py on the
gfx950 build.  The oracle needs no reference: emulator and reward stack are deterministic, so an
env resumed from a checkpoint and fed the same actions must return, bit for bit, what the env it
was saved from returned."""
import numpy as np
import torch

from pokegym_amd.info import FIELDS

N = 70            # two 64-env groups, the second partial
MAX_STEPS = 12    # cap_log2 = 10: a 4 KB seen table
T1, T2 = 5, 10    # steps before the checkpoint, steps recorded after it (across the episode end)
S = (0, 31, 32, 63, 64, 69)                  # checkpointed envs -> slots 0..5
# destination -> slot: other sub-blocks, the other group both ways, slot 0 twice, and env 66, which
# is never reset (seen tag 0, reset count 0)
D = {5: 0, 33: 1, 62: 2, 65: 3, 1: 4, 40: 5, 68: 0, 66: 2}
NEVER_RESET = 66
COORD = FIELDS.index("coord")                # np.sum(counts_map): the env's own, NaN without the heat map
EXPLORATION = FIELDS.index("reward.exploration")


def slot_map(mapping, n=N):
    slot = np.full(n, -1, np.int32)
    for e, k in mapping.items():
        slot[e] = k
    return slot


def outputs(emu, envs):
    """Everything a step returns for `envs`, as host arrays."""
    idx = torch.as_tensor(list(envs), device=emu.device)
    flag = emu.info_flag[idx].cpu().numpy()
    info = emu.info[:, idx].cpu().numpy().copy()
    info[COORD] = 0.0
    info[:, flag == 0] = 0.0                 # a record is only defined where the flag is set
    bits = emu.info_bits[:, idx].cpu().numpy().copy()
    bits[:, flag == 0] = 0
    snap = emu.snapshot_range(0, emu.n)
    return {"rew": emu.rewards[idx].cpu().numpy().copy(), "term": emu.terminals[idx].cpu().numpy().copy(),
            "trunc": emu.truncations[idx].cpu().numpy().copy(), "obs": emu.obs[idx].cpu().numpy().copy(),
            "errors": emu.errors[idx].cpu().numpy().copy(), "flag": flag, "info": info, "bits": bits,
            "snap": snap[list(envs)].copy()}


def same(a, b, what, cols_a=None, cols_b=None):
    """Bit-for-bit equality of two outputs() records (optionally of chosen columns)."""
    for k in a:
        x, y = a[k], b[k]
        if k in ("info", "bits"):
            x = x if cols_a is None else x[:, cols_a]
            y = y if cols_b is None else y[:, cols_b]
        else:
            x = x if cols_a is None else x[cols_a]
            y = y if cols_b is None else y[cols_b]
        assert x.shape == y.shape, (what, k)
        assert x.tobytes() == y.tobytes(), (what, k)


def masked(envs, dev, n=N):
    m = np.zeros(n, np.uint8)
    m[list(envs)] = 1
    return dev(m, np.uint8)


class Script:
    """Per-step, per-env inputs: a random action and, as the benchmark ROM keeps its player
    elsewhere, the coordinates the reward stack reads (D361 y, D362 x, D35E map), written with
    set_ram before the step — a random walk over an 6 x 6 patch of maps 0 and 1, so that seen sets
    grow, revisit, and the visited mask is rebuilt at map changes."""

    def __init__(self, steps, n, seed, dev):
        rng = np.random.default_rng(seed)
        self.acts = dev(rng.integers(0, 8, (steps, n)), np.uint8)
        self.pos = dev(rng.integers(0, 6, (steps, n, 2)), np.uint8)
        self.map = dev(np.cumsum(rng.random((steps, n, 1)) < 0.2, axis=0) % 2, np.uint8)

    def copy_rows(self, t, dst, other, t_other, src):
        """Step t of envs dst takes the inputs `other` has at step t_other for envs src."""
        for mine, theirs in ((self.acts, other.acts), (self.pos, other.pos), (self.map, other.map)):
            mine[t, dst] = theirs[t_other, src]

    def step(self, emu, t):
        emu.set_ram(0xD361, self.pos[t])
        emu.set_ram(0xD35E, self.map[t])
        emu.step(self.acts[t])


def prologue(emu, sc, dev):
    """T1 steps with per-env random actions; some envs get one or two extra masked resets (their
    seen tags and step counters then differ from the others'), env NEVER_RESET none at all."""
    emu.reset(masked(set(range(N)) - {NEVER_RESET}, dev))
    sc.step(emu, 0)
    sc.step(emu, 1)
    emu.reset(masked((1, 5, 33, 40), dev))
    sc.step(emu, 2)
    emu.reset(masked((33, 65, 68), dev))
    sc.step(emu, 3)
    sc.step(emu, 4)


def step_and_autoreset(emu, sc, t, skip_reset=()):
    """One step, the outputs of every env, then the reset of the finished envs (as VecEnv does)."""
    sc.step(emu, t)
    out = outputs(emu, range(N))
    term = emu.terminals.clone()
    for e in skip_reset:
        term[e] = 0
    emu.reset(term)
    return out


def twin_continuation(make, dev, mover="resume", seed=11):
    """The main scenario.  Returns (rec, rep): rec[t] the outputs of every env of the original run
    at step T1 + t, rep[t] those of the replay after the resume (mover="resume") or a plain
    bank_load (mover="load", the control); rec0 / rep0 the state straight after checkpoint / resume.
    With mover="resume" the non-participants are checked against a twin handle in here."""
    sc = Script(T1 + 2 * T2, N, seed, dev)
    emu = make(N, reward=True, max_episode_steps=MAX_STEPS)
    twin = make(N, reward=True, max_episode_steps=MAX_STEPS) if mover == "resume" else None
    emu.bank_create(8)
    emu.bank_enable_episodes()
    assert emu.bank_has_episodes
    prologue(emu, sc, dev)
    if twin is not None:
        prologue(twin, sc, dev)
        same(outputs(emu, range(N)), outputs(twin, range(N)), "prologue")
    pre = outputs(emu, range(N))
    emu.bank_checkpoint(dev(slot_map({e: k for k, e in enumerate(S)})))
    rec0 = outputs(emu, range(N))
    same(pre, rec0, "a checkpoint leaves every env as it is")
    for k, e in enumerate(S):                # the machine part is what a plain save stores
        assert emu.bank_get(k) == bytes(rec0["snap"][e]), e
    # env NEVER_RESET reloads its template at its first reset: it is compared up to the episode's
    # end only, and not reset here
    rec = []
    for t in range(T2):
        rec.append(step_and_autoreset(emu, sc, T1 + t, skip_reset=(NEVER_RESET,)))
        if twin is not None:
            same(rec[-1], step_and_autoreset(twin, sc, T1 + t, skip_reset=(NEVER_RESET,)), ("sources unchanged", t))
    assert any(r["term"][list(S)].any() for r in rec[:-1]), "the recorded steps must cross the episode end"
    # resume into envs with other histories
    dst = list(D)
    src = [S[D[e]] for e in dst]
    before = outputs(emu, range(N))
    if mover == "resume":
        emu.bank_resume(dev(slot_map(D)))
    else:
        emu.bank_load(dev(slot_map(D)))
    rep0 = outputs(emu, range(N))
    others = [e for e in range(N) if e not in D]
    same(before, rep0, "envs taking no part", others, others)
    assert emu.bank_rejects() == 0
    rep = []
    for t in range(T2):
        sc.copy_rows(T1 + T2 + t, dst, sc, T1 + t, src)
        rep.append(step_and_autoreset(emu, sc, T1 + T2 + t, skip_reset=(NEVER_RESET,)))
        if twin is not None:
            same(rep[-1], step_and_autoreset(twin, sc, T1 + T2 + t, skip_reset=(NEVER_RESET,)), ("non-participants", t), others, others)
    emu.close()
    if twin is not None:
        twin.close()
    return rec0, rec, rep0, rep


def check_twin_continuation(make, dev):
    rec0, rec, rep0, rep = twin_continuation(make, dev, "resume")
    dst = list(D)
    src = [S[D[e]] for e in dst]
    for k in ("obs", "snap", "errors"):      # straight after the resume, before any step
        assert rep0[k][dst].tobytes() == rec0[k][src].tobytes(), k
    ended = False
    for t in range(T2):
        same(rep[t], rec[t], ("replay", t), dst[:-1], src[:-1])
        if not ended:                        # env NEVER_RESET: up to the end of the episode
            same(rep[t], rec[t], ("replay of the env that was never reset", t), dst[-1:], src[-1:])
            ended = bool(rec[t]["term"][src[-1]])
    assert ended
    # the tag hazard, on the seen count itself: every destination had live entries of its own tag
    # (it moved for 15 steps); at the episode's end its exploration term is the source's
    for d, s in zip(dst, src):
        t = next(t for t in range(T2) if rec[t]["term"][s])
        assert rep[t]["flag"][d] == 1 and rec[t]["flag"][s] == 1
        assert rep[t]["info"][EXPLORATION, d] == rec[t]["info"][EXPLORATION, s] > 0.0, (d, s)


def check_control(make, dev):
    """The same inputs with a plain bank_load: the machine jumps, the bookkeeping does not, so some
    reward or visited-mask byte of a destination must differ — else the main test proves nothing."""
    _, rec, _, rep = twin_continuation(make, dev, "load")
    dst = list(D)
    src = [S[D[e]] for e in dst]
    differs = any(rep[t]["rew"][dst].tobytes() != rec[t]["rew"][src].tobytes()
                  or rep[t]["obs"][dst][..., 3].tobytes() != rec[t]["obs"][src][..., 3].tobytes() for t in range(T2))
    assert differs


def check_rejects(make, dev):
    """Rejected envs stay untouched in every part and are counted; checkpointed slots export the
    env's snapshot; a plain save or put empties a slot's episode part; growth empties them all."""
    sc = Script(6, N, 2, dev)
    emu = make(N, reward=True, max_episode_steps=MAX_STEPS)
    twin = make(N, reward=True, max_episode_steps=MAX_STEPS)
    emu.bank_create(5)
    emu.bank_enable_episodes()
    for h in (emu, twin):
        h.reset()
        for t in range(3):
            sc.step(h, t)
    pool_state = emu.snapshot(7)
    emu.bank_save(dev(slot_map({2: 1})))              # slot 1: machine part only
    emu.bank_put(2, pool_state)                       # slot 2: machine part only
    emu.bank_checkpoint(dev(slot_map({9: 0, 64: 4})))
    assert emu.bank_get(0) == emu.snapshot(9) and emu.bank_get(4) == emu.snapshot(64)
    assert emu.bank_rejects() == 0
    emu.bank_checkpoint(dev(slot_map({12: 5})))       # slot >= K
    assert emu.bank_rejects() == 1
    before = outputs(emu, range(N))
    emu.bank_resume(dev(slot_map({3: 5, 10: 3, 40: 1, 65: 2, 69: 70000})))
    assert emu.bank_rejects() == 5
    same(before, outputs(emu, range(N)), "rejected envs untouched")
    # a checkpointed slot saved over, or put over, loses its episode part
    emu.bank_save(dev(slot_map({9: 0})))
    emu.bank_put(4, pool_state)
    emu.bank_resume(dev(slot_map({20: 0, 21: 4})))
    assert emu.bank_rejects() == 2
    same(before, outputs(emu, range(N)), "slots without an episode part")
    same(before, outputs(twin, range(N)), "twin")
    for t in range(3, 5):
        sc.step(emu, t)
        sc.step(twin, t)
        same(outputs(emu, range(N)), outputs(twin, range(N)), ("after the rejects", t))
    # argument guards
    L, h = emu._L, emu._h
    slot = dev(slot_map({0: 0}))
    for fn in (L.pk_bank_checkpoint, L.pk_bank_resume):
        assert fn(h, slot.data_ptr(), 32, 6, None) < 0      # env0 not a multiple of 64
        assert fn(h, slot.data_ptr(), 64, 7, None) < 0      # end past n
        assert fn(h, None, 0, N, None) < 0
    assert L.pk_bank_enable_episodes(h) < 0                 # once
    same(outputs(emu, range(N)), outputs(twin, range(N)), "after the refused calls")
    # growth of the seen set empties every episode part
    emu.bank_checkpoint(dev(slot_map({9: 0})))
    emu.set_episode_params(4000, 4.0)
    before = outputs(emu, range(N))
    emu.bank_resume(dev(slot_map({20: 0})))
    assert emu.bank_rejects() == 1
    same(before, outputs(emu, range(N)), "resume from a checkpoint older than the growth")
    emu.bank_checkpoint(dev(slot_map({9: 0})))             # the reallocated tables work
    emu.bank_resume(dev(slot_map({20: 0})))
    assert emu.bank_rejects() == 0
    assert emu.snapshot(20) == emu.snapshot(9)
    sc.copy_rows(5, [20], sc, 5, [9])
    sc.step(emu, 5)
    assert emu.rewards[20] == emu.rewards[9] and torch.equal(emu.obs[20], emu.obs[9])
    emu.close()
    twin.close()
    # handles that cannot carry episodes
    plain = make(N, reward=True, max_episode_steps=MAX_STEPS)
    L, h = plain._L, plain._h
    assert L.pk_bank_has_episodes(h) == 0
    assert L.pk_bank_enable_episodes(h) < 0                 # no bank
    plain.bank_create(2)
    assert L.pk_bank_checkpoint(h, slot.data_ptr(), 0, N, None) < 0
    assert L.pk_bank_resume(h, slot.data_ptr(), 0, N, None) < 0
    assert L.pk_bank_has_episodes(h) == 0 and L.pk_last_error()
    plain.bank_save(slot)                                   # the bank itself is as before
    assert plain.bank_get(0) == plain.snapshot(0)
    plain.close()
    bare = make(N, reward=False)
    bare.bank_create(2)
    L, h = bare._L, bare._h
    assert L.pk_bank_enable_episodes(h) < 0                 # no PK_F_REWARD
    assert L.pk_bank_checkpoint(h, slot.data_ptr(), 0, N, None) < 0
    assert L.pk_bank_resume(h, slot.data_ptr(), 0, N, None) < 0
    assert L.pk_bank_has_episodes(h) == 0
    bare.close()


def check_fork(env, dev):
    """VecEnv(48, batch_size=24, bank_slots=1, fork_slots=3) over two sub-batches: an episode
    checkpointed into a user slot and resumed two steps later brings its return and length along;
    after fork(dst, src) and identical actions the dst rows of obs, reward and done equal the src
    rows, and so do the episode return / length."""
    import pytest
    n = env.num_envs
    rng = np.random.default_rng(6)

    def step(pairs=()):
        """Random actions and coordinates (Script) for every env; env d of a pair gets env s's."""
        a, pos = rng.integers(0, 8, n), rng.integers(0, 6, (env.emu.n, 2))
        for d, s in pairs:
            a[d] = a[s]
            pos[env.phys(d)] = pos[env.phys(s)]
        env.emu.set_ram(0xD361, dev(pos, np.uint8))
        return env.step(dev(a, np.uint8))

    env.reset()
    step()
    step()
    ck = env.stats.ep_return[3].clone()
    env.checkpoint_to_bank([3], [0])
    step()
    step()
    env.resume_from_bank([40], [0])              # env 40 is now two steps into env 3's episode
    assert float(env.stats.ep_length[40]) == 2.0 and float(env.stats.ep_length[3]) == 4.0
    assert env.stats.ep_return[40] == ck
    env.resume_from_bank([41], [2])              # a scratch slot nothing was forked through yet
    assert env.emu.bank_rejects() == 1 and float(env.stats.ep_length[41]) == 4.0
    dst, src = [30, 47, 1, 25], [0, 5, 40, 0]
    with pytest.raises(ValueError):
        env.fork([1, 1], [0, 2])                 # a destination twice
    with pytest.raises(ValueError):
        env.fork([1, 5], [5, 0])                 # a destination that is a source
    with pytest.raises(ValueError):
        env.fork([1, 2, 3, 4], [5, 6, 7, 8])     # more distinct sources than scratch slots
    with pytest.raises(ValueError):
        env.fork([1, 2], [5])
    env.fork(dst, src)
    assert env.emu.bank_rejects() == 0
    obs = env.emu.obs
    for d, s in zip(dst, src):
        assert torch.equal(obs[env.phys(d)], obs[env.phys(s)]), (d, s)
        assert env.save_state(d) == env.save_state(s), (d, s)
    ended = 0
    for t in range(11):
        o, r, term, trunc, _ = step(list(zip(dst, src)))
        assert torch.equal(o[dst], o[src]), t
        assert torch.equal(r[dst], r[src]) and torch.equal(term[dst], term[src]) and torch.equal(trunc[dst], trunc[src]), t
        assert torch.equal(env.stats.ep_return[dst], env.stats.ep_return[src]), t
        assert torch.equal(env.stats.ep_length[dst], env.stats.ep_length[src]), t
        ended += int(term[dst].sum())
    assert ended == len(dst)                     # every forked episode ended inside the window


def check_pool_slots(make, dev):
    """VecEnv(48, batch_size=24, state_pool=two states, bank_slots=1, fork_slots=2, bank_episodes=True,
    archive_cells=4) in padded 64-env slots: start_slots — with the episode return and length — of a
    resumed, a forked and an explored env are the source's at its checkpoint, whichever sub-batch
    either is in; every other env, a rejected one included, keeps its own; a save_to_bank over a
    checkpointed slot makes the next resume from it a reject."""
    from pokegym_amd.env import VecEnv
    n, user = 48, 2                                  # slots: the pool's 0 and 1, the user's 2, fork 3-4, cells 5-8
    seed = make(2)
    seed.poke(0, 0xD361, bytes([2, 3]))
    seed.poke(1, 0xD361, bytes([4, 5]))
    pool = [seed.snapshot(0), seed.snapshot(1)]
    seed.close()
    emu = make(128, reward=True, reload_on_reset=True, max_episode_steps=1000)
    env = VecEnv(n, emulator=emu, batch_size=24, log_interval=0, state_pool=pool, bank_slots=1, fork_slots=2,
                 bank_episodes=True, archive_cells=4)
    assert env._padded and emu.bank_slots == 9 and env._arch0 == 5
    rng = np.random.default_rng(9)

    def step():
        env.emu.set_ram(0xD361, dev(rng.integers(0, 6, (emu.n, 2)), np.uint8))      # Script's walk: rewards differ
        env.step(dev(rng.integers(0, 8, n), np.uint8))

    def values():
        return {"slot": env.start_slots.cpu().numpy().copy(), "ret": env.stats.ep_return.cpu().numpy().copy(),
                "len": env.stats.ep_length.cpu().numpy().copy()}

    def moved(before, mapping, at, what):
        """Env d of mapping = {d: s} holds what env s held in record `at`, the others what they held before."""
        after = values()
        rest = [e for e in range(n) if e not in mapping]
        for k in after:
            assert after[k][list(mapping)].tobytes() == at[k][list(mapping.values())].tobytes(), (what, k)
            assert after[k][rest].tobytes() == before[k][rest].tobytes(), (what, k, "the others keep theirs")

    env.reset()
    start = values()["slot"]
    assert set(start.tolist()) == {0, 1}
    zeros, ones = np.flatnonzero(start == 0), np.flatnonzero(start == 1)
    step()
    step()
    # an env of the second sub-batch that started from slot 0, resumed over one of the first that started from 1
    src, dst = int(zeros[zeros >= 24][0]), int(ones[ones < 24][0])
    rejected = int(ones[ones < 24][1])
    env.checkpoint_to_bank([src], [user])
    ck = values()
    step()
    before = values()
    assert before["len"][dst] == 3.0 and ck["len"][src] == 2.0 and before["ret"][dst] != ck["ret"][src]
    env.resume_from_bank([dst, rejected], [user, 3])             # a scratch slot nothing was forked through yet
    assert emu.bank_rejects() == 1
    moved(before, {dst: src}, ck, "resume")
    assert values()["slot"][dst] == 0 and values()["slot"][rejected] == 1
    step()
    # fork both ways: a source of slot 1 in the first sub-batch, the resumed env (slot 0, a step behind)
    src1 = int(ones[ones < 24][2])
    pairs = {int(zeros[zeros >= 24][1]): src1, int(ones[ones >= 24][0]): dst, int(zeros[zeros < 24][0]): src1}
    before = values()
    env.fork(list(pairs), list(pairs.values()))
    assert emu.bank_rejects() == 0
    moved(before, pairs, before, "fork")
    assert [values()["slot"][d] for d in pairs] == [1, 0, 1] and [before["slot"][d] for d in pairs] == [0, 1, 0]
    step()
    # the archive: envs that started from slot 0 win every cell, envs that started from 1 explore
    slots = values()["slot"]
    before = values()
    won = env.archive_update(scores=dev(rng.random(n) + (slots == 0), np.float64), keys=dev(np.arange(n) % 4, np.int64))
    at_ck = values()
    moved(before, {}, before, "update")
    winner = {int(s): e for e, s in enumerate(won.cpu().numpy()) if s >= 0}
    assert len(winner) == 4 and all(slots[e] == 0 for e in winner.values())
    step()
    now = values()["slot"]
    explorers = [int(e) for half in (np.flatnonzero(now[:24] == 1)[:2], 24 + np.flatnonzero(now[24:] == 1)[:2]) for e in half]
    assert len(explorers) == 4
    before = values()
    drawn = env.archive_explore(masked(explorers, dev, n)).cpu().numpy()
    assert (drawn[explorers] >= 5).all() and (np.delete(drawn, explorers) == -1).all() and emu.bank_rejects() == 0
    mapping = {e: winner[int(drawn[e])] for e in explorers}
    moved(before, mapping, at_ck, "explore")
    assert (values()["slot"][explorers] == 0).all() and (values()["len"][explorers] == at_ck["len"][list(mapping.values())]).all()
    # a plain save over the checkpointed slot leaves it without an episode
    before = values()
    env.save_to_bank([0], [user])
    env.resume_from_bank([rejected], [user])
    assert emu.bank_rejects() == 1
    moved(before, {}, before, "resume from a slot saved over")
    emu.close()
