"""Shared scenarios of the action-trajectory tests (pk_traj_*, ABI v10): test_hostsim_traj.py runs
them on the host-simulation build, test_gpu_traj.py on the gfx950 build.  The oracles need no
reference.  A Python list model says what every env's trajectory must be after each call; and as
emulator and reward stack are deterministic, replaying a recorded trajectory from its recorded
origin on a second handle must rebuild the recorded env bit for bit.

Envs that must stay replayable are driven with actions only (no set_ram), on handles that reload on
every reset; the origin slots are made to differ once, by poking coordinates before a bank_save."""
import numpy as np

import episodes_common as ec

N = 70                   # two 64-env groups, the second partial
MAX_STEPS = 40           # cap_log2 = 10: rows of 768 bytes
CAP = 768
BROKEN, OVERFLOW, EMPTY = 1, 2, 4
POOL = (0, 1)            # origin slots with a state; slot 2 stays empty (a rejected origin)
EMPTY_SLOT = 2
CK0 = 4                  # first slot the scenarios checkpoint into
SLOTS = 24
# staggered resets: env -> steps it has made when the prologue ends (every other env: 33)
STAGGER = {0: 2, 9: 0, 31: 1, 32: 15, 40: 16, 63: 17, 64: 0, 66: 15, 69: 16}
STAGGER_ORIGIN = {0: EMPTY_SLOT, 9: 0, 31: 1, 32: -1, 40: 0, 63: 1, 64: EMPTY_SLOT, 66: 0, 69: 1}
PROLOGUE = 33


def sequential(first, second):
    first()
    second()


def slot_map(mapping, n=N):
    return ec.slot_map(mapping, n)


def make_pool(emu, dev):
    """Slots 0 and 1: the template with other coordinates (the reward stack reads them)."""
    emu.poke(0, 0xD361, bytes([2, 3]))
    emu.poke(1, 0xD361, bytes([4, 5]))
    emu.poke(1, 0xD35E, bytes([1]))
    emu.bank_save(dev(slot_map({0: 0, 1: 1}, emu.n)))


class Run:
    """A handle that records trajectories, next to the list model of what it must hold."""

    def __init__(self, make, dev, n=N, seed=5, reload=True, episodes=True, pool=True, par=sequential, **kw):
        kw.setdefault("reward", True)
        if kw["reward"]:
            kw["reload_on_reset"] = reload
        self.emu = make(n, max_episode_steps=MAX_STEPS, **kw)
        self.dev, self.n, self.par = dev, n, par
        self.emu.traj_enable()
        assert self.emu.traj_capacity == CAP
        self.origin, self.acts, self.flags = [-1] * n, [[] for _ in range(n)], [0] * n
        self.reloads = reload or not kw["reward"]
        self.was_reset = [False] * n
        if pool:
            self.emu.bank_create(SLOTS)
            if episodes:
                self.emu.bank_enable_episodes()
            make_pool(self.emu, dev)
            self.flags[0] = self.flags[1] = BROKEN         # poked
        self.rng = np.random.default_rng(seed)

    # -- the calls, mirrored into the model ---------------------------------------------------
    def reset(self, envs=None, slots=None, ranges=False):
        """Masked reset; slots: {env: origin slot} (others: the template)."""
        envs = list(range(self.n)) if envs is None else list(envs)
        mask = ec.masked(envs, self.dev, self.n)
        if slots is None:
            self.emu.reset(mask)
        elif ranges:
            sm = self.dev(slot_map(slots, self.n))
            self.par(lambda: self.emu.reset_range_from(0, 64, sm, mask),
                     lambda: self.emu.reset_range_from(64, self.n - 64, sm, mask))
        else:
            self.emu.reset_from(self.dev(slot_map(slots, self.n)), mask)
        for e in envs:
            reloaded = self.reloads or not self.was_reset[e]
            s = (slots or {}).get(e, -1)
            self.origin[e] = s if (reloaded and s in POOL) else -1
            self.acts[e] = []
            self.flags[e] = 0 if reloaded else BROKEN
            self.was_reset[e] = True

    def step(self, acts=None, ranges=False):
        a = self.rng.integers(0, 8, self.n).astype(np.uint8) if acts is None else np.asarray(acts, np.uint8)
        t = self.dev(a, np.uint8)
        if ranges:
            self.par(lambda: self.emu.step_range(0, t[:64]), lambda: self.emu.step_range(64, t[64:]))
        else:
            self.emu.step(t)
        for e in range(self.n):
            if len(self.acts[e]) < CAP:
                self.acts[e].append(int(a[e]))
            else:
                self.flags[e] |= OVERFLOW
        return a

    def prologue(self, ranges=False):
        """PROLOGUE steps with masked resets in between, from the template, from the two pool
        slots and from the empty one, so that the envs of STAGGER end at their lengths."""
        self.reset()
        for t in range(PROLOGUE + 1):
            due = [e for e, k in STAGGER.items() if PROLOGUE - k == t]
            if due:
                self.reset(due, {e: STAGGER_ORIGIN[e] for e in due}, ranges=ranges)
            if t < PROLOGUE:
                self.step(ranges=ranges)
        assert self.emu.bank_rejects() == sum(1 for s in STAGGER_ORIGIN.values() if s == EMPTY_SLOT)

    def checkpoint(self, mapping):
        self.emu.bank_checkpoint(self.dev(slot_map(mapping, self.n)))
        return {k: (self.origin[e], list(self.acts[e]), self.flags[e]) for e, k in mapping.items()}

    def take(self, env, rec):
        """env continues the episode of a checkpoint record."""
        self.origin[env], self.acts[env], self.flags[env] = rec[0], list(rec[1]), rec[2]

    # -- comparisons --------------------------------------------------------------------------
    def want(self, origin, acts, flags):
        row = np.full(CAP, 0xFF, np.uint8)
        row[:len(acts)] = acts
        return origin, len(acts), flags, row.tobytes()

    def check(self, envs=None, what=""):
        d = host(self.emu.trajectories())
        for e in (range(self.n) if envs is None else envs):
            got = (int(d["origin"][e]), int(d["length"][e]), int(d["flags"][e]), d["actions"][e].tobytes())
            assert got[:3] == self.want(self.origin[e], self.acts[e], self.flags[e])[:3], (what, e, got[:3])
            assert got[3] == self.want(self.origin[e], self.acts[e], self.flags[e])[3], (what, e, "actions")

    def check_slot(self, slot, rec, what=""):
        d = host(self.emu.bank_trajectories(slot, 1))
        got = (int(d["origin"][0]), int(d["length"][0]), int(d["flags"][0]), d["actions"][0].tobytes())
        assert got == self.want(*rec), (what, slot, got[:3])

    def close(self):
        self.emu.close()


def host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def same_traj(a, b, envs, what):
    for k in a:
        assert a[k][envs].tobytes() == b[k][envs].tobytes(), (what, k)


# -- 1. recording ---------------------------------------------------------------------------------
def check_recording(make, dev, par=sequential):
    """Random actions with masked resets from the template, the pool slots and a rejected slot, the
    steps and resets issued as two sub-batch ranges (on two streams where there are streams)."""
    run = Run(make, dev, par=par)
    run.check(what="fresh handle")
    run.prologue(ranges=True)
    run.check(what="prologue")
    lengths = sorted({len(a) for a in run.acts})
    assert lengths == [0, 1, 2, 15, 16, 17, 33]
    assert {run.origin[e] for e in STAGGER} == {-1, 0, 1}
    for _ in range(3):
        run.step(ranges=True)
    run.check(what="three more steps")
    # sub-range reads: the same rows, and nothing outside the range is written
    d = host(run.emu.trajectories(64, 6))
    full = host(run.emu.trajectories())
    for k in d:
        assert d[k].tobytes() == full[k][64:].tobytes(), k
    run.close()
    # without the reward stack every reset reloads
    bare = Run(make, dev, reward=False, episodes=False)
    bare.reset()
    bare.step()
    bare.reset([3, 65], {3: 1, 65: EMPTY_SLOT})
    bare.step()
    bare.check(what="no reward stack")
    assert bare.origin[3] == 1 and bare.origin[65] == -1 and len(bare.acts[3]) == 1 and len(bare.acts[4]) == 2
    bare.close()


# -- 2. travel ------------------------------------------------------------------------------------
SRC = (9, 31, 32, 40, 63, 5)             # lengths 0, 1, 15, 16, 17, 33 -> slots CK0 ..
# destination -> source index: other sub-blocks, the other group both ways, one slot twice
DST = {33: 0, 1: 1, 65: 2, 20: 3, 68: 4, 47: 5, 64: 2}
REJECTED = {10: EMPTY_SLOT, 50: 0, 67: SLOTS + 3}     # empty, no episode part, out of range


def travel(make, dev, with_twin=True):
    """Prologue, checkpoint of SRC, three steps, resume of DST (and three rejects), four steps; a
    twin handle that makes the same steps without any bank call.  Returns the run, its checkpoint
    records and the envs' snapshots at the checkpoint."""
    run = Run(make, dev)
    run.prologue()
    if not with_twin:
        twin = None
    else:
        twin = Run(make, dev)
        twin.prologue()
    recs = run.checkpoint({e: CK0 + k for k, e in enumerate(SRC)})
    snaps = {e: run.emu.snapshot(e) for e in SRC}
    for k, e in enumerate(SRC):
        run.check_slot(CK0 + k, recs[CK0 + k], "slot = source at the checkpoint")
        assert len(recs[CK0 + k][1]) == (0, 1, 15, 16, 17, 33)[k]
    run.check(what="a checkpoint leaves the envs alone")
    for _ in range(3):
        a = run.step()
        if twin is not None:
            twin.step(a)
    run.emu.bank_resume(dev(slot_map({**{d: CK0 + k for d, k in DST.items()}, **REJECTED})))
    assert run.emu.bank_rejects() == len(REJECTED)
    for d, k in DST.items():
        run.take(d, recs[CK0 + k])
        assert run.emu.snapshot(d) == snaps[SRC[k]]
    run.check(what="resumed")
    for _ in range(4):
        a = run.step()
        if twin is not None:
            twin.step(a)
    run.check(what="resumed, then its own actions")
    for k, e in enumerate(SRC):              # the slots did not move
        run.check_slot(CK0 + k, recs[CK0 + k], "slot after the resumes")
    if twin is not None:
        others = [e for e in range(N) if e not in DST]
        same_traj(host(run.emu.trajectories()), host(twin.emu.trajectories()), others, "non-participants and rejects")
        twin.close()
    return run, recs, snaps


def check_travel(make, dev):
    run, _, _ = travel(make, dev)
    run.close()


def check_fork(env, dev):
    """VecEnv(48, batch_size=24, bank_slots=1, fork_slots=3, record_trajectories=True) on a handle
    that reloads on every reset: a fork destination's trajectory is the source's at the fork plus
    its own later actions; logical env indices go through phys()."""
    n = env.num_envs
    rng = np.random.default_rng(6)
    acts = [[] for _ in range(n)]

    def step():
        a = rng.integers(0, 8, n)
        env.step(dev(a, np.uint8))
        for e in range(n):
            acts[e].append(int(a[e]))

    env.reset()
    for _ in range(3):
        step()
    dst, src = [30, 47, 1, 25], [0, 5, 40, 0]
    env.fork(dst, src)
    assert env.emu.bank_rejects() == 0
    for d, s in zip(dst, src):
        acts[d] = list(acts[s])
    for _ in range(2):
        step()
    for e in dst + src + [24, 23]:
        t = env.trajectory(e)
        assert t["origin"] == -1 and t["replayable"] and t["actions"].tolist() == acts[e], e
    t = env.slot_trajectory(env._fork0)      # the scratch slot of the first distinct source, env 0
    assert t["actions"].tolist() == acts[0][:3] and t["replayable"]
    t = env.slot_trajectory(0)               # the user's slot: nothing was checkpointed into it
    assert t["origin"] == -1 and len(t["actions"]) == 0 and not t["replayable"]


# -- 3. replay oracle -----------------------------------------------------------------------------
def check_replay(make, dev):
    """replay() of recorded trajectories — sources, resumed envs (another env's past plus their
    own actions) and untouched ones — on a second handle with the same pool rebuilds each env's
    machine state, and resumed from the rebuilt slots the envs continue as the originals do."""
    run, _, _ = travel(make, dev, with_twin=False)
    envs = [9, 31, 32, 5, 33, 65, 64, 47, 66, 69, 12]
    d = host(run.emu.trajectories())
    assert not d["flags"][envs].any()
    assert {int(d["origin"][e]) for e in envs} == {-1, 0, 1}
    rep = Run(make, dev, seed=99)
    slots = [CK0 + i for i in range(len(envs))]
    rep.emu.replay(d["origin"][envs], d["actions"][envs], d["length"][envs], slots, flags=d["flags"][envs])
    for e, s in zip(envs, slots):
        assert rep.emu.bank_get(s) == run.emu.snapshot(e), ("machine state", e)
    t = host(rep.emu.bank_trajectories(CK0, len(envs)))
    for k in ("origin", "length", "flags", "actions"):
        assert t[k].tobytes() == d[k][envs].tobytes(), ("the rebuilt slots carry the trajectories", k)
    # the same envs of the second handle continue the rebuilt episodes
    rep.emu.bank_resume(dev(slot_map(dict(zip(envs, slots)))))
    assert rep.emu.bank_rejects() == 0
    ended = False
    for t in range(6):                       # across the episodes' ends (lengths up to 40)
        a = run.step()
        rep.step(a)
        ec.same(ec.outputs(run.emu, envs), ec.outputs(rep.emu, envs), ("continuation", t))
        ended = ended or bool(run.emu.terminals[47])    # resumed at 33 steps, 37 when travel() ends
    assert ended
    run.close()
    rep.close()


# -- 4. flags -------------------------------------------------------------------------------------
def check_flags(make, dev):
    run = Run(make, dev)
    run.reset()
    run.step()
    run.step()
    state = run.emu.snapshot(11)
    run.emu.bank_load(dev(slot_map({3: 0, 65: 1, 30: EMPTY_SLOT})))   # env 30 is rejected: untouched
    assert run.emu.bank_rejects() == 1
    run.emu.load_env(7, state)
    run.emu.poke(9, 0xD362, bytes([1]))
    for e in (3, 65, 7, 9):
        run.flags[e] = BROKEN
    run.check(what="bank_load, load_env and poke flag the envs they touch")
    run.step()
    run.check(what="recording goes on")
    d = host(run.emu.trajectories())
    with_flags = [3, 4]
    try:
        run.emu.replay(d["origin"][with_flags], d["actions"][with_flags], d["length"][with_flags], [CK0, CK0 + 1],
                       flags=d["flags"][with_flags])
        raise AssertionError("replay() took a broken trajectory")
    except ValueError:
        pass
    run.check(what="a refused replay touches nothing")
    run.reset([3, 7], {3: 1})
    run.check(what="a reloading reset clears the flags")
    run.emu.set_ram(0xD361, dev(np.zeros((N, 1)), np.uint8))
    run.flags = [f | BROKEN for f in run.flags]
    run.check(what="set_ram flags every env")
    run.close()
    # the reference's reset rule: only an env's first reset reloads
    keep = Run(make, dev, reload=False)
    keep.reset(range(0, N, 2), {4: 1})
    keep.step()
    keep.check(what="first resets reload")
    assert keep.origin[4] == 1 and keep.flags[4] == 0
    keep.reset([4, 5], {4: 0, 5: 0})         # env 4's second reset, env 5's first
    keep.check(what="a reset that keeps the machine")
    assert (keep.origin[4], keep.flags[4], keep.origin[5], keep.flags[5]) == (-1, BROKEN, 0, 0)
    try:
        keep.emu.replay([-1], [np.zeros(2, np.uint8)], [2], [CK0], envs=[4])
        raise AssertionError("replay() on an env whose resets no longer reload")
    except ValueError:
        pass
    keep.close()


def check_overflow(make, dev):
    """64 envs of one-frame steps stepped CAP + 1 times without a reset."""
    emu = make(64, frame_skip=1, release_frame=0, reward=False, render=False, max_episode_steps=MAX_STEPS)
    emu.traj_enable()
    rng = np.random.default_rng(3)
    acts = rng.integers(0, 8, (CAP + 1, 64)).astype(np.uint8)
    dacts = dev(acts, np.uint8)
    for t in range(CAP):
        emu.step(dacts[t])
    d = host(emu.trajectories())
    assert (d["length"] == CAP).all() and not d["flags"].any()
    emu.step(dacts[CAP])
    d = host(emu.trajectories())
    assert (d["length"] == CAP).all() and (d["flags"] == OVERFLOW).all() and (d["origin"] == -1).all()
    assert d["actions"].tobytes() == np.ascontiguousarray(acts[:CAP].T).tobytes()
    emu.close()


# -- 5. archive -----------------------------------------------------------------------------------
A0, CELLS = 8, 8


def check_archive(make, dev):
    """Records and draws of the archive carry trajectories through the checkpoint / resume path."""
    run = Run(make, dev)
    run.emu.archive_create(A0, CELLS, 7)
    run.prologue()
    keys = np.arange(N, dtype=np.int64) % 5
    scores = run.rng.random(N)
    out = dev(np.full(N, -7), np.int32)
    run.emu.archive_update(dev(keys, np.int64), dev(scores, np.float64), None, out=out)
    won = out.cpu().numpy()
    winners = {int(s): e for e, s in enumerate(won) if s >= 0}
    assert len(winners) == 5
    recs = {s: (run.origin[e], list(run.acts[e]), run.flags[e]) for s, e in winners.items()}
    for s in winners:
        run.check_slot(s, recs[s], "a winner's slot")
    lengths = run.emu.archive_read()["lengths"]
    for s in winners:
        assert lengths[s - A0] == len(recs[s][1])
    run.step()
    run.step()
    explorers = [2, 33, 64, 69, 20]
    run.emu.archive_explore(ec.masked(explorers, dev, N), out=out)
    drawn = out.cpu().numpy()
    assert run.emu.bank_rejects() == 0
    for e in explorers:
        assert drawn[e] in winners
        run.take(e, recs[int(drawn[e])])
    run.check(what="explorers carry their cell's trajectory")
    run.step()
    run.check(what="and append their own actions")
    run.close()


def check_archive_vecenv(env, make, dev):
    """VecEnv(N, state_pool=2 states, bank_episodes, archive_cells, record_trajectories) over an
    emulator that reloads on every reset: archive_trajectory(cell), replayed on a second handle whose
    bank holds the same pool, reaches the cell's recorded length and its slot's machine state."""
    rng = np.random.default_rng(8)
    env.reset()
    for t in range(6):
        env.step(dev(rng.integers(0, 8, N), np.uint8))
        if t == 2:
            env.archive_update(scores=dev(rng.random(N), np.float64), keys=dev(np.arange(N) % 3, np.int64))
    env.archive_update(scores=dev(rng.random(N) + 1.0, np.float64), keys=dev(np.arange(N) % 4, np.int64))
    st = env.archive_state()
    assert st["used"] == 4 and set(st["lengths"][:4].tolist()) <= {3, 6} and 6 in st["lengths"][:4]
    rep = Run(make, dev, pool=False)
    rep.emu.bank_create(SLOTS)
    rep.emu.bank_enable_episodes()
    for k in range(env.pool_size):
        rep.emu.bank_put(k, env.emu.bank_get(k))
    trajs = [env.archive_trajectory(c) for c in range(4)]
    assert all(t["replayable"] for t in trajs) and {t["origin"] for t in trajs} <= {0, 1}
    rep.emu.replay([t["origin"] for t in trajs], [t["actions"] for t in trajs], [len(t["actions"]) for t in trajs],
                   [CK0 + c for c in range(4)])
    for c in range(4):
        assert len(trajs[c]["actions"]) == st["lengths"][c]
        assert rep.emu.bank_get(CK0 + c) == env.emu.bank_get(env._arch0 + c), c
    rep.close()
    try:
        env.archive_trajectory(env.archive_cells)
        raise AssertionError("no such cell")
    except ValueError:
        pass


# -- 6. guards ------------------------------------------------------------------------------------
def check_guards(make, dev):
    # a handle that never enables trajectories
    plain = make(N, reward=True, max_episode_steps=MAX_STEPS)
    L, h = plain._L, plain._h
    plain.bank_create(4)
    plain.bank_enable_episodes()
    buf = dev(np.zeros(N), np.int32)
    assert plain.traj_capacity == 0
    assert L.pk_traj_get(h, 0, N, buf.data_ptr(), None, None, None, None) < 0 and L.pk_last_error()
    assert L.pk_bank_traj_get(h, 0, 1, buf.data_ptr(), None, None, None, None) < 0
    plain.reset()
    plain.step(dev(np.full(N, 3), np.uint8))
    plain.bank_checkpoint(dev(slot_map({9: 0})))
    plain.step(dev(np.full(N, 1), np.uint8))
    before = plain.snapshot(9)
    plain.bank_checkpoint(dev(slot_map({9: 1})))
    plain.bank_resume(dev(slot_map({20: 1, 21: 3})))           # slot 3 is empty
    assert plain.bank_rejects() == 1 and plain.snapshot(20) == before == plain.bank_get(1)
    plain.close()
    # both orders of traj_enable and bank_enable_episodes
    for traj_first in (True, False):
        emu = make(N, reward=True, reload_on_reset=True, max_episode_steps=MAX_STEPS)
        emu.bank_create(4)
        if traj_first:
            emu.traj_enable()
            emu.bank_enable_episodes()
        else:
            emu.bank_enable_episodes()
            emu.traj_enable()
        assert emu._L.pk_traj_enable(emu._h) < 0                # once
        assert emu.traj_capacity == CAP
        emu.reset()
        for a in (3, 1, 4):
            emu.step(dev(np.full(N, a), np.uint8))
        emu.bank_checkpoint(dev(slot_map({9: 0, 69: 2})))
        d = host(emu.bank_trajectories(0, 4))
        assert d["length"].tolist() == [3, 0, 3, 0] and d["flags"].tolist() == [0, EMPTY, 0, EMPTY]
        assert d["origin"].tolist() == [-1] * 4
        assert d["actions"][2, :4].tolist() == [3, 1, 4, 0xFF] and (d["actions"][1] == 0xFF).all()
        emu.bank_save(dev(slot_map({9: 0})))                    # a plain save empties the part
        assert host(emu.bank_trajectories(0, 1))["flags"].tolist() == [EMPTY]
        # argument guards
        L, h = emu._L, emu._h
        buf = dev(np.zeros(N), np.int32)
        assert L.pk_traj_get(h, 32, 6, buf.data_ptr(), None, None, None, None) < 0      # env0 not a multiple of 64
        assert L.pk_traj_get(h, 64, 7, buf.data_ptr(), None, None, None, None) < 0      # end past n
        assert L.pk_traj_get(h, 0, 0, buf.data_ptr(), None, None, None, None) < 0
        assert L.pk_bank_traj_get(h, 3, 2, buf.data_ptr(), None, None, None, None) < 0  # slots past the bank
        assert L.pk_bank_traj_get(h, 0, 0, buf.data_ptr(), None, None, None, None) < 0
        assert L.pk_traj_get(h, 64, 6, None, None, None, None, None) == 0               # every pointer may be NULL
        if traj_first:
            # growth of the seen set: new rows, every env BROKEN until its next reloading reset
            emu.set_episode_params(4000, 4.0)
            assert emu.traj_capacity == 6144
            d = host(emu.trajectories())
            assert (d["flags"] == BROKEN).all() and d["actions"].shape == (N, 6144)
            assert host(emu.bank_trajectories(0, 4))["flags"].tolist() == [EMPTY] * 4
            emu.reset(ec.masked(range(1, N), dev))
            for a in (2, 5):
                emu.step(dev(np.full(N, a), np.uint8))
            emu.bank_checkpoint(dev(slot_map({9: 1})))
            emu.bank_resume(dev(slot_map({66: 1})))
            emu.step(dev(np.full(N, 7), np.uint8))
            d = host(emu.trajectories())
            assert d["flags"].tolist() == [BROKEN] + [0] * (N - 1)
            assert d["length"].tolist() == [6] + [3] * (N - 1)
            assert d["actions"][66, :4].tolist() == [2, 5, 7, 0xFF] and d["actions"][9, :4].tolist() == [2, 5, 7, 0xFF]
            assert host(emu.bank_trajectories(1, 1))["actions"][0, :3].tolist() == [2, 5, 0xFF]
        emu.close()
    # without a bank, and without the reward stack: trajectories alone
    bare = make(N, reward=False, max_episode_steps=MAX_STEPS)
    bare.traj_enable()
    assert bare._L.pk_bank_traj_get(bare._h, 0, 1, None, None, None, None, None) < 0    # no bank
    bare.set_episode_params(4000, 4.0)
    assert bare.traj_capacity == 6144
    bare.close()
