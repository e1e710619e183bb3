"""Shared scenarios of the generic-episode-part tests (pk_bank_enable_generic_episodes): checkpoints,
resumes, forks and the archive on a handle without the reward stack.  test_hostsim_generic.py runs
them on the host-simulation build, test_gpu_generic.py on the gfx950 build.  Everything runs the
benchmark ROM; the oracle needs no reference: the emulator is deterministic, so an env resumed from
a checkpoint and fed the same actions must return, bit for bit, what the env it was saved from
returned.  The probe rewards are checked against probes.model() besides.  make(n, **kw) builds an
emulator (4 frames per step), dev(values, dtype) a tensor on its device."""
import numpy as np
import pytest
import torch

import archive_common as ac
from pokegym_amd import _native
from pokegym_amd import probes as P

N = 128                 # two 64-env groups: a range call with env0 = 64 exists
MAX_STEPS = 9           # the sources are 5 steps in at the checkpoint: they truncate inside the 6 recorded steps
T1, T2 = 5, 6
PROBES, STACK = _native.PK_GEP_PROBES, _native.PK_GEP_STACK
FREE = 0xDA00           # a WRAM byte the benchmark ROM never writes (check_newmax asserts it)
# the 1,440-piece row (two passes of a workgroup over one chunk and a second chunk) and the 270-piece
# row, which is no multiple of the 256-thread pass
STACKS = ((2, 4, "hwc"), (4, 3, "chw"))
S = (0, 31, 63, 64, 100, 127)                       # checkpointed envs -> slots 0..5, both groups
# destination -> slot: both groups both ways, slots 0 and 2 twice
D = {5: 0, 33: 1, 62: 2, 65: 3, 101: 4, 126: 5, 68: 0, 70: 2}
RESET_EARLY = (5, 33, 65, 68, 20, 21)               # reset again before the checkpoint: another step counter
# rejected env -> (slot, its twin env: the same actions from the start, no resume)
REJECTS = {10: (6, 13), 11: (99, 14), 12: (7, 15)}  # an empty slot, a slot >= K, a slot filled by pk_bank_save
K = 9


def program():
    """pkbench's program, a NEWMAX probe and a NONE probe over two bytes the ROM leaves alone."""
    return P.pkbench_program() + [P.u8(FREE, op="newmax", weight=2.0), P.u8(FREE + 1)]


def row_bytes(stack):
    s, d, _ = stack
    return d * (144 // s) * (160 // s)


def layout_bytes(parts, m, stack):
    """The layout formula of include/pokegym_amd.h: 20 register words, m padded to 4 words, the stack row."""
    return 80 + (4 * ((m + 3) // 4 * 4) if parts & PROBES else 0) + (row_bytes(stack) if parts & STACK else 0)


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def slot_map(mapping, n=N):
    slot = np.full(n, -1, np.int32)
    for e, k in mapping.items():
        slot[e] = k
    return slot


def actions(steps, n, seed):
    """Seeded random actions; every rejected env's twin presses what the env presses."""
    acts = np.random.default_rng(seed).integers(0, 8, (steps, n)).astype(np.uint8)
    for e, (_, twin) in REJECTS.items():
        acts[:, twin] = acts[:, e]
    return acts


class Rig:
    """A handle without the reward stack with pkbench's probes and a frame stack, driven as VecEnv
    drives it (step, push, evaluate into the emulator's own reward and terminal arrays), with the
    numpy model of the probe state and of the step counter beside it: step() asserts the rewards, the
    terminals, the truncations and the features of every env against them."""

    def __init__(self, make, dev, parts, stack=STACKS[0], slots=K, max_steps=MAX_STEPS, n=N, traj=None):
        self.dev, self.n, self.max_steps, self.prog = dev, n, max_steps, program()
        self.emu = emu = make(n, reward=False, max_episode_steps=max_steps)
        emu.probes_create(self.prog)
        emu.stack_create(stack[0], stack[1], stack[2], "mean")
        emu.bank_create(slots)
        if traj == "before":
            emu.traj_enable()
        if parts is not None:
            assert emu._L.pk_bank_enable_generic_episodes(emu._h, parts) == 0
            assert emu.generic_parts == parts and emu.generic_episode_bytes == layout_bytes(parts, len(self.prog), stack)
            assert emu.bank_has_episodes
        if traj == "after":
            emu.traj_enable()
        self.parts = parts or 0
        self.feat = dev(np.zeros((n, len(self.prog))), np.int32)
        self.state = np.zeros((n, len(self.prog)), np.uint32)
        self.time = np.zeros(n, np.int64)

    def read(self, addr, length):
        return self.emu.get_ram(addr, length).cpu().numpy()

    def start(self):
        self.emu.reset()
        self.emu.stack_push(fill_only=True)
        self.emu.probes_eval(rebase_only=True, features=self.feat)
        P.model(self.prog, self.read, self.state, rebase_only=True)
        self.time[:] = 0

    def reset(self, envs):
        """A masked reset alone: the envs' stacks and probe words go stale, which is the point."""
        m = np.zeros(self.n, np.uint8)
        m[list(envs)] = 1
        self.emu.reset(self.dev(m, np.uint8))
        self.time[list(envs)] = 0

    def stack(self):
        return self.emu.stack.reshape(self.n, -1).cpu().numpy().copy()

    def step(self, acts, what=None, snap=True):
        emu = self.emu
        emu.step(self.dev(acts, np.uint8))
        emu.stack_push()
        emu.probes_eval(rewards=emu.rewards, terminals=emu.terminals, features=self.feat)
        self.time += 1
        r, done, v, _, _ = P.model(self.prog, self.read, self.state)
        out = {"rew": emu.rewards.cpu().numpy().copy(), "term": emu.terminals.cpu().numpy().copy(),
               "trunc": emu.truncations.cpu().numpy().copy(), "feat": self.feat.cpu().numpy().copy(),
               "stack": self.stack(), "screen": emu.screen.cpu().numpy().copy()}
        if snap:
            out["snap"] = emu.snapshot_range(0, self.n).copy()
        assert np.array_equal(bits64(out["rew"]), bits64(r)), what
        assert np.array_equal(out["trunc"] != 0, self.time >= self.max_steps), what
        assert np.array_equal(out["term"] != 0, done | (self.time >= self.max_steps)), what
        assert np.array_equal(out["feat"], v), what
        return out

    def resumed(self, mapping, ck_state, ck_time):
        """The model after a resume of env <- slot for the accepted pairs of `mapping`."""
        for e, k in mapping.items():
            self.time[e] = ck_time[k]
            if self.parts & PROBES:
                self.state[e] = ck_state[k]

    def close(self):
        self.emu.close()


def same(a, b, ea, eb, what, keys=None):
    """Bit-for-bit equality of the rows ea of record a and eb of record b."""
    for k in (a if keys is None else keys):
        x, y = a[k][list(ea)], b[k][list(eb)]
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k)


def ranges(call, slots, dev):
    """A bank call as two range calls, one per group."""
    t = dev(slots, np.int32)
    call(t, 0, 64)
    call(t, 64, 64)


# ---- 1. guards ------------------------------------------------------------------------------------

def check_guards(make, dev):
    """Every failure the header lists is a negative code that leaves the handle usable and unchanged;
    the reward stack's enable keeps refusing a handle without it; the exchange refuses generic parts;
    the bytes per slot follow the layout formula for parts 0..3."""
    emu = make(N, reward=False, max_episode_steps=MAX_STEPS)
    L, h = emu._L, emu._h
    enable, prog, stack = L.pk_bank_enable_generic_episodes, program(), STACKS[0]

    def said(text):
        return text in L.pk_last_error().decode(errors="replace")

    def off():
        return L.pk_bank_generic_parts(h) == 0 and L.pk_bank_generic_episode_bytes(h) == 0 and not L.pk_bank_has_episodes(h)

    assert enable(None, 0) < 0
    assert enable(h, 0) < 0 and said("no bank") and off()
    emu.bank_create(6)
    slots = dev(slot_map({0: 0, 64: 1}), np.int32)
    for call in (L.pk_bank_checkpoint, L.pk_bank_resume):               # before the enable
        assert call(h, slots.data_ptr(), 0, N, None) < 0 and said("no episode parts")
    assert L.pk_bank_enable_episodes(h) < 0 and said("PK_F_REWARD") and off()
    for bad in (4, 8, 0x80000000, 0x80000003, 7):
        assert enable(h, bad) < 0 and said("unknown parts") and off(), bad
    assert enable(h, PROBES) < 0 and said("no probe program") and off()
    assert enable(h, STACK) < 0 and said("no frame stack") and off()
    assert enable(h, PROBES | STACK) < 0 and off()
    emu.probes_create(prog)
    assert enable(h, STACK) < 0 and said("no frame stack") and off()
    assert enable(h, PROBES | STACK) < 0 and off()
    emu.stack_create(*stack, "mean")
    emu.reset()                                                         # the handle is usable after the failures
    emu.step(dev(np.zeros(N), np.uint8))
    emu.bank_save(slots)
    assert emu.bank_rejects() == 0
    assert enable(h, PROBES | STACK) == 0                                # a correct call after the failures
    assert L.pk_bank_generic_parts(h) == (PROBES | STACK | 0x80000000) and L.pk_bank_has_episodes(h) == 1
    assert L.pk_bank_generic_episode_bytes(h) == layout_bytes(3, len(prog), stack) == 80 + 4 * 8 + 4 * 72 * 80
    for again in (0, PROBES | STACK):
        assert enable(h, again) < 0 and said("already carries")
    assert L.pk_bank_generic_parts(h) == (PROBES | STACK | 0x80000000)
    assert L.pk_bank_enable_episodes(h) < 0 and said("PK_F_REWARD")     # after the generic enable too
    emu.bank_resume(slots)                                              # slots filled by a plain save: rejects
    assert emu.bank_rejects() == 2
    emu.bank_checkpoint(slots)
    emu.bank_resume(dev(slot_map({1: 0, 65: 1}), np.int32))
    assert emu.bank_rejects() == 0
    emu.archive_create(2, 4, 1)
    assert L.pk_archive_exchange_enable(h) < 0 and said("generic") and L.pk_archive_payload_bytes(h) == 0
    emu.close()
    for parts, st in ((0, STACKS[0]), (PROBES, STACKS[1]), (STACK, STACKS[1]), (STACK, STACKS[0])):
        rig = Rig(make, dev, parts, st, slots=2, n=64)                   # Rig asserts the formula
        assert rig.emu.generic_episode_bytes == {0: 80, PROBES: 80 + 32, STACK: 80 + row_bytes(st)}[parts]
        rig.close()
    bare = make(64, reward=False)                                        # parts = 0 needs neither feature
    bare.bank_create(1)
    assert bare.generic_parts is None
    bare.bank_enable_generic_episodes(probes=False, stack=False)
    assert bare.generic_parts == 0 and bare.generic_episode_bytes == 80
    bare.close()
    rew = make(64, reward=True, max_episode_steps=MAX_STEPS)
    rew.bank_create(2)
    assert rew._L.pk_bank_enable_generic_episodes(rew._h, 0) < 0 and said("reward stack")
    assert not rew.bank_has_episodes and rew.generic_parts is None
    rew.bank_enable_episodes()                                           # and the reward stack's own enable works
    assert rew.bank_has_episodes and rew.generic_parts is None and rew.generic_episode_bytes == 0
    assert rew._L.pk_bank_enable_generic_episodes(rew._h, 0) < 0
    rew.close()


# ---- 2. and 4. continuation against the twin ----------------------------------------------------------

def check_continuation(make, dev, parts=PROBES | STACK, stack=STACKS[0]):
    """Checkpoint six envs of both groups in two range calls, play on and record; then other envs of the
    same handle — stale in registers, probe words and stack — resume from the slots, several from one
    slot, and are fed the recorded actions.  With every part carried, every recorded quantity of a
    destination equals its source's at every step.  A part that was not asked for stays the
    destination's: its stack bytes are the ones it had, its rewards follow its own probe words (the
    model), while the registers — the truncation step — follow the source in every case.  A rejected env
    equals its untouched twin in every quantity at every step, and is counted."""
    rig = Rig(make, dev, parts, stack)
    emu = rig.emu
    acts = actions(T1 + 2 * T2, N, 17)
    rig.start()
    for t in range(T1):
        if t == 3:
            rig.reset(RESET_EARLY)
        rig.step(acts[t], t, snap=False)
    pre = {"stack": rig.stack(), "snap": emu.snapshot_range(0, N).copy()}
    ranges(emu.bank_checkpoint, slot_map({e: k for k, e in enumerate(S)}), dev)
    emu.bank_save(dev(slot_map({40: 7}), np.int32))
    rec0 = {"stack": rig.stack(), "snap": emu.snapshot_range(0, N).copy()}
    same(pre, rec0, range(N), range(N), "a checkpoint leaves every env as it is")
    for k, e in enumerate(S):                                            # the machine part is what a plain save stores
        assert emu.bank_get(k) == bytes(rec0["snap"][e]), e
    ck_state, ck_time = {k: rig.state[e].copy() for k, e in enumerate(S)}, {k: rig.time[e] for k, e in enumerate(S)}
    rec = [rig.step(acts[T1 + t], ("record", t)) for t in range(T2)]
    assert [int(r["trunc"][S[0]]) for r in rec] == [0, 0, 0, 1, 1, 1]    # the episode's end is inside
    assert not rec[-1]["trunc"][list(RESET_EARLY)].any()                 # the destinations' own counters are behind
    for e, k in D.items():                                               # every destination is stale in every part
        src = S[k]
        assert not np.array_equal(rec[-1]["stack"][e], rec0["stack"][src]) and rig.time[e] != ck_time[k]
    assert sum(not np.array_equal(rig.state[e], ck_state[k]) for e, k in D.items()) >= len(D) // 2
    before = {"stack": rig.stack(), "snap": emu.snapshot_range(0, N).copy()}
    assert emu.bank_rejects() == 0
    ranges(emu.bank_resume, slot_map({**D, **{e: k for e, (k, _) in REJECTS.items()}}), dev)
    assert emu.bank_rejects() == len(REJECTS)
    rig.resumed(D, ck_state, ck_time)
    after = {"stack": rig.stack(), "snap": emu.snapshot_range(0, N).copy()}
    dst, src = list(D), [S[k] for k in D.values()]
    others = sorted(set(range(N)) - set(dst))
    same(before, after, others, others, "a resume writes the accepted destinations only")
    same(after, rec0, dst, src, "the machines are the sources' at the checkpoint", keys=("snap",))
    if parts & STACK:
        same(after, rec0, dst, src, "the stack rows came with the slots", keys=("stack",))
    else:
        same(after, before, dst, dst, "the stack rows stay the destinations'", keys=("stack",))
    replay = acts[T1 + T2:].copy()
    replay[:, dst] = acts[T1:T1 + T2][:, src]
    full = ("rew", "term", "trunc", "feat", "stack", "screen", "snap") if parts == (PROBES | STACK) else None
    for t in range(T2):
        out = rig.step(replay[t], ("replay", t))                         # asserts rewards and features against the model
        same(out, rec[t], dst, src, ("replay", t),
             keys=full or ("trunc", "screen", "snap") + (("rew", "term", "feat") if parts & PROBES else ()))
        for e, (_, twin) in REJECTS.items():
            same(out, out, [e], [twin], ("a rejected env equals its twin", t, e))
    rig.close()


# ---- 3. NEWMAX keeps its maximum ----------------------------------------------------------------------

def check_newmax(make, dev):
    """One WRAM byte under a NEWMAX probe of weight 2, driven with set_ram: up to 50 (the destinations
    to 90), a checkpoint, down to 30, a second checkpoint, a resume into other envs, up to 40 and then to
    70.  With PK_GEP_PROBES the env resumed from the second slot pays nothing at 40 and 2 * 20 at 70:
    only above the checkpoint's maximum.  Without the part, after the rebase a caller makes today, it
    pays 2 * 10 and 2 * 30: from the lower value.  The first slot holds the byte at its maximum, where
    both pay 0 and 2 * 20.  Without the part and without a rebase the destination's own 90 stays."""
    srcs, first, second, kept = (3, 70), (5, 100), (6, 101), (7, 102)
    pays = {}
    for parts in (PROBES, 0):
        rig = Rig(make, dev, parts, STACKS[1], slots=4, max_steps=1000)
        emu, j = rig.emu, len(rig.prog) - 2
        acts = actions(8, N, 23)

        def put(values):
            emu.set_ram(FREE, dev(np.asarray(values, np.uint8).reshape(N, 1), np.uint8))

        def evaluate(what):
            rew = dev(np.zeros(N), np.float64)
            emu.probes_eval(set=True, rewards=rew)
            r, _, _, _, _ = P.model(rig.prog, rig.read, rig.state)
            got = rew.cpu().numpy()
            assert np.array_equal(bits64(got), bits64(r)), (parts, what)
            return got

        rig.start()
        up = np.full(N, 50)
        up[list(first + second + kept)] = 90
        put(up)
        for t in range(3):
            rig.step(acts[t], t, snap=False)
        assert np.array_equal(rig.read(FREE, 1)[:, 0], up)               # the ROM left the byte alone
        assert (rig.state[:, j] == up).all()
        emu.bank_checkpoint(dev(slot_map({srcs[0]: 0, srcs[1]: 1}), np.int32))
        ck = {0: (rig.state[srcs[0]].copy(), rig.time[srcs[0]]), 1: (rig.state[srcs[1]].copy(), rig.time[srcs[1]])}
        put(np.full(N, 30))
        rig.step(acts[3], "down", snap=False)
        emu.bank_checkpoint(dev(slot_map({srcs[0]: 2, srcs[1]: 3}), np.int32))
        ck.update({2: (rig.state[srcs[0]].copy(), rig.time[srcs[0]]), 3: (rig.state[srcs[1]].copy(), rig.time[srcs[1]])})
        mapping = {first[0]: 0, first[1]: 1, second[0]: 2, second[1]: 3, kept[0]: 2, kept[1]: 3}
        emu.bank_resume(dev(slot_map(mapping), np.int32))
        assert emu.bank_rejects() == 0
        rig.resumed(mapping, {k: v[0] for k, v in ck.items()}, {k: v[1] for k, v in ck.items()})
        assert rig.read(FREE, 1)[list(first), 0].tolist() == [50, 50] and rig.read(FREE, 1)[list(second), 0].tolist() == [30, 30]
        if not parts:   # the rebase a caller makes today for the envs whose machine was replaced
            m = np.zeros(N, np.uint8)
            m[list(first + second)] = 1
            emu.probes_eval(dev(m, np.uint8), rebase_only=True)
            P.model(rig.prog, rig.read, rig.state, m, rebase_only=True)
        evaluate("settle")                                               # what the other probes owe is paid here
        put(np.full(N, 40))
        at40 = evaluate(40)
        put(np.full(N, 70))
        at70 = evaluate(70)
        pays[parts] = {name: (at40[list(envs)].tolist(), at70[list(envs)].tolist())
                       for name, envs in (("first", first), ("second", second), ("kept", kept), ("src", srcs))}
        rig.close()
    assert pays[PROBES]["second"] == ([0.0, 0.0], [40.0, 40.0])
    assert pays[0]["second"] == ([20.0, 20.0], [60.0, 60.0])
    assert pays[PROBES]["first"] == pays[0]["first"] == ([0.0, 0.0], [40.0, 40.0])
    assert pays[PROBES]["kept"] == ([0.0, 0.0], [40.0, 40.0]) and pays[0]["kept"] == ([0.0, 0.0], [0.0, 0.0])
    assert pays[PROBES]["src"] == pays[0]["src"] == ([0.0, 0.0], [40.0, 40.0])


# ---- 5. the archive on a generic handle ---------------------------------------------------------------

def archive_run(make, dev, stack=STACKS[0], cells=8, slot0=2, seed=7):
    """Ten steps with an update per step under pk_frame_keys(16, 16, 4) keys and the accumulated probe
    reward as the score, two explores; everything the archive reports equals archive_common.Model.
    Every env of the second explore then continues like a twin env resumed from the same slot with
    pk_bank_resume.  Returns what a second run must repeat."""
    rig = Rig(make, dev, PROBES | STACK, stack, slots=slot0 + cells, max_steps=1000)
    emu = rig.emu
    emu.archive_create(slot0, cells, seed)
    model = ac.Model(cells, slot0, seed)
    acts = actions(14, N, 29)
    ret = dev(np.zeros(N), np.float64)
    out = dev(np.full(N, -7), np.int32)
    outs = []
    rig.start()

    def explore(envs, what):
        mask = np.zeros(N, np.uint8)
        mask[list(envs)] = 1
        out.fill_(-7)
        emu.archive_explore(dev(mask, np.uint8), out=out)
        want, rejects = model.explore(N, list(envs))
        got = out.cpu().numpy()
        assert got.tolist() == want.tolist() and rejects == 0 and emu.bank_rejects() == 0, what
        model.check(emu, what)
        rig.resumed({e: int(k) for e, k in enumerate(got) if k >= 0}, ck_state, ck_time)
        outs.append(got.copy())
        return got

    ck_state, ck_time = {}, {}
    for t in range(10):
        rig.step(acts[t], t, snap=False)
        ret += emu.rewards
        keys = emu.frame_keys(16, 16, 4).cpu().numpy().view(np.uint64)
        scores = ret.cpu().numpy().copy()
        out.fill_(-7)
        emu.archive_update(ac.k64(keys.tolist(), dev), dev(scores, np.float64), None, out=out)
        want, winner = model.update(keys.tolist(), scores, rig.time)
        assert out.cpu().numpy().tolist() == want.tolist(), t
        model.check(emu, t)
        assert emu.bank_rejects() == 0
        for c, e in winner.items():
            ck_state[slot0 + c], ck_time[slot0 + c] = rig.state[e].copy(), rig.time[e]
        outs.append(out.cpu().numpy().copy())
        if t == 4:
            explore((1, 40, 64, 90, 127), "first explore")
    assert model.used >= 2 and model.draw_calls == 1
    explored = (2, 33, 63, 65, 111)
    twins = (3, 34, 62, 66, 112)
    got = explore(explored, "second explore")
    mapping = {tw: int(got[e]) for e, tw in zip(explored, twins)}
    emu.bank_resume(dev(slot_map(mapping), np.int32))
    assert emu.bank_rejects() == 0
    rig.resumed(mapping, ck_state, ck_time)
    more = acts[10:].copy()
    more[:, list(twins)] = more[:, list(explored)]
    for t in range(3):
        o = rig.step(more[t], ("after the explore", t))
        same(o, o, explored, twins, ("explored env and resumed twin", t))
    got = emu.archive_read()
    rig.close()
    return got, outs


def check_archive(make, dev):
    a, oa = archive_run(make, dev)
    b, ob = archive_run(make, dev)
    for k in a:
        assert np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k], k
    assert len(oa) == len(ob) and all(np.array_equal(x, y) for x, y in zip(oa, ob))


# ---- trajectories in both orders ----------------------------------------------------------------------

def check_traj_orders(make, dev):
    """pk_traj_enable before or after the enable gives the slots their trajectory part: a checkpointed
    slot reports its source's origin, length and actions, and a resumed env continues the list."""
    for order in ("before", "after"):
        rig = Rig(make, dev, 0, STACKS[1], slots=3, max_steps=100, n=64, traj=order)
        emu = rig.emu
        acts = actions(6, 64, 31)
        rig.start()
        for t in range(4):
            rig.step(acts[t], t, snap=False)
        emu.bank_checkpoint(dev(slot_map({9: 1}, 64), np.int32))
        tr = emu.bank_trajectories(0, 3)
        assert tr["flags"].cpu().numpy().tolist() == [_native.PK_TRAJ_EMPTY, 0, _native.PK_TRAJ_EMPTY], order
        assert int(tr["length"][1]) == 4 and int(tr["origin"][1]) == -1
        assert tr["actions"][1, :4].cpu().numpy().tolist() == acts[:4, 9].tolist()
        rig.step(acts[4], 4, snap=False)
        emu.bank_resume(dev(slot_map({20: 1}, 64), np.int32))
        rig.resumed({20: 1}, {1: rig.state[20]}, {1: 4})
        rig.step(acts[5], 5, snap=False)
        mine = emu.trajectories(0, 64)
        assert int(mine["length"][20]) == 5 and int(mine["flags"][20]) == 0
        assert mine["actions"][20, :5].cpu().numpy().tolist() == acts[:4, 9].tolist() + [int(acts[5, 20])]
        emu.set_episode_params(5000, 1.0)                                # longer rows; never empties generic parts
        assert emu.traj_capacity >= 5000
        emu.bank_resume(dev(slot_map({21: 1}, 64), np.int32))
        assert emu.bank_rejects() == 0
        assert int(emu.trajectories(0, 64)["flags"][21]) & _native.PK_TRAJ_BROKEN      # the slot's actions stayed behind
        rig.close()


# ---- 6. VecEnv ----------------------------------------------------------------------------------------

def make_vecenv(make, **kw):
    from pokegym_amd.env import VecEnv
    emu = make(N, reward=False, max_episode_steps=1000)
    args = dict(emulator=emu, batch_size=64, log_interval=0, probes=program(), probe_features=True, frame_stack=4,
                stack_layout="hwc", bank_slots=2, bank_episodes="generic", fork_slots=2, archive_cells=8,
                archive_key="frame", record_trajectories=True)
    args.update(kw)
    return VecEnv(N, **args)


def check_vecenv(make, dev):
    """VecEnv(bank_episodes="generic"): a forked env returns what its source returns, step for step —
    observation (the stack), rewards, terminals, probe_values, episode return and length; an explored
    env shows the observation and the probe_values the winner had at its checkpoint; a cell's
    trajectory replays into the slot's machine."""
    env = make_vecenv(make)
    emu = env.emu
    assert emu.generic_parts == (PROBES | STACK) and emu.bank_slots == 2 + 2 + 8 and emu.archive_cells == 8
    acts = actions(16, N, 37)
    env.reset()
    for t in range(4):
        env.step(dev(acts[t], np.uint8))
    src, dst = [3, 70, 3], [10, 20, 100]
    env.fork(dst, src)
    assert emu.bank_rejects() == 0
    obs = env._logical(env._obs_buffer()).cpu().numpy()
    pv = env.probe_values.cpu().numpy()
    assert np.array_equal(obs[dst], obs[src]) and np.array_equal(pv[dst], pv[src])
    for t in range(4, 10):
        a = acts[t].copy()
        a[dst] = a[src]
        o, rew, term, trunc, _ = env.step(dev(a, np.uint8))
        o, rew, term, pv = o.cpu().numpy(), rew.cpu().numpy(), term.cpu().numpy(), env.probe_values.cpu().numpy()
        assert np.array_equal(o[dst], o[src]), t
        assert np.array_equal(bits64(rew[dst]), bits64(rew[src])) and np.array_equal(term[dst], term[src]), t
        assert np.array_equal(pv[dst], pv[src]), t
        for stat in (env.stats.ep_return, env.stats.ep_length):
            s = stat.cpu().numpy()
            assert np.array_equal(bits64(s[dst]), bits64(s[src])), t
    assert len({o[e].tobytes() for e in range(N)}) > 8                  # not a comparison of equal envs
    won = env.archive_update().cpu().numpy()
    at_ck = {"obs": env._logical(env._obs_buffer()).cpu().numpy().copy(), "pv": env.probe_values.cpu().numpy().copy(),
             "ret": env.stats.ep_return.cpu().numpy().copy(), "snap": emu.snapshot_range(0, N).copy()}
    winner = {int(s): e for e, s in enumerate(won) if s >= 0}
    assert winner
    for t in range(10, 13):
        env.step(dev(acts[t], np.uint8))
    mask = np.zeros(N, np.uint8)
    mask[[1, 64, 90]] = 1
    before = env.probe_values.cpu().numpy().copy()
    drawn = env.archive_explore(dev(mask, np.uint8)).cpu().numpy()
    assert (drawn[[1, 64, 90]] >= 0).all() and (np.delete(drawn, [1, 64, 90]) == -1).all()
    obs, pv, ret = env._logical(env._obs_buffer()).cpu().numpy(), env.probe_values.cpu().numpy(), env.stats.ep_return.cpu().numpy()
    for e in (1, 64, 90):
        w = winner[int(drawn[e])]
        assert np.array_equal(obs[e], at_ck["obs"][w]) and np.array_equal(pv[e], at_ck["pv"][w]), e
        assert bits64(ret[e]) == bits64(at_ck["ret"][w]), e
    rest = np.delete(np.arange(N), [1, 64, 90])
    assert np.array_equal(pv[rest], before[rest])
    # a cell's trajectory rebuilds the slot's machine on a handle of its own
    cell = int(drawn[1]) - env._arch0
    tr = env.archive_trajectory(cell)
    assert tr["replayable"] and tr["origin"] == -1
    assert len(tr["actions"]) == int(env.archive_state()["lengths"][cell]) > 0
    other = make(64, reward=False, max_episode_steps=1000)
    other.bank_create(1)
    other.traj_enable()
    other.bank_enable_generic_episodes(probes=False, stack=False)
    other.replay([tr["origin"]], [tr["actions"]], [len(tr["actions"])], [0])
    assert other.bank_get(0) == emu.bank_get(int(drawn[1])) == bytes(at_ck["snap"][winner[int(drawn[1])]])
    other.close()
    emu.close()


def check_vecenv_padded(make, dev):
    """VecEnv(48, batch_size=24, bank_episodes="generic", probe_features=True, frame_stack=2) in padded
    64-env slots: a checkpoint of the second sub-batch resumed into the first (and a resume from an empty
    slot), a fork both ways, an archive_update and an archive_explore.  After each of them probe_values,
    the episode return and length and the stack rows of the touched envs are the source's at its
    checkpoint, and their next step — fed the action the source took then — pays the source's reward
    and leaves the source's values.  Every env no call has touched yet, the rejected one and the
    neighbours of the touched ones among them, equals the same env of a twin that makes no bank call,
    in all of that and at every step."""
    from pokegym_amd.env import VecEnv
    n = 48

    def vecenv():
        return VecEnv(n, emulator=make(N, reward=False, max_episode_steps=1000), batch_size=24, log_interval=0,
                      reward=False, bank_episodes="generic", probes=P.pkbench_program(), probe_features=True,
                      frame_stack=2, bank_slots=2, fork_slots=2, archive_cells=4, archive_key="frame")

    env, twin = vecenv(), vecenv()
    assert env._padded and env.emu.generic_parts == (PROBES | STACK)
    acts = np.random.default_rng(43).integers(0, 8, (16, n)).astype(np.uint8)
    touched = set()

    def values(v):
        return {"pv": v.probe_values.cpu().numpy().copy(), "ret": bits64(v.stats.ep_return.cpu().numpy()).copy(),
                "len": v.stats.ep_length.cpu().numpy().copy(),
                "stack": v._logical(v.emu.stack).reshape(n, -1).cpu().numpy().copy()}

    def untouched(rec, other, what):
        rest = sorted(set(range(n)) - touched)
        same(rec, other, rest, rest, what)

    def step(t, press=None):
        """Step t of both, env d pressing press[d]: the actions, the rewards and the values after the step."""
        a = acts[t].copy()
        for d, action in (press or {}).items():
            a[d] = action
        rec = {"a": a, "rew": bits64(env.step(dev(a, np.uint8))[1].cpu().numpy()).copy(), **values(env)}
        other = {"rew": bits64(twin.step(dev(acts[t], np.uint8))[1].cpu().numpy()), **values(twin)}
        untouched({k: rec[k] for k in other}, other, ("the envs no call touched equal the twin's", t))
        log[t] = rec
        return rec

    def moved(before, mapping, at, what):
        """After a call: env d of mapping = {d: s} holds what env s held in record `at`, the others what
        they held before the call; the neighbours of every d are among the others."""
        after = values(env)
        dst = list(mapping)
        same(after, at, dst, [mapping[d] for d in dst], what)
        rest = sorted(set(range(n)) - set(dst))
        same(after, before, rest, rest, (what, "the others keep theirs"))
        touched.update(dst)

    def follows(t, mapping, u, what):
        """Step t, the first after a call: env d of mapping = {d: s} continues as env s did at step u."""
        rec = step(t, {d: log[u]["a"][s] for d, s in mapping.items()})
        dst = list(mapping)
        same(rec, log[u], dst, [mapping[d] for d in dst], what, keys=("rew", "pv", "ret", "len", "stack"))

    log = {}
    env.reset()
    twin.reset()
    for t in range(4):
        step(t)
    # a checkpoint of the second sub-batch, resumed two steps later into the first; slot 1 is empty
    src, dst, rejected = 30, 5, 7
    before = values(env)
    env.checkpoint_to_bank([src], [0])
    ck = values(env)
    same(ck, before, range(n), range(n), "a checkpoint leaves every env as it is")
    step(4)
    step(5)
    before = values(env)
    assert not np.array_equal(before["stack"][dst], ck["stack"][src]) and before["len"][dst] != ck["len"][src]
    env.resume_from_bank([dst, rejected], [0, 1])
    assert env.emu.bank_rejects() == 1
    moved(before, {dst: src}, ck, "resume")
    assert values(env)["len"][dst] == 4.0
    follows(6, {dst: src}, 4, "the step after the resume")
    assert rejected not in touched                                       # step() compared it with the twin's
    # a fork both ways; source 5 is two steps behind in its episode
    pairs = {6: 29, 40: 5, 20: 29}
    before = values(env)
    assert before["len"][5] != before["len"][40]
    env.fork(list(pairs), list(pairs.values()))
    assert env.emu.bank_rejects() == 0
    moved(before, pairs, before, "fork")
    rec = step(7, {d: acts[7][s] for d, s in pairs.items()})
    same(rec, rec, list(pairs), list(pairs.values()), "the step after the fork", keys=("rew", "pv", "ret", "len", "stack"))
    # the archive: the winners' values at the update come back at the explore, two steps later
    before = values(env)
    won = env.archive_update().cpu().numpy()
    at_ck = values(env)
    same(at_ck, before, range(n), range(n), "an update leaves every env as it is")
    winner = {int(s): e for e, s in enumerate(won) if s >= 0}
    assert winner and all(env._arch0 <= s < env._arch0 + 4 for s in winner)
    step(8)
    step(9)
    explorers = [4, 23, 24, 47]                                           # both ends of both sub-batches
    mask = np.zeros(n, np.uint8)
    mask[explorers] = 1
    before = values(env)
    drawn = env.archive_explore(dev(mask, np.uint8)).cpu().numpy()
    assert (drawn[explorers] >= 0).all() and (np.delete(drawn, explorers) == -1).all() and env.emu.bank_rejects() == 0
    mapping = {e: winner[int(drawn[e])] for e in explorers}
    assert any(before["len"][e] != at_ck["len"][w] for e, w in mapping.items())
    moved(before, mapping, at_ck, "explore")
    follows(10, mapping, 8, "the step after the explore")
    assert len({rec["stack"][e].tobytes() for e in range(n)}) > 8       # not a comparison of equal envs
    assert len(set(log[10]["ret"].tolist())) > 4
    env.emu.close()
    twin.emu.close()


def check_vecenv_errors(make, dev):
    """The constructor's rules; and a reward env with a frame stack still refills after a resume."""
    from pokegym_amd.env import VecEnv
    for kw, emu_kw in ((dict(bank_episodes="generic", bank_slots=1), dict(reward=True)),
                       (dict(bank_episodes=True, bank_slots=1), dict(reward=False)),
                       (dict(bank_episodes="generic", bank_slots=1, archive_cells=2, archive_exchange=True), dict(reward=False)),
                       (dict(bank_episodes="Generic", bank_slots=1), dict(reward=False)),
                       (dict(bank_episodes="generic"), dict(reward=False))):
        emu = make(64, **emu_kw)
        with pytest.raises(ValueError):
            VecEnv(64, emulator=emu, log_interval=0, **kw)
        emu.close()
    emu = make(64, reward=False)
    with pytest.raises(ValueError, match="needs the reward stack"):     # the error it raised before
        VecEnv(64, emulator=emu, log_interval=0, bank_episodes=True, bank_slots=1)
    emu.close()
    emu = make(64, reward=True, max_episode_steps=1000)
    env = VecEnv(64, emulator=emu, log_interval=0, bank_episodes=True, bank_slots=1, frame_stack=4)
    env.reset()
    acts = actions(4, 64, 41)
    for t in range(4):
        env.step(dev(acts[t], np.uint8))
    env.checkpoint_to_bank([2], [0])
    env.resume_from_bank([9], [0])
    st = emu.stack.cpu().numpy()
    assert all(np.array_equal(st[9][0], st[9][k]) for k in range(1, 4))  # refilled: four copies of one frame
    assert not all(np.array_equal(st[2][0], st[2][k]) for k in range(1, 4))
    emu.close()
