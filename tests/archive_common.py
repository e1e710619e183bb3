"""Shared scenarios of the exploration-archive tests (pk_archive_*, ABI v9): test_hostsim_archive.py
runs them on the host-simulation build, test_gpu_archive.py on the gfx950 build.  The oracle is the
sequential model of include/pokegym_amd.h, stated once here (Model); slot contents are checked
against snapshots, continuations against a twin handle that never had an archive."""
import math

import numpy as np
import torch

import episodes_common as ec

N = 128                 # two 64-env groups
MAX_STEPS = ec.MAX_STEPS
M64 = (1 << 64) - 1
NOKEY = M64
GOLD = 0x9E3779B97F4A7C15


def mix(z):
    """splitmix64's finaliser."""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


class Model:
    """The normative model: update walks the envs in ascending order, explore draws by prefix sums."""

    def __init__(self, n_cells, slot0, seed):
        self.n_cells, self.slot0, self.seed = n_cells, slot0, seed
        self.index, self.key, self.record, self.visits, self.picks = {}, [], [], [], []
        self.overflow = self.draw_calls = 0

    @property
    def used(self):
        return len(self.key)

    def update(self, keys, scores, lengths, mask=None, envs=None):
        """Returns slot_of_env_out over all envs (-1 outside `envs`, which the device leaves alone)."""
        out = np.full(len(keys), -1, np.int32)
        winner = {}
        for e in (range(len(keys)) if envs is None else envs):
            k, s = int(keys[e]), float(scores[e])
            if (mask is not None and not mask[e]) or k == NOKEY or math.isnan(s):
                continue
            c = self.index.get(k)
            if c is None:
                if self.used == self.n_cells:
                    self.overflow += 1
                    continue
                c = self.used
                self.index[k] = c
                self.key.append(k)
                self.record.append(None)
                self.visits.append(0)
                self.picks.append(0)
            self.visits[c] += 1
            rec = self.record[c]
            if rec is None or s > rec[0] or (s == rec[0] and int(lengths[e]) < rec[1]):
                self.record[c] = (s, int(lengths[e]))
                winner[c] = e
        for c, e in winner.items():
            out[e] = self.slot0 + c
        return out, winner

    def explore(self, n, masked):
        out = np.full(n, -1, np.int32)
        rejects = 0
        if self.used == 0:
            rejects = len(masked)
        else:
            prefix, run = [], 0
            for c in range(self.used):
                run += (1 << 32) // math.isqrt((self.visits[c] + self.picks[c] + 1) << 16)
                prefix.append(run)
            for e in masked:
                r = mix((self.seed + GOLD * ((self.draw_calls << 32) + e + 1)) & M64) % run
                c = next(c for c in range(self.used) if prefix[c] > r)
                out[e] = self.slot0 + c
            for e in masked:
                self.picks[out[e] - self.slot0] += 1
        self.draw_calls += 1
        return out, rejects

    def check(self, emu, what=""):
        """archive_read equals the model."""
        got = emu.archive_read()
        u = self.used
        assert got["used"] == u and got["overflow"] == self.overflow, (what, got["used"], u, got["overflow"], self.overflow)
        assert got["keys"][:u].tolist() == self.key, what
        assert got["scores"][:u].tolist() == [r[0] for r in self.record], what
        assert got["lengths"][:u].tolist() == [r[1] for r in self.record], what
        assert got["visits"][:u].tolist() == self.visits, what
        assert got["picks"][:u].tolist() == self.picks, what
        assert (got["keys"][u:] == NOKEY).all() and not got["visits"][u:].any() and not got["scores"][u:].any(), what
        return got


def k64(keys, dev):
    """Key words (python ints / uint64) as the int64 tensor the binding takes."""
    return dev(np.array(keys, np.uint64).view(np.int64), np.int64)


class Run:
    """A handle with bank, episode parts and archive, stepped by an episodes_common Script; keeps the
    step counter the device keeps per env (PK_R_TIME: steps since the env's last reset)."""

    def __init__(self, make, dev, n_cells, slot0=2, seed=7, archive=True, script_seed=3, steps=24, **kw):
        self.dev, self.n_cells, self.slot0 = dev, n_cells, slot0
        self.emu = make(N, reward=True, max_episode_steps=MAX_STEPS, **kw)
        self.sc = ec.Script(steps, N, script_seed, dev)
        self.t = 0
        self.length = np.zeros(N, np.int64)
        if archive:
            self.emu.bank_create(slot0 + n_cells)
            self.emu.bank_enable_episodes()
            self.emu.archive_create(slot0, n_cells, seed)
            assert self.emu.archive_cells == n_cells
        self.model = Model(n_cells, slot0, seed)
        self.out = dev(np.full(N, -7), np.int32)

    def reset(self, envs=None):
        if envs is None:
            self.emu.reset()
            self.length[:] = 0
        else:
            self.emu.reset(ec.masked(envs, self.dev, N))
            self.length[list(envs)] = 0

    def step(self, k=1):
        for _ in range(k):
            self.sc.step(self.emu, self.t)
            self.t += 1
            self.length += 1

    def prologue(self):
        """Four steps; two sets of envs are reset on the way, so step counters are 4, 2 and 1."""
        self.reset()
        self.step(2)
        self.reset([1, 5, 33, 40, 64, 77])
        self.step()
        self.reset([33, 65, 100])
        self.step()

    def update(self, keys, scores, mask=None, env0=0, count=None, check_slots=True):
        """One pk_archive_update checked against the model: the record, slot_of_env_out, no rejects,
        and every winner's slot holding the winner's snapshot taken before the call."""
        emu, dev = self.emu, self.dev
        count = N - env0 if count is None else count
        snap = emu.snapshot_range(0, N) if check_slots else None
        self.out.fill_(-7)
        emu.archive_update(k64(keys, dev), dev(scores, np.float64), None if mask is None else dev(mask, np.uint8),
                           env0, count, out=self.out)
        want, winner = self.model.update(keys, scores, self.length, mask, range(env0, env0 + count))
        want[:env0] = -7
        want[env0 + count:] = -7
        assert self.out.cpu().numpy().tolist() == want.tolist()
        self.model.check(emu)
        assert emu.bank_rejects() == 0
        if check_slots:
            for c, e in winner.items():
                assert emu.bank_get(self.slot0 + c) == bytes(snap[e]), (c, e)
        return winner

    def close(self):
        self.emu.close()


def step_and_autoreset(emu, sc, t):
    """One step, the outputs of every env, then the reset of the finished envs (as VecEnv does)."""
    sc.step(emu, t)
    out = ec.outputs(emu, range(N))
    emu.reset(emu.terminals.clone())
    return out


BASE_KEYS = [0x0000000100000005, 0x0000000200000005, 0x0000000100000006, 7, 8, 9, M64 - 1, 1 << 63,
             0x00000000FFFFFFFF, 0xFFFFFFFF00000000, 0, 0x0102030405060708]


def parity_inputs():
    """Keys with duplicates inside a wave, across waves and across the two groups, two pairs that
    differ only in their high / only in their low 32 bits, the reserved key, a NaN score, a mask,
    score ties with unequal step counters (the reset envs of Run.prologue) and full ties."""
    rng = np.random.default_rng(5)
    keys = [BASE_KEYS[(e * 7 + e // 64) % len(BASE_KEYS)] for e in range(N)]
    keys[0] = keys[1] = keys[2] = keys[66] = 7            # full tie of 0 and 2; env 1 is two steps in
    keys[100] = NOKEY
    scores = rng.integers(0, 3, N).astype(np.float64)
    scores[[0, 1, 2, 66]] = 2.0
    scores[33] = 0.0                                      # the other key-7 env with a short episode
    scores[50] = np.nan
    scores[10] = -0.0
    mask = np.ones(N, np.uint8)
    mask[[3, 70]] = 0
    return keys, scores, mask


def check_model_parity(make, dev, **kw):
    """Three updates — new cells; some improved and some not; nothing better — each equal to the
    model in archive_read, slot_of_env_out, rejects and the winners' slot contents.  Returns what
    the determinism scenario compares."""
    run = Run(make, dev, n_cells=40, **kw)
    run.prologue()
    keys, scores, mask = parity_inputs()
    w1 = run.update(keys, scores, mask)
    assert w1[run.model.index[7]] == 1                     # the tie on the score goes to the shorter episode
    assert len(w1) == run.model.used == len(BASE_KEYS)
    run.step()
    rng = np.random.default_rng(6)
    scores2 = scores + rng.integers(-1, 2, N)              # NaN stays NaN
    keys2 = list(keys)
    keys2[20], keys2[90] = 0xABCDEF, 0xABCDEF              # a new cell among known ones
    w2 = run.update(keys2, scores2, None)
    assert 0 < len(w2) < run.model.used
    run.step()
    best = {k: run.model.record[c][0] for k, c in run.model.index.items()}
    scores3 = np.array([best.get(k, 0.0) for k in keys2]) - 1.0
    scores3[run.length == run.length.max()] += 1.0         # equal scores, longer episodes
    w3 = run.update(keys2, scores3, None)
    assert not w3
    got = run.emu.archive_read()
    slots = [run.emu.bank_get(run.slot0 + c) for c in range(got["used"])]
    run.close()
    return got, slots


def check_determinism(make, dev):
    a, sa = check_model_parity(make, dev)
    b, sb = check_model_parity(make, dev)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True) if isinstance(a[k], np.ndarray) else a[k] == b[k], k
    assert sa == sb


def check_capacity(make, dev):
    run = Run(make, dev, n_cells=5)
    run.prologue()
    keys = [1000 + (e * 5) % 9 for e in range(N)]          # 9 distinct keys, first envs 0, 1, 2, ...
    scores = np.arange(N, dtype=np.float64) % 11
    run.update(keys, scores)
    first = {}
    for e, k in enumerate(keys):
        first.setdefault(k, e)
    assert run.model.key == sorted(first, key=first.get)[:5] and run.model.overflow > 0
    run.step()
    run.update(keys, scores + 1.0)                         # the five cells still update, the rest overflows again
    run.close()
    run = Run(make, dev, n_cells=N)                        # the index at its design load
    run.prologue()
    keys = [(e << 32) | (N - e) for e in range(N)]
    run.update(keys, np.zeros(N), check_slots=False)
    assert run.model.used == N and run.model.overflow == 0
    w = run.update(keys[::-1], np.ones(N), check_slots=False)
    assert len(w) == N and run.model.used == N
    run.close()


def check_continuation(make, dev):
    """explore twice: draws, picks and the call counter follow the model; a resumed env holds its
    slot's state and, fed the winner's later inputs, returns what the winner returned (the winner's
    later steps come from a twin handle that ran the same script without an archive)."""
    T2 = 6
    run = Run(make, dev, n_cells=16, seed=99, script_seed=13)
    twin = Run(make, dev, n_cells=16, archive=False, script_seed=13)
    for r in (run, twin):
        r.prologue()
    T1 = run.t
    keys = [e % 5 for e in range(N)]
    scores = np.random.default_rng(8).integers(0, 50, N).astype(np.float64)
    winner = run.update(keys, scores)
    source = {run.slot0 + c: e for c, e in winner.items()}
    rec = []
    for t in range(T2):
        rec.append(step_and_autoreset(twin.emu, twin.sc, T1 + t))
        ec.same(step_and_autoreset(run.emu, run.sc, T1 + t), rec[-1], ("an update leaves every env as it is", t))
    masks = ([3, 17, 64, 90, 127], [4, 65, 66])
    before = ec.outputs(run.emu, range(N))
    drawn = {}
    for m in masks:
        run.out.fill_(-7)
        run.emu.archive_explore(ec.masked(m, dev, N), out=run.out)
        want, rejects = run.model.explore(N, m)
        assert run.out.cpu().numpy().tolist() == want.tolist() and rejects == 0
        drawn.update({e: int(want[e]) for e in m})
    run.model.check(run.emu)
    assert run.emu.bank_rejects() == 0 and run.model.draw_calls == 2 and sum(run.model.picks) == len(drawn)
    after = ec.outputs(run.emu, range(N))
    others = [e for e in range(N) if e not in drawn]
    ec.same(before, after, "envs taking no part", others, others)
    dst = list(drawn)
    src = [source[drawn[e]] for e in dst]
    for e in dst:
        assert bytes(after["snap"][e]) == run.emu.bank_get(drawn[e]), e
    for t in range(T2):
        run.sc.copy_rows(T1 + T2 + t, dst, run.sc, T1 + t, src)
        out = step_and_autoreset(run.emu, run.sc, T1 + T2 + t)
        ec.same(out, rec[t], ("replay", t), dst, src)
    run.close()
    twin.close()
    # an empty archive: every masked env is a reject and stays as it is
    run = Run(make, dev, n_cells=4)
    run.prologue()
    before = ec.outputs(run.emu, range(N))
    run.emu.archive_explore(ec.masked([0, 9, 64], dev, N), out=run.out)
    want, rejects = run.model.explore(N, [0, 9, 64])
    assert rejects == 3 and run.emu.bank_rejects() == 3 and (run.out.cpu().numpy() == -1).all()
    ec.same(before, ec.outputs(run.emu, range(N)), "empty archive")
    run.model.check(run.emu)
    run.close()


def check_cell_keys(make, dev):
    rng = np.random.default_rng(4)
    emu = make(N, reward=False)
    badges = rng.integers(0, 256, (N, 1))
    pos = rng.integers(0, 256, (N, 5))                     # D35E map .. D361 y, D362 x
    emu.set_ram(0xD356, dev(badges, np.uint8))
    emu.set_ram(0xD35E, dev(pos, np.uint8))
    b = emu.get_ram(0xD356, 1).cpu().numpy().astype(np.uint64)[:, 0]
    p = emu.get_ram(0xD35E, 5).cpu().numpy().astype(np.uint64)
    assert np.array_equal(b, badges[:, 0]) and np.array_equal(p, pos)
    for shift in (0, 2):
        sh = np.uint64(shift)
        want = p[:, 0] | (p[:, 4] >> sh) << np.uint64(8) | (p[:, 3] >> sh) << np.uint64(16) | b << np.uint64(24)
        got = emu.cell_keys(shift).cpu().numpy()
        assert got.tolist() == want.astype(np.int64).tolist(), shift
        part = dev(np.full(N, -5), np.int64)
        emu.cell_keys(shift, out=part, env0=64, count=40)
        part = part.cpu().numpy()
        assert part[64:104].tolist() == got[64:104].tolist() and (part[:64] == -5).all() and (part[104:] == -5).all()
    assert emu._L.pk_cell_keys(emu._h, 8, part.ctypes.data, 0, N, None) < 0
    emu.close()


def check_guards(make, dev):
    def calls(emu):
        L, h = emu._L, emu._h
        k, s, o = dev(np.zeros(N), np.int64), dev(np.zeros(N), np.float64), dev(np.zeros(N), np.int32)
        assert L.pk_archive_update(h, k.data_ptr(), s.data_ptr(), None, 0, N, o.data_ptr(), None) < 0 and L.pk_last_error()
        assert L.pk_archive_explore(h, None, 0, N, o.data_ptr(), None) < 0 and L.pk_last_error()
        assert L.pk_archive_read(h, None, None, None, None, None, None, None) < 0 and L.pk_last_error()
        assert L.pk_archive_cells(h) == 0

    sc = ec.Script(4, N, 2, dev)
    emu = make(N, reward=True, max_episode_steps=MAX_STEPS)
    twin = make(N, reward=True, max_episode_steps=MAX_STEPS)
    for h in (emu, twin):
        h.reset()
        sc.step(h, 0)
    L, h = emu._L, emu._h
    assert L.pk_archive_create(h, 0, 4, 0) < 0 and L.pk_last_error()       # no bank
    emu.bank_create(6)
    assert L.pk_archive_create(h, 0, 4, 0) < 0 and L.pk_last_error()       # no episode parts
    calls(emu)
    emu.bank_enable_episodes()
    emu.bank_checkpoint(dev(ec.slot_map({9: 1}, N)))
    held = emu.bank_get(1)
    assert L.pk_archive_create(h, 3, 4, 0) < 0                             # a range past the bank
    assert L.pk_archive_create(h, 0, 0, 0) < 0
    calls(emu)
    emu.archive_create(2, 4, 0)
    assert L.pk_archive_create(h, 2, 4, 0) < 0 and L.pk_last_error()       # twice
    assert emu.archive_cells == 4
    k, s = dev(np.zeros(N), np.int64), dev(np.zeros(N), np.float64)
    assert L.pk_archive_update(h, k.data_ptr(), s.data_ptr(), None, 32, 8, None, None) < 0   # env0 not a multiple of 64
    assert L.pk_archive_update(h, None, s.data_ptr(), None, 0, N, None, None) < 0
    assert L.pk_archive_explore(h, None, 64, N, None, None) < 0            # end past n
    assert emu.archive_read()["used"] == 0
    assert emu.bank_get(1) == held and emu.bank_rejects() == 0
    for t in range(1, 3):
        sc.step(emu, t)
        sc.step(twin, t)
    ec.same(ec.outputs(emu, range(N)), ec.outputs(twin, range(N)), "the handle steps as before")
    emu.close()
    twin.close()


def check_ranges(make, dev, streams=None):
    """update over range 0, then over range 64, equals one call over both in the archive and in
    the slots; streams = a function (first, second) that runs the two calls on two streams."""
    res = []
    for split in (False, True):
        run = Run(make, dev, n_cells=40)
        run.prologue()
        keys, scores, mask = parity_inputs()
        k, s, m = k64(keys, dev), dev(scores, np.float64), dev(mask, np.uint8)
        if not split:
            run.emu.archive_update(k, s, m)
        elif streams is None:
            run.emu.archive_update(k, s, m, 0, 64)
            run.emu.archive_update(k, s, m, 64, 64)
        else:
            streams(lambda: run.emu.archive_update(k, s, m, 0, 64), lambda: run.emu.archive_update(k, s, m, 64, 64))
        run.model.update(keys, scores, run.length, mask)
        got = run.model.check(run.emu)
        res.append((got, [run.emu.bank_get(run.slot0 + c) for c in range(got["used"])]))
        run.close()
    assert res[0][1] == res[1][1]


def check_vecenv(env, dev):
    """VecEnv(48, batch_size=24, archive_cells=8) in padded slots: default keys and scores, the
    winners' episode return / length travel to the envs that explore, padding envs never show."""
    n = env.num_envs
    rng = np.random.default_rng(9)

    def step():
        pos = rng.integers(0, 3, (env.emu.n, 2))
        env.emu.set_ram(0xD361, dev(pos, np.uint8))
        return env.step(dev(rng.integers(0, 8, n), np.uint8))

    env.reset()
    for _ in range(3):
        step()
    keys = env.cell_keys().cpu().numpy()
    pos = env.emu.get_ram(0xD35E, 5).cpu().numpy()
    for e in (0, 23, 24, 47):
        p = pos[env.phys(e)].astype(np.int64)
        assert keys[e] == p[0] | p[4] << 8 | p[3] << 16 | int(env.emu.get_ram(0xD356, 1)[env.phys(e), 0]) << 24
    ret, length = env.stats.ep_return.clone(), env.stats.ep_length.clone()
    won = env.archive_update().cpu().numpy()
    st = env.archive_state()
    model = Model(8, env._arch0, 0)
    want, _ = model.update(keys.view(np.uint64), ret.cpu().numpy(), length.cpu().numpy())
    assert won.tolist() == want.tolist()
    assert st["used"] == model.used and st["overflow"] == model.overflow
    assert int(st["visits"].sum()) + st["overflow"] == n        # the 80 padding envs are nowhere
    assert st["keys"][:st["used"]].tolist() == model.key and st["scores"][:st["used"]].tolist() == [r[0] for r in model.record]
    step()
    step()
    masked = [2, 30, 47]
    m = np.zeros(n, np.uint8)
    m[masked] = 1
    before_ret, before_len = env.stats.ep_return.clone(), env.stats.ep_length.clone()
    drawn = env.archive_explore(dev(m, np.uint8)).cpu().numpy()
    assert env.emu.bank_rejects() == 0
    for e in range(n):
        if e in masked:
            w = int(np.flatnonzero(won == drawn[e])[0])
            assert env.stats.ep_return[e] == ret[w] and env.stats.ep_length[e] == length[w] == 3.0, e
            assert env.save_state(e) == env.emu.bank_get(int(drawn[e])), e
        else:
            assert drawn[e] == -1 and env.stats.ep_return[e] == before_ret[e] and env.stats.ep_length[e] == before_len[e]
    assert int(env.archive_state()["picks"].sum()) == len(masked)
    step()
