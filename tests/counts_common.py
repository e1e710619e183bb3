"""Shared scenarios of the visit-count tests (pk_counts_*): test_hostsim_counts.py runs them on the
host-simulation build, test_gpu_counts.py on the gfx950 build.  The oracle is the model of
include/pokegym_amd.h, stated once here (Model).  Keys travel as int64 tensors holding the 64 key
bits; the model works on Python ints."""
import numpy as np
import pytest

N = 128                 # two 64-env groups
LG = 10
LIMIT = 768             # 3 * 2^(LG - 2)
M64 = (1 << 64) - 1
NOKEY = M64


def mix(z):
    """splitmix64's finaliser over a uint64 array (products mod 2^64)."""
    z = np.asarray(z, np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def chain_keys(bucket, k, lg=LG):
    """k keys whose probes all start at entry `bucket` of a 2^lg-entry table (found on the CPU)."""
    cand = np.arange(1, 1 << 18, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    hit = cand[(mix(cand) & np.uint64((1 << lg) - 1)) == np.uint64(bucket)]
    assert len(hit) >= k
    return hit[:k]


def bonus_of(c, beta):
    """beta / sqrt(c) as IEEE f64, 0.0 where c is 0."""
    c = np.asarray(c, np.uint64)
    out = np.zeros(len(c), np.float64)
    nz = c != 0
    out[nz] = np.float64(beta) / np.sqrt(c[nz].astype(np.float64))
    return out


class Model:
    def __init__(self, lg=LG):
        self.limit = 3 << (lg - 2)
        self.count, self.sent, self.overflow = {}, {}, 0

    @property
    def used(self):
        return len(self.count)

    def update(self, keys, mask=None, env0=0, count=None, beta=1.0, peek=False):
        """(counts uint64, bonus f64) over the range's envs."""
        keys = [int(k) for k in np.asarray(keys).view(np.uint64)]
        count = len(keys) - env0 if count is None else count
        part = [e for e in range(env0, env0 + count) if (mask is None or mask[e]) and keys[e] != NOKEY]
        is_open = self.used + count <= self.limit
        if not peek:
            for e in part:
                k = keys[e]
                if k not in self.count:
                    if not is_open:
                        self.overflow += 1
                        continue
                    self.count[k], self.sent[k] = 0, 0
                self.count[k] += 1
        c = np.zeros(count, np.uint64)
        for e in part:
            c[e - env0] = self.count.get(keys[e], 0)
        return c, bonus_of(c, beta)

    def add(self, recs, foreign=False):
        recs = np.asarray(recs).view(np.uint64).reshape(-1, 2)
        is_open = self.used + len(recs) <= self.limit
        for k, c in recs.tolist():
            if k == NOKEY or c == 0:
                continue
            if k not in self.count:
                if not is_open:
                    self.overflow += 1
                    continue
                self.count[k], self.sent[k] = 0, 0
            self.count[k] += c
            if foreign:
                self.sent[k] += c
        return self

    def pack(self, delta=False):
        rows = []
        for k in sorted(self.count):
            v = self.count[k] - (self.sent[k] if delta else 0)
            if delta:
                self.sent[k] = self.count[k]
            if v:
                rows.append((k, v))
        return np.array(rows, np.uint64).reshape(-1, 2)


def packed(emu, delta=False):
    return emu.counts_pack(delta).cpu().numpy().view(np.uint64)


def same_table(emu, model):
    assert np.array_equal(packed(emu), model.pack()), "full pack"
    assert emu.counts_read() == {"used": model.used, "overflow": model.overflow}
    assert model.used <= model.limit


class Pair:
    """A handle and its model, driven together: every call's outputs are compared on the spot."""

    def __init__(self, emu, dev, lg=LG):
        self.emu, self.dev, self.model = emu, dev, Model(lg)
        emu.counts_create(lg)
        assert emu.counts_limit == self.model.limit
        self.log = []

    def update(self, keys, mask=None, env0=0, count=None, beta=1.0, peek=False):
        n = self.emu.n
        keys = np.asarray(keys, np.uint64)
        count = n - env0 if count is None else count
        c_out, b_out = self.dev(np.full(n, -7), np.int64), self.dev(np.full(n, -7.0), np.float64)
        m = None if mask is None else self.dev(mask, np.uint8)
        self.emu.counts_update(self.dev(keys.view(np.int64), np.int64), m, env0, count, beta, peek, c_out, b_out)
        want_c, want_b = self.model.update(keys, mask, env0, count, beta, peek)
        c, b = c_out.cpu().numpy(), b_out.cpu().numpy()
        rng = slice(env0, env0 + count)
        assert np.array_equal(c[rng].view(np.uint64), want_c), (len(self.log), "counts")
        # bit-equal: f64 sqrt and divide are correctly rounded on both sides
        assert np.array_equal(b[rng].view(np.uint64), want_b.view(np.uint64)), (len(self.log), "bonus")
        out = np.ones(n, bool)
        out[rng] = False
        assert (c[out] == -7).all() and (b[out] == -7.0).all(), "written outside the range"
        self.log.append((c.copy(), b.copy()))
        return want_c, want_b

    def add(self, recs, foreign=False):
        recs = np.ascontiguousarray(recs, np.uint64).reshape(-1, 2)
        self.emu.counts_add(self.dev(recs.view(np.int64), np.int64), foreign)
        self.model.add(recs, foreign)

    def pack(self, delta=False):
        got, want = packed(self.emu, delta), self.model.pack(delta)
        assert np.array_equal(got, want), ("delta" if delta else "full", len(got), len(want))
        self.log.append(got.copy())
        return got

    def same(self):
        same_table(self.emu, self.model)


def pool40():
    """40 keys: a probe chain of 9 from entry 1020, which wraps past entry 1023, one of 9 from entry
    500, and 22 random words, some with the top bit set."""
    rnd = np.random.default_rng(11).integers(0, 1 << 63, 22, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    keys = np.concatenate([chain_keys(1020, 9), chain_keys(500, 9), rnd])
    assert len(np.unique(keys)) == 40 and (keys >> np.uint64(63)).any() and NOKEY not in keys.tolist()
    return keys


def model_sequence(make, dev):
    """About 20 calls with heavy duplicates; returns everything the handle gave back."""
    emu = make(N)
    p = Pair(emu, dev)
    rng = np.random.default_rng(12)
    pool = pool40()
    fresh = np.arange(1, N + 1, dtype=np.uint64) * np.uint64(0xD1B54A32D192ED03)
    assert not set(fresh.tolist()) & set(pool.tolist())
    p.update(np.concatenate([pool[:18]] * 8)[:N])                        # both chains first: 18 entries on 2 starts
    for t in range(18):
        keys = pool[rng.integers(0, 40, N)]
        mask = rng.integers(0, 2, N).astype(np.uint8) if t % 3 == 1 else None
        if t == 5:
            keys = np.full(N, pool[3], np.uint64)                        # all 128 envs on one key, of the wrapping chain
        if t == 9:
            keys = fresh                                                 # 128 distinct new keys
        if t == 13:
            keys = keys.copy()
            keys[::7] = NOKEY
        p.update(keys, mask, beta=(1.0, 0.5, 0.37)[t % 3])
        if t % 6 == 5:
            p.same()
    assert p.model.used == 40 + N and p.model.overflow == 0
    assert p.model.count[int(pool[3])] > N
    p.pack()
    p.same()
    emu.close()
    return p.log


def check_model_equality(make, dev):
    model_sequence(make, dev)


def check_run_to_run(make, dev):
    a, b = model_sequence(make, dev), model_sequence(make, dev)
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, tuple):
            assert all(u.tobytes() == v.tobytes() for u, v in zip(x, y))
        else:
            assert x.tobytes() == y.tobytes()


def check_ranges(make, dev):
    emu = make(N)
    p = Pair(emu, dev)
    rng = np.random.default_rng(13)
    pool = pool40()
    for env0, count in ((0, 64), (64, 64), (64, 37), (0, N)):
        keys = pool[rng.integers(0, 40, N)]
        keys[[3, 70, 99]] = NOKEY                                        # 99 is in (64, 37), 110 is past it
        mask = np.ones(N, np.uint8)
        mask[[5, 64, 100, 110]] = 0
        before = dict(p.model.count)
        c, b = p.update(keys, mask, env0, count, beta=0.25)
        for e in (3, 5, 64, 70, 99, 100):
            if env0 <= e < env0 + count:
                assert c[e - env0] == 0 and b[e - env0] == 0.0
        counted = sum(p.model.count.values()) - sum(before.values())
        in_range = [e for e in range(env0, env0 + count) if mask[e] and keys[e] != NOKEY]
        assert counted == len(in_range)
        p.same()
    emu.close()


def new_keys(start, k):
    return (np.arange(start, start + k, dtype=np.uint64) + np.uint64(1)) * np.uint64(0xA0761D6478BD642F)


def check_full_table(make, dev):
    emu = make(N)
    p = Pair(emu, dev)
    for i in range(5):
        p.update(new_keys(i * N, N))
    p.update(new_keys(5 * N, N), env0=0, count=64)
    assert p.model.used == 704
    p.same()
    keys = new_keys(6 * N, N)                                            # 704 + 64 = 768 <= limit: open
    p.update(keys, env0=64, count=64)
    assert p.model.used == LIMIT and p.model.overflow == 0
    p.same()
    # closed: 32 new keys are turned away one by one, 32 stored ones count on
    keys = new_keys(7 * N, N)
    keys[32:64] = new_keys(0, 32)
    c, b = p.update(keys, env0=0, count=64, beta=2.0)
    assert (c[:32] == 0).all() and (b[:32] == 0.0).all() and (c[32:] == 2).all()
    assert p.model.used == LIMIT and p.model.overflow == 32
    p.same()
    keys[:] = keys[0]                                                    # one absent key, 128 envs
    p.update(keys)
    assert p.model.overflow == 32 + N
    p.update(keys, peek=True)
    p.same()
    emu.counts_clear()
    p.model = Model()
    p.same()
    c, _ = p.update(new_keys(9 * N, N))
    assert (c == 1).all() and p.model.used == N
    p.same()
    emu.close()


def check_peek(make, dev):
    emu = make(N)
    p = Pair(emu, dev)
    pool = pool40()
    rng = np.random.default_rng(14)
    for _ in range(3):
        p.update(pool[rng.integers(0, 30, N)])
    before, read = packed(emu), emu.counts_read()
    keys = pool[rng.integers(0, 40, N)]                                  # pool[30:] is not stored
    keys[9] = NOKEY
    mask = rng.integers(0, 2, N).astype(np.uint8)
    c, b = p.update(keys, mask, beta=0.5, peek=True)
    assert (c != 0).any() and (c[np.isin(keys, pool[30:])] == 0).all()
    p.update(keys, None, 64, 37, peek=True)
    assert np.array_equal(packed(emu), before) and emu.counts_read() == read
    p.same()
    assert packed(emu, delta=True).tolist() == before.tolist()           # a peek sent nothing either
    emu.close()


def check_pack_add(make, dev):
    A, B = Pair(make(N), dev), Pair(make(N), dev)
    pool = pool40()
    rng = np.random.default_rng(15)
    for _ in range(3):
        A.update(pool[rng.integers(0, 25, N)])
    full_a = A.pack()
    assert len(full_a) == A.model.used and np.array_equal(full_a, A.model.pack())
    # A's delta into the empty B and B's delta back: B sends nothing on, A stays as it is
    d_a = A.pack(delta=True)
    assert np.array_equal(d_a, full_a)
    B.add(d_a, foreign=True)
    d_b = B.pack(delta=True)
    assert len(d_b) == 0
    assert np.array_equal(A.pack(), full_a) and np.array_equal(B.pack(), full_a)
    assert len(A.pack(delta=True)) == 0                                  # nothing counted since
    # B counts keys of its own, some of them A's
    own = Model()
    for _ in range(2):
        keys = pool[rng.integers(15, 40, N)]
        B.update(keys)
        own.update(keys)
    d_b = B.pack(delta=True)
    assert np.array_equal(d_b, own.pack())                               # B's own counts only
    A.add(d_b, foreign=True)
    union = Model().add(full_a).add(own.pack())
    assert np.array_equal(A.pack(), union.pack()) and np.array_equal(B.pack(), union.pack())
    assert len(A.pack(delta=True)) == 0 and len(B.pack(delta=True)) == 0
    keys = pool[rng.integers(0, 40, N)]
    A.update(keys)
    assert np.array_equal(A.pack(delta=True), Model().add(np.stack([keys, np.ones(N, np.uint64)], 1)).pack())
    A.same()
    # a closed add: 768 records on a table that holds 40 keys; the absent ones overflow one by one
    recs = np.stack([new_keys(0, LIMIT), np.full(LIMIT, 3, np.uint64)], 1)
    recs[:20, 0] = pool[:20]
    recs[20, 0] = NOKEY
    recs[21, 1] = 0
    before = B.model.overflow
    B.add(recs)
    assert B.model.used == 40 and B.model.overflow - before == LIMIT - 22
    B.same()
    B.add(recs[:LIMIT - 40])                                             # 40 + 728 = 768: open
    assert B.model.used == 40 + LIMIT - 40 - 22 and B.model.overflow - before == LIMIT - 22
    B.same()
    A.emu.close()
    B.emu.close()


def check_guards(make, dev):
    big = make(1024)
    assert big._L.pk_counts_create(big._h, LG) < 0 and big._L.pk_last_error()     # limit 768 < 1,024 envs
    assert big.counts_limit == 0
    big.counts_create(LG + 1)
    assert big.counts_limit == 2 * LIMIT
    big.close()
    emu = make(N)
    L, h = emu._L, emu._h
    keys = dev(np.arange(N), np.int64)
    c_out, b_out = dev(np.full(N, -7), np.int64), dev(np.full(N, -7.0), np.float64)
    recs = dev(np.full((LIMIT, 2), 5), np.int64)
    n_out = dev(np.full(1, -7), np.int32)
    kp, cp, bp, rp, npp = (t.data_ptr() for t in (keys, c_out, b_out, recs, n_out))
    used, over = np.zeros(1, np.uint64), np.zeros(1, np.uint64)

    def untouched():
        assert L.pk_last_error()
        assert (c_out.cpu().numpy() == -7).all() and (b_out.cpu().numpy() == -7.0).all()
        assert (recs.cpu().numpy() == 5).all() and (n_out.cpu().numpy() == -7).all()

    def every_call_refused():
        assert L.pk_counts_update(h, kp, None, 0, N, 1.0, 0, cp, bp, None) < 0
        assert L.pk_counts_add(h, rp, 4, 0, None) < 0
        assert L.pk_counts_pack(h, 0, rp, LIMIT, npp, None) < 0
        assert L.pk_counts_read(h, used.ctypes.data_as(L.pk_counts_read.argtypes[1]), None) < 0
        assert L.pk_counts_clear(h, None) < 0
        assert L.pk_counts_limit(h) == 0
        untouched()

    every_call_refused()                                                 # no table
    for lg in (9, 31, 0):
        assert L.pk_counts_create(h, lg) < 0
        every_call_refused()
    emu.counts_create(LG)
    assert L.pk_counts_create(h, LG) < 0 and L.pk_counts_create(h, LG + 1) < 0    # a second create
    assert emu.counts_limit == LIMIT
    for args in ((kp, None, 32, 8), (kp, None, 64, 65), (kp, None, 128, 1), (kp, None, 0, 0), (None, None, 0, N)):
        for flags in (0, 1):
            assert L.pk_counts_update(h, args[0], args[1], args[2], args[3], 1.0, flags, cp, bp, None) < 0, args
            untouched()
    assert L.pk_counts_update(h, kp, None, 0, N, 1.0, 2, cp, bp, None) < 0         # an unknown flag
    assert L.pk_counts_pack(h, 0, rp, LIMIT - 1, npp, None) < 0
    assert L.pk_counts_pack(h, 0, None, LIMIT, npp, None) < 0
    assert L.pk_counts_pack(h, 0, rp + 8, LIMIT, npp, None) < 0
    assert L.pk_counts_add(h, rp, 0, 0, None) < 0
    assert L.pk_counts_add(h, rp, (1 << 30) + 1, 0, None) < 0
    assert L.pk_counts_add(h, None, 4, 0, None) < 0
    assert L.pk_counts_add(h, rp + 8, 4, 0, None) < 0
    untouched()
    assert emu.counts_read() == {"used": 0, "overflow": 0}
    # NULL outputs are legal, and the last group is a legal range
    assert L.pk_counts_update(h, kp, None, 64, 64, 1.0, 0, None, None, None) == 0
    assert emu.counts_read() == {"used": 64, "overflow": 0}
    emu.close()


class _Counter:
    """Counts the calls of an emulator's counts_* / key methods."""

    def __init__(self, emu):
        self.calls = []
        for name in ("counts_create", "counts_update", "counts_add", "counts_pack", "counts_pack_raw", "counts_read",
                     "counts_clear", "frame_keys", "cell_keys"):
            setattr(emu, name, self._wrap(name, getattr(emu, name)))

    def _wrap(self, name, fn):
        def call(*a, **k):
            self.calls.append(name)
            return fn(*a, **k)
        return call


def _bits(t):
    return t.cpu().numpy().view(np.uint64)


def check_vecenv(make_env, dev):
    """make_env(num_envs, batch_size, **kw): a VecEnv with reward=False on the benchmark ROM,
    frame_skip 4, max_episode_steps 5.  Twelve steps each of a two-batch env through step(), the same
    through recv() / send() with a flush between a send and its recv, and a one-batch env.  A twin
    emulator without the bonus is stepped with the same actions and reset by hand, so the key of the
    frame every step ends on is known for the envs that finish too: novelty_keys equals it — the key
    is taken after the step and before the auto-reset — and the rewards are the model's bonus, fed
    with those keys in the order the table was updated."""
    steps, beta = 12, 0.5
    for num, bs, pipeline in ((48, 24, False), (48, 24, True), (64, None, False)):
        env = make_env(num, bs, novelty_log2=LG, novelty_beta=beta, novelty_key="frame", novelty_frame=(16, 16, 8))
        twin = make_env(num, bs).emu
        assert env.emu.n == twin.n == (128 if bs else 64) and env.emu.counts_limit == LIMIT
        model = Model()
        rng = np.random.default_rng(16)
        seen = {"finished": 0, "moved": 0}

        def play(b, a):
            """The twin's step of sub-batch b: the keys of the frames it ends on, who finished, and the
            keys of the frames the finished envs restart from."""
            psl = env._prange(b)
            n_b = psl.stop - psl.start
            twin.step_range(psl.start, a)
            k = _bits(twin.frame_keys(16, 16, 8, env0=psl.start, count=n_b))[psl]
            done = twin.terminals[psl].cpu().numpy().astype(bool)
            r = k
            if done.any():
                twin.reset_range(psl.start, n_b, twin.terminals)
                r = _bits(twin.frame_keys(16, 16, 8, env0=psl.start, count=n_b))[psl]
            return k, done, r

        def check(b, rew, term, played, counted=None):
            """What the env returned for sub-batch b against the twin and the model; reads the env's
            buffers on the current stream, without joining the sub-batch streams."""
            k, done, r = played
            psl = env._prange(b)
            assert np.array_equal(term.cpu().numpy().astype(bool), done)
            assert np.array_equal(_bits(env._nov_keys[psl]), k), (num, pipeline, b, "keys: the frame before the auto-reset")
            c, bonus = model.update(k, beta=beta) if counted is None else counted
            assert np.array_equal(_bits(rew), bonus.view(np.uint64)), (num, pipeline, b)
            assert np.array_equal(_bits(env._nov_counts[psl]), c)
            assert np.array_equal(_bits(env._nov_bonus[psl]), bonus.view(np.uint64))
            # the frame a finished env restarts from gained no count: the table holds for its key what the model holds
            if done.any():
                probe = np.full(env.emu.n, NOKEY, np.uint64)
                probe[psl] = r
                held, _ = env.emu.counts_update(dev(probe.view(np.int64), np.int64), None, psl.start, len(k), 1.0, True)
                assert _bits(held[psl])[done].tolist() == [model.count.get(int(x), 0) for x in r[done]]
            seen["finished"] += int(done.sum())
            seen["moved"] += int((k[done] != r[done]).sum())

        twin.reset()
        if pipeline:
            env.async_reset()
            sent, early = {}, {}
            for i in range(steps * env.num_batches + env.num_batches):
                _, rew, term, _, _, _, _ = env.recv()
                b = env._current
                if b in sent:
                    check(b, rew, term, sent.pop(b), early.pop(b, None))
                else:
                    assert (rew.cpu().numpy() == 0).all()
                a = dev(rng.integers(0, 8, env.batch_size), np.uint8)
                env.send(a)
                sent[b] = play(b, a)
                if i in (9, 14):
                    # what counts_sync() does between a send and its recv: the sub-batches in flight are
                    # counted now, in batch order, and their recv() still returns the bonus
                    env._join_streams()
                    env._novelty_flush()
                    for f in sorted(sent):
                        if f not in early:
                            early[f] = model.update(sent[f][0], beta=beta)
            env._join_streams()
            env._novelty_flush()                                          # the two sends nobody received
            for f in sorted(sent):
                if f not in early:
                    model.update(sent[f][0], beta=beta)
            last = np.concatenate([sent[f][0] for f in sorted(sent)])
            total = (steps + 1) * num
        else:
            env.reset()
            for _ in range(steps):
                a = dev(rng.integers(0, 8, num), np.uint8)
                _, rew, term, _, _ = env.step(a)
                played = [play(b, a[env._range(b)]) for b in range(env.num_batches)]
                for b in range(env.num_batches):
                    sl = env._range(b)
                    check(b, rew[sl], term[sl], played[b])
            last = np.concatenate([p[0] for p in played])
            total = steps * num
        assert np.array_equal(_bits(env.novelty_keys), last)
        assert np.array_equal(_bits(env.novelty_bonus), bonus_of(_bits(env.novelty_counts), beta).view(np.uint64))
        assert seen["finished"] >= 2 * num                               # two auto-resets per env ...
        assert seen["moved"] > 0                                         # ... some from a frame that is not the restart frame
        got = packed(env.emu)
        assert np.array_equal(got, model.pack())
        assert int(got[:, 1].sum()) == total                             # one count per env and step
        assert float(env.stats.ep_return.abs().sum()) == 0.0             # the statistics keep the extrinsic return
        env.emu.close()
        twin.close()
    # off: not one counts or keys call, by step() or by the pipeline
    env = make_env(48, 24)
    tally = _Counter(env.emu)
    env.reset()
    _, rew, _, _, _ = env.step(dev(np.zeros(48), np.uint8))
    assert (rew.cpu().numpy() == 0).all()
    env.async_reset()
    for _ in range(4):
        env.recv()
        env.send(dev(np.zeros(24), np.uint8))
    env._join_streams()
    assert tally.calls == [] and env.emu.counts_limit == 0
    with pytest.raises(RuntimeError):
        env.novelty_keys
    with pytest.raises(RuntimeError):
        env.counts_sync()
    env.emu.close()
    for bad in ({"novelty_key": "screen"}, {"novelty_frame": (12, 16, 8)}, {"novelty_frame": (16, 32, 8)},
                {"novelty_frame": (16, 16, 1)}, {"novelty_frame": (16, 16, 257)}, {"novelty_frame": (16, 16)},
                {"novelty_frame": None}):
        for lg in (0, LG):
            with pytest.raises(ValueError):
                make_env(64, None, novelty_log2=lg, **bad)


def check_vecenv_ram_keys(make_env, dev):
    """novelty_key "ram" and "frame+ram" take pk_cell_keys and the salted frame key."""
    import cells_common as cc
    for name in ("ram", "frame+ram"):
        env = make_env(48, 24, novelty_log2=LG, novelty_key=name, novelty_frame=(16, 24, 5))
        env.reset()
        rng = np.random.default_rng(17)
        env.emu.set_ram(0xD361, dev(rng.integers(0, 3, (env.emu.n, 2)), np.uint8))
        _, rew, term, _, _ = env.step(dev(rng.integers(0, 8, 48), np.uint8))
        assert not term.any()
        ram = cc.ram_keys(env)
        order = [env.phys(e) for e in range(48)]
        want = ram if name == "ram" else cc.model(env.emu.screen.cpu().numpy()[order], 16, 24, 5, ram)[0]
        assert np.array_equal(_bits(env.novelty_keys), want), name
        model = Model()
        bonus = np.concatenate([model.update(want[env._range(b)])[1] for b in range(2)])
        assert np.array_equal(_bits(rew), bonus.view(np.uint64)), name
        env.emu.close()


EXPORTS = ("pk_counts_create", "pk_counts_limit", "pk_counts_update", "pk_counts_add", "pk_counts_pack",
           "pk_counts_read", "pk_counts_clear")
