"""Shared scenarios of the archive-exchange tests (pk_archive_pack / pk_archive_merge, ABI v11):
test_hostsim_exchange.py runs them on the host-simulation build, test_gpu_exchange.py on the gfx950
build, two handles in one process.  The oracle is the sequential model of include/pokegym_amd.h,
stated once here (XModel, an extension of archive_common.Model); slot contents are compared with the
source handle's slots, continuations with the source handle's own."""
import math

import numpy as np
import torch

import archive_common as ac
import episodes_common as ec
from pokegym_amd.emulator import BatchedEmulator

N = ac.N
NOKEY = ac.NOKEY
M32 = (1 << 32) - 1
XREC = BatchedEmulator.XREC


class XModel(ac.Model):
    """archive_common.Model with the exchange words: sent counts and dirty per cell, pack and merge."""

    def __init__(self, n_cells, slot0, seed):
        super().__init__(n_cells, slot0, seed)
        self.sent_visits, self.sent_picks, self.dirty = [], [], []

    def _grow(self):
        while len(self.dirty) < self.used:
            self.sent_visits.append(0)
            self.sent_picks.append(0)
            self.dirty.append(0)

    def update(self, *a, **kw):
        out, winner = super().update(*a, **kw)
        self._grow()
        for c in winner:
            self.dirty[c] = 1
        return out, winner

    def pack(self, fmt, delta=False, cell0=0, count=None, max_payloads=None):
        """Returns (records, the cells whose payloads are shipped, in payload order)."""
        count = self.n_cells - cell0 if count is None else count
        max_payloads = count if max_payloads is None else max_payloads
        recs = np.zeros(count, XREC)
        recs["key"], recs["payload"] = NOKEY, -1
        cells = []
        for i in range(count):
            c = cell0 + i
            if c >= self.used:
                continue
            r = recs[i]
            r["key"], r["score"], r["length"], r["format"] = self.key[c], self.record[c][0], self.record[c][1], fmt
            r["visits"], r["picks"], want = self.visits[c], self.picks[c], True
            if delta:
                r["visits"] = (self.visits[c] - self.sent_visits[c]) & M32
                r["picks"] = (self.picks[c] - self.sent_picks[c]) & M32
                self.sent_visits[c], self.sent_picks[c] = self.visits[c], self.picks[c]
                want = bool(self.dirty[c])
            if want and len(cells) < max_payloads:
                r["payload"] = len(cells)
                cells.append(c)
                if delta:
                    self.dirty[c] = 0
        return recs, cells

    def merge(self, recs, n_payloads, fmt):
        """Walks the records in ascending order.  Returns (cell_out, {cell: winning record}, rejects)."""
        out = np.full(len(recs), -1, np.int32)
        winner, rejects = {}, 0
        for i, r in enumerate(recs):
            k, s, p, length = int(r["key"]), float(r["score"]), int(r["payload"]), int(r["length"])
            if k == NOKEY:
                continue
            if int(r["format"]) != fmt or p >= n_payloads or math.isnan(s):
                rejects += 1
                continue
            c = self.index.get(k)
            if c is None:
                if p < 0 or self.used == self.n_cells:
                    self.overflow += 1
                    continue
                c = self.used
                self.index[k] = c
                self.key.append(k)
                self.record.append(None)
                self.visits.append(0)
                self.picks.append(0)
                self._grow()
            self.visits[c] = (self.visits[c] + int(r["visits"])) & M32
            self.picks[c] = (self.picks[c] + int(r["picks"])) & M32
            self.sent_visits[c] = (self.sent_visits[c] + int(r["visits"])) & M32
            self.sent_picks[c] = (self.sent_picks[c] + int(r["picks"])) & M32
            rec = self.record[c]
            if p >= 0 and (rec is None or s > rec[0] or (s == rec[0] and length < rec[1])):
                self.record[c] = (s, length)
                winner[c] = i
        for c, i in winner.items():
            out[i] = c
        return out, winner, rejects

    def table(self):
        return {k: (self.record[c], self.visits[c], self.picks[c]) for k, c in self.index.items()}


class Run(ac.Run):
    """archive_common.Run with trajectories, the exchange words and the extended model."""

    def __init__(self, make, dev, n_cells, traj=True, exchange=True, **kw):
        super().__init__(make, dev, n_cells, **kw)
        self.model = XModel(n_cells, self.slot0, self.model.seed)
        if traj:
            self.emu.traj_enable()
        if exchange:
            self.emu.archive_exchange_enable()
            assert self.emu.archive_payload_bytes > 0 and self.emu.archive_payload_bytes % 16 == 0
        self.fmt = self.emu.archive_format

    def sparse_update(self, entries):
        """entries {env: (key, score)}: an update in which only those envs take part."""
        keys, scores, mask = [NOKEY] * N, np.zeros(N), np.zeros(N, np.uint8)
        for e, (k, s) in entries.items():
            keys[e], scores[e], mask[e] = k, s, 1
        return self.update(keys, scores, mask)

    def explore(self, envs):
        self.emu.archive_explore(ec.masked(envs, self.dev, N), out=self.out)
        want, rejects = self.model.explore(N, envs)
        assert self.out.cpu().numpy().tolist() == want.tolist() and rejects == 0

    def pack(self, **kw):
        """One pk_archive_pack checked against the model.  Returns host records, device payloads."""
        rec, pay, n = self.emu.archive_pack(**kw)
        want, cells = self.model.pack(self.fmt, **kw)
        got = rec.cpu().numpy().view(XREC).reshape(-1)
        assert got.tobytes() == want.tobytes(), [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:3]
        assert int(n) == len(cells)
        return got, pay[:len(cells)], cells

    def merge(self, recs, pay, source=None):
        """One pk_archive_merge checked against the model in archive_read, cell_out, rejects and
        overflow; with source = (run, cell of every payload row) each winner's slot equals the
        source's slot.  Returns (cell_out, winner)."""
        out = self.dev(np.full(len(recs), -7), np.int32)
        self.emu.archive_merge(self.dev(np.ascontiguousarray(recs).view(np.uint8).reshape(len(recs), -1), np.uint8), pay, out=out)
        want, winner, rejects = self.model.merge(recs, 0 if pay is None else len(pay), self.fmt)
        assert out.cpu().numpy().tolist() == want.tolist()
        self.model.check(self.emu)
        assert self.emu.bank_rejects() == rejects
        if source is not None:
            src, cells = source
            for c, i in winner.items():
                same_slot(self, c, src, cells[int(recs[i]["payload"])])
        return want, winner

    def slot(self, c):
        return slot_bytes(self.emu, self.slot0 + c)


def slot_bytes(emu, slot):
    """Everything that can be read of a slot: its v9 export and its trajectory part."""
    t = emu.bank_trajectories(slot, 1)
    return (emu.bank_get(slot),) + tuple(t[k].cpu().numpy().tobytes() for k in ("origin", "length", "flags", "actions"))


def same_slot(a, ca, b, cb):
    assert a.slot(ca) == b.slot(cb), (ca, cb)


def table(emu):
    got = emu.archive_read()
    u = got["used"]
    return {int(k): (float(s), int(ln), int(v), int(p)) for k, s, ln, v, p in
            zip(got["keys"][:u], got["scores"][:u], got["lengths"][:u], got["visits"][:u], got["picks"][:u])}


def read_equal(a, b, what=""):
    for k in ("used", "keys", "scores", "lengths", "visits", "picks"):
        assert np.array_equal(a[k], b[k]), (what, k)


# -- 1. clone -------------------------------------------------------------------------------------
def check_clone(make, dev, set_ilv):
    set_ilv("32")
    a = Run(make, dev, n_cells=40)
    a.prologue()
    keys, scores, mask = ac.parity_inputs()
    a.update(keys, scores, mask)
    a.step()
    a.update(keys, scores + np.random.default_rng(6).integers(-1, 2, N), None)
    a.explore([3, 17, 64, 90])
    before = a.emu.archive_read()
    recs, pay, cells = a.pack()
    read_equal(before, a.emu.archive_read(), "a full pack leaves the archive as it is")
    assert before["overflow"] == a.emu.archive_read()["overflow"] and cells == list(range(a.model.used))
    set_ilv("16")                                          # slots are dense: the image interleave does not matter
    b = Run(make, dev, n_cells=40, script_seed=17)
    b.reset()
    out, winner = b.merge(recs, pay, (a, cells))
    used = a.model.used
    assert out[:used].tolist() == list(range(used)) and (out[used:] == -1).all()
    read_equal(a.emu.archive_read(), b.emu.archive_read(), "clone")
    for c in range(used):
        same_slot(b, c, a, c)
    ta, tb = a.emu.bank_trajectories(a.slot0, used), b.emu.bank_trajectories(b.slot0, used)
    for k in ta:
        assert torch.equal(ta[k].cpu(), tb[k].cpu()), k
    # envs resumed from the same cells on both handles, fed the same inputs, return the same
    envs, cell = [3, 70, 127], [0, 5, used - 1]
    resume = dev(ec.slot_map({e: a.slot0 + c for e, c in zip(envs, cell)}, N))
    sc = ec.Script(6, N, 23, dev)
    for r in (a, b):
        r.emu.bank_resume(resume)
        assert r.emu.bank_rejects() == 0
    ra, rb = ec.outputs(a.emu, envs), ec.outputs(b.emu, envs)
    for k in ("obs", "snap", "errors"):                    # straight after the resume, before any step
        assert ra[k].tobytes() == rb[k].tobytes(), k
    for t in range(6):
        sc.step(a.emu, t)
        sc.step(b.emu, t)
        ec.same(ec.outputs(a.emu, envs), ec.outputs(b.emu, envs), ("continuation", t))
    a.close()
    b.close()


# -- 2. merge model ---------------------------------------------------------------------------------
def scenario(make, dev):
    """Two handles with different scripts over overlapping keys.  Step counters after the prologue
    (archive_common.Run.prologue): 4, except envs 1, 5, 40, 64, 77 (2) and 33, 65, 100 (1)."""
    a = Run(make, dev, n_cells=40, script_seed=3)
    b = Run(make, dev, n_cells=40, script_seed=29, seed=11)
    for r in (a, b):
        r.prologue()
    a.sparse_update({0: (100, 5.0), 2: (101, 1.0),         # keys only in A
                     3: (105, 9.0), 7: (105, 2.0), 8: (105, 2.0), 66: (105, 1.0),   # A's record is better
                     4: (106, 2.0),                        # B's is better
                     1: (107, 4.0),                        # equal scores, A's episode is shorter (2 < 4)
                     6: (108, 6.0),                        # a full tie across the handles
                     70: (100, 1.0), 10: (109, -0.0)})
    b.sparse_update({0: (105, 3.0), 2: (106, 7.0), 3: (107, 4.0), 4: (108, 6.0), 9: (109, 0.0), 12: (109, -1.0),
                     6: (110, 1.0), 64: (111, 2.0), 20: (105, 3.0)})     # 110, 111: keys only in B
    a.explore([5, 9, 64])
    b.explore([2, 3])
    return a, b


def merge_inputs(a, dev):
    """A's archive packed twice — all cells, then the first six with three payloads — and joined
    into one record array, so every key of the second pack is a duplicate; then the reserved key, a
    foreign format, a payload row past the array, a NaN score and a record without a payload."""
    r1, p1, c1 = a.pack(count=a.model.used + 2)            # two cells past the ones in use: key UINT64_MAX
    r2, p2, c2 = a.pack(count=6, max_payloads=3)
    r2 = r2.copy()
    r2["payload"][r2["payload"] >= 0] += len(c1)
    extra = np.zeros(5, XREC)
    extra[:] = r1[0]
    extra["format"][0] ^= 1 << 16                          # another seen-set capacity
    extra["payload"][1] = len(c1) + len(c2)                # a row past the payload array
    extra["score"][2] = np.nan
    extra["payload"][3], extra["visits"][3] = -1, 5        # counts only
    extra["key"][4] = NOKEY
    recs = np.concatenate([r1, r2, extra])
    return recs, torch.cat([p1, p2]), c1 + c2


def check_merge_model(make, dev):
    """Returns what the determinism scenario compares."""
    a, b = scenario(make, dev)
    recs, pay, cells = merge_inputs(a, dev)
    own = {k: b.slot(c) for k, c in b.model.index.items()}
    out, winner = b.merge(recs, pay, (a, cells))
    idx = b.model.index
    assert b.emu.archive_read()["overflow"] == 0
    won = {b.model.key[c] for c in winner}
    assert won == {100, 101, 105, 107}                     # new keys, the better record, the shorter episode
    assert all(i < a.model.used for i in winner.values())  # ties inside the call go to the lower record
    for k in (106, 108, 109, 110, 111):                    # B's better record, the full tie, -0.0 == 0.0, B's own keys
        assert b.slot(idx[k]) == own[k], k
    got = b.emu.archive_read()
    slots = [b.slot(c) for c in range(got["used"])]
    a.close()
    b.close()
    return got, out.tolist(), slots


def check_determinism(make, dev):
    a, oa, sa = check_merge_model(make, dev)
    b, ob, sb = check_merge_model(make, dev)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True) if isinstance(a[k], np.ndarray) else a[k] == b[k], k
    assert oa == ob and sa == sb


# -- 3. capacity ------------------------------------------------------------------------------------
def check_capacity(make, dev):
    a, b = scenario(make, dev)
    b.close()
    small = Run(make, dev, n_cells=5, script_seed=31)
    small.prologue()
    small.sparse_update({0: (100, 50.0), 1: (900, 1.0), 2: (901, 1.0)})
    assert small.model.used == 3
    recs, pay, cells = a.pack(count=a.model.used)
    assert recs["key"][:4].tolist() == [100, 107, 101, 105]
    bare = recs[2:4].copy()                                # keys 101 and 105 without their payloads
    bare["payload"], bare["visits"] = -1, 3
    recs = np.concatenate([bare[:1], recs, bare])
    # walk: 101 without a payload finds no cell (overflow); 100 is known; 107 and 101 take the two
    # free cells in record order; the other new keys overflow; then 101, now known, counts its
    # visits, and 105, unknown and without a payload, overflows
    out, winner = small.merge(recs, pay, (a, cells))
    m = small.model
    assert m.used == 5 and m.key[3:] == [107, 101] and sorted(winner) == [3, 4]
    assert m.overflow == 1 + (a.model.used - 3) + 1
    assert m.visits[4] == a.model.visits[a.model.index[101]] + 3
    unknown = bare[:1].copy()
    unknown["key"] = 4242                                  # full archive, no payload: overflow either way
    small.merge(unknown, None)
    assert m.overflow == 3 + (a.model.used - 3)
    a.close()
    small.close()


# -- 4. delta ---------------------------------------------------------------------------------------
def check_delta(make, dev):
    a, b = scenario(make, dev)
    # deltas taken before either merge, then exchanged: both sides hold the same table
    ra, pa, ca = a.pack(delta=True)
    rb, pb, cb = b.pack(delta=True)
    assert ca == list(range(a.model.used)) and cb == list(range(b.model.used))
    a.merge(rb, pb, (b, cb))
    b.merge(ra, pa, (a, ca))
    assert table(a.emu) == table(b.emu) and len(table(a.emu)) == 9
    # nothing happened since: all-zero counts, no payloads; what B sent is never sent on
    r, p, c = a.pack(delta=True)
    assert not c and not r["visits"].any() and not r["picks"].any() and (r["payload"] == -1).all()
    # one more update with three winners: exactly those payloads, and the new visits
    a.step()
    w = a.sparse_update({0: (100, 9.0), 3: (106, 9.0), 4: (111, 9.0), 7: (105, 0.0)})
    assert len(w) == 3
    r, p, c = a.pack(delta=True, max_payloads=1)
    assert c == [min(w)] and int(r["visits"].sum()) == 4
    r, p, c2 = a.pack(delta=True, max_payloads=1)
    r, p, c3 = a.pack(delta=True, max_payloads=1)
    assert c + c2 + c3 == sorted(w) and not r["visits"].any()
    r, p, c = a.pack(delta=True, max_payloads=1)
    assert not c
    # a ranged delta pack only touches its cells
    a.explore([1, 2, 3, 4, 5, 6])
    r, p, c = a.pack(delta=True, cell0=2, count=3)
    r2, p, c = a.pack(delta=True)
    assert int(r["picks"].sum()) + int(r2["picks"].sum()) == 6 and not r2["picks"][2:5].any()
    a.close()
    b.close()


# -- 6. guards --------------------------------------------------------------------------------------
def check_guards(make, dev):
    rec = dev(np.zeros((4, 48)), np.uint8)
    pay = dev(np.zeros((4, 16)), np.uint8)
    n, out = dev(np.zeros(1), np.int32), dev(np.zeros(4), np.int32)

    def refused(emu, enable=True):
        L, h = emu._L, emu._h
        if enable:
            assert L.pk_archive_exchange_enable(h) < 0 and L.pk_last_error()
        assert L.pk_archive_pack(h, 0, 0, 4, 4, rec.data_ptr(), pay.data_ptr(), n.data_ptr(), None) < 0 and L.pk_last_error()
        assert L.pk_archive_merge(h, rec.data_ptr(), 4, pay.data_ptr(), 4, out.data_ptr(), None) < 0 and L.pk_last_error()

    bare = make(N, reward=True, max_episode_steps=ac.MAX_STEPS)   # no archive
    refused(bare)
    assert bare.archive_payload_bytes == 0
    bare.close()
    run = Run(make, dev, n_cells=6, exchange=False)
    twin = Run(make, dev, n_cells=6, exchange=False)
    for r in (run, twin):
        r.prologue()
        r.sparse_update({0: (1, 1.0), 1: (2, 2.0), 64: (3, 3.0)})
    refused(run.emu, enable=False)                                # not enabled
    assert run.emu.archive_payload_bytes == 0
    run.emu.archive_exchange_enable()
    pb = run.emu.archive_payload_bytes
    fmt = run.emu.archive_format
    assert fmt >> 24 == 1 and fmt & (1 << 23) and (fmt >> 16) & 0x7F == 10 and pb > 74512 + 272 + 4096 + 8192 + 256
    L, h = run.emu._L, run.emu._h
    assert L.pk_archive_exchange_enable(h) < 0 and L.pk_last_error()   # twice
    held = [run.slot(c) for c in range(3)]
    pay = dev(np.zeros((4, pb)), np.uint8)
    for args in ((0, 3, 4, 4), (0, 0, 0, 4), (0, 6, 1, 1), (2, 0, 4, 4)):       # ranges past the cells, no cell, unknown flags
        assert L.pk_archive_pack(h, *args, rec.data_ptr(), pay.data_ptr(), n.data_ptr(), None) < 0
    assert L.pk_archive_pack(h, 0, 0, 4, 4, None, pay.data_ptr(), n.data_ptr(), None) < 0
    assert L.pk_archive_pack(h, 0, 0, 4, 4, rec.data_ptr(), None, n.data_ptr(), None) < 0
    assert L.pk_archive_pack(h, 1, 0, 4, 4, rec.data_ptr() + 8, pay.data_ptr(), n.data_ptr(), None) < 0
    assert L.pk_archive_merge(h, None, 4, pay.data_ptr(), 4, None, None) < 0
    assert L.pk_archive_merge(h, rec.data_ptr(), 0, pay.data_ptr(), 4, None, None) < 0
    assert L.pk_archive_merge(h, rec.data_ptr(), 65537, pay.data_ptr(), 4, None, None) < 0
    assert L.pk_archive_merge(h, rec.data_ptr(), 4, None, 4, None, None) < 0
    run.model.check(run.emu)
    assert [run.slot(c) for c in range(3)] == held and run.emu.bank_rejects() == 0
    run.model.dirty = [0] * run.model.used                        # dirty starts clear: only later winners are shipped
    r, p, c = run.pack(delta=True, max_payloads=0)                # counts only, no payload array
    assert (r["payload"] == -1).all() and r["visits"][:3].tolist() == [1, 1, 1]
    # the twin never enables the exchange: both handles go on alike
    for t in range(2):
        for r in (run, twin):
            r.step()
            r.sparse_update({0: (1, 5.0 + t), 2: (9, 1.0)})
        ec.same(ec.outputs(run.emu, range(N)), ec.outputs(twin.emu, range(N)), ("the handle steps as before", t))
    read_equal(run.emu.archive_read(), twin.emu.archive_read())
    r, p, c = run.pack(delta=True)
    assert c == [0, 3]                                            # the cells whose record changed since the enable
    assert [run.slot(c) for c in range(4)] == [twin.slot(c) for c in range(4)]
    run.close()
    twin.close()


# -- 7. VecEnv --------------------------------------------------------------------------------------
def check_vecenv(env, other, dev):
    """Two VecEnv(48, batch_size=24, archive_cells=8, archive_exchange=True) in padded slots: the
    exporter's archive, imported by the other, brings the winners' episode return / length to the
    envs that explore there."""
    n = env.num_envs
    rng = np.random.default_rng(9)

    def step(v):
        pos = rng.integers(0, 3, (v.emu.n, 2))
        v.emu.set_ram(0xD361, dev(pos, np.uint8))
        return v.step(dev(rng.integers(0, 8, n), np.uint8))

    for v in (env, other):
        v.reset()
    for _ in range(3):
        step(env)
    step(other)
    ret, length = env.stats.ep_return.clone(), env.stats.ep_length.clone()
    won = env.archive_update().cpu().numpy()
    d = env.archive_export()
    st = env.archive_state()
    used = st["used"]
    assert d["records"].shape == (8, 48) and d["payloads"].shape == (used, env.emu.archive_payload_bytes)
    assert set(d) == {"records", "payloads", "ck_return", "ck_length", "ck_valid", "ck_slots"}
    cells = other.archive_import(d).cpu().numpy()
    assert cells[:used].tolist() == list(range(used)) and (cells[used:] == -1).all()
    read_equal(st, other.archive_state(), "import")
    masked = [2, 30, 47]
    m = np.zeros(n, np.uint8)
    m[masked] = 1
    drawn = other.archive_explore(dev(m, np.uint8)).cpu().numpy()
    assert other.emu.bank_rejects() == 0
    for e in masked:
        w = int(np.flatnonzero(won == drawn[e] - other._arch0 + env._arch0)[0])
        assert other.stats.ep_return[e] == ret[w] and other.stats.ep_length[e] == length[w] == 3.0, e
        assert other.save_state(e) == env.emu.bank_get(int(drawn[e]) - other._arch0 + env._arch0), e
    step(other)
    st = other.archive_state()
    other.archive_sync()                                          # world size 1: nothing happens
    read_equal(st, other.archive_state(), "sync alone")
