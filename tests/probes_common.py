"""Shared scenarios of the RAM-probe tests (pk_probe_*): test_hostsim_probes.py runs them on the
host-simulation build, test_gpu_probes.py on the gfx950 build.  The oracle is the model of
include/pokegym_amd.h as pokegym_amd/probes.py states it in numpy (probes.model).  make(n, **kw)
builds an emulator, dev(values, dtype) a tensor on its device."""
import ctypes
import functools
from fractions import Fraction

import numpy as np
import pytest

from pokegym_amd import _native
from pokegym_amd import probes as P

REBASE_ONLY, SET = 1, 2
WRAM, HRAM = 0xC000, 0xFF80
# every kind, reduce, op and cmp at least once: len 3, BITS over 512 bytes and over 1, 64 elements with a
# stride that is not their length, an element that ends at 0xDFFF, one in the echo range, one in HRAM
FULL = [
    P.Probe(0xC010, 3, kind="le", op="delta", weight=0.5, done=("ge", 0xC00000)),
    P.Probe(0xDFFD, 3, kind="be", op="newmax", weight=0.25),
    P.Probe(0xE100, 2, kind="bcd", op="change", weight=1.5),
    P.Probe(0xFF90, 1, kind="bits", done=("eq", 1)),
    P.Probe(0xC800, 512, kind="bits", op="delta", weight=-0.125, done=("le", 2030)),
    P.Probe(0xD000, 2, 64, 5, kind="le", reduce="sum", op="newmax", weight=1e-3),
    P.Probe(0xD200, 1, 64, 3, kind="le", reduce="max", op="change", weight=-2.0, done=("ne", 255)),
    P.Probe(0xC020, 3, 4, 7, kind="bcd", reduce="max", op="delta", weight=1.0 / 3.0),
    P.Probe(0xFFF0, 2, 5, 3, kind="be", reduce="sum"),
    P.Probe(0xFD00, 16, 8, 32, kind="bits", reduce="max", op="newmax", weight=3.0),
]


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def random_ram(n, seed):
    """(wram uint8 (n, 0x2000), hram uint8 (n, 0x7F)): every byte value, so nibbles above 9, and runs of
    0xFF over the 64-element array of FULL in half of the envs and over the bit counts in a few."""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 256, (n, 0x2000), dtype=np.uint8)
    h = rng.integers(0, 256, (n, 0x7F), dtype=np.uint8)
    ff = rng.integers(0, 2, n).astype(bool)
    w[ff, 0x1200:0x1200 + 16] = 0xFF
    w[::7, 0x0800:0x0A00] = 0xFF
    w[1::7, 0x0800:0x0A00] = 0x00
    h[::5, 0x10] = 0xFF
    return w, h


def put_ram(emu, dev, seed):
    w, h = random_ram(emu.n, seed)
    emu.set_ram(WRAM, dev(w, np.uint8))
    emu.set_ram(HRAM, dev(h, np.uint8))


def reader(emu):
    return lambda addr, length: emu.get_ram(addr, length).cpu().numpy()


class Twin:
    """An emulator with a program, its three output tensors, and the model's copy of state and outputs:
    eval() runs one call on both and compares every element of every array, so whatever a call writes
    outside its range or its participants shows."""

    def __init__(self, emu, program, dev, seed=5):
        import torch
        self.emu, self.program, self.dev, self.n, self.m = emu, list(program), dev, emu.n, len(program)
        emu.probes_create(program)
        assert emu.probe_count == self.m
        rng = np.random.default_rng(seed)
        self.state = np.zeros((self.n, self.m), np.uint32)
        self.rew = rng.standard_normal(self.n)
        self.term = (rng.integers(0, 4, self.n) == 0).astype(np.uint8) * 0x40      # a bit the OR must keep
        self.feat = rng.integers(-99, 0, (self.n, self.m)).astype(np.int32)
        # copies: on the host-simulation build dev() wraps the array's own memory
        self.rew_t, self.term_t, self.feat_t = (dev(self.rew.copy(), np.float64), dev(self.term.copy(), np.uint8),
                                                dev(self.feat.copy(), np.int32))
        self.torch = torch

    def eval(self, mask=None, rebase_only=False, set=False, env0=0, count=None, rew=True, term=True, feat=True,
             call=None, what=None):
        count = self.n - env0 if count is None else count
        md = None if mask is None else self.dev(mask, np.uint8)
        kw = dict(rebase_only=rebase_only, set=set, rewards=self.rew_t if rew else None,
                  terminals=self.term_t if term else None, features=self.feat_t if feat else None)
        if call is None:
            self.emu.probes_eval(md, env0=env0, count=count, **kw)
        else:
            call(md, kw)
        st = self.state.copy()
        r, done, v, ev, took = P.model(self.program, reader(self.emu), st, mask, rebase_only)
        inr = np.zeros(self.n, bool)
        inr[env0:env0 + count] = True
        self.state[inr] = st[inr]
        ev, took = ev & inr, took & inr
        if rew:
            self.rew[ev] = r[ev] if set else self.rew[ev] + r[ev]
        if term:
            self.term[ev] = done[ev] if set else self.term[ev] | done[ev]
        if feat:
            self.feat[took] = v[took]
        self.same(what)
        return r, done, v, ev

    def same(self, what=None):
        assert np.array_equal(bits64(self.rew_t.cpu().numpy()), bits64(self.rew)), what
        assert np.array_equal(self.term_t.cpu().numpy(), self.term), what
        assert np.array_equal(self.feat_t.cpu().numpy(), self.feat), what


def check_model(make, dev, n=130):
    """FULL on random RAM: three evaluations with fresh random RAM in between, the second with a random
    rebase mask; rewards, terminals and features are bit-equal to the model after each."""
    emu = make(n)
    put_ram(emu, dev, 10)
    tw = Twin(emu, FULL, dev)
    seen_done = set()
    for t in range(3):
        put_ram(emu, dev, 11 + t)
        mask = None
        if t == 1:
            rng = np.random.default_rng(3)
            mask = rng.integers(0, 2, n).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)
        r, done, v, ev = tw.eval(mask, what=t)
        seen_done |= set(done[ev].tolist())
        assert len(np.unique(r[ev])) > n // 4 and (v[:, 4] == 4096).any() and (v[:, 4] == 0).any()
        assert (v[:, 6] == 255).any() and (v[:, 6] < 255).any()
        assert (v >= 0).all() and v.max() < 1 << 30
    assert seen_done == {False, True}
    emu.close()


# the probes' weights in program order: 0.1, -2.5e-3, 1/3 and 1e17.  A contraction can only show where
# a product is added to a sum that is not 0 and not much larger than the product, so 0.1 comes a second
# time behind the others, and 1e17 twice with nearly opposite differences: behind the first the sum is
# of the product's size.
ROUND_WEIGHTS = (0.1, -2.5e-3, 1.0 / 3.0, 0.1, 1e17, 1e17)


@functools.lru_cache(maxsize=None)
def rounding_inputs(n):
    """(before, after): per env six 24-bit values each; probe j's difference is after - before.  The
    last probe's difference is minus the fifth's but for a few hundred."""
    rng = np.random.default_rng(21)
    after = rng.integers(1 << 20, 1 << 23, (n, 6))
    after[:, 0] >>= 12                                                   # a small first sum: -2.5e-3's product is of its size
    before = np.zeros((n, 6), np.int64)
    before[:, 5] = after[:, 4] + rng.integers(1, 500, n) * rng.choice([-1, 1], n)
    after[:, 5] = 0
    return before, after


def check_rounding_is_decidable(n=64):
    """With numpy and exact fractions alone: behind every weight there is an env whose sum, rounded once
    from the exact product as a fused multiply-add rounds it, differs from the sum of the rounded
    product — the inputs of check_rounding tell the two evaluations apart."""
    before, after = rounding_inputs(n)
    d = after - before
    assert (np.abs(d) < 1 << 24).all() and (d[:, 5] < 0).all()
    differ = np.zeros(6, int)
    for e in range(n):
        r = np.float64(0.0)
        for j, w in enumerate(ROUND_WEIGHTS):
            unfused = r + np.float64(w) * np.float64(int(d[e, j]))
            fused = float(Fraction(float(r)) + Fraction(float(w)) * int(d[e, j]))
            differ[j] += float(unfused) != fused
            r = unfused
    assert differ[0] == 0 and (differ[[1, 2, 3, 5]] > 0).all(), differ      # each of the four weights decides


def check_rounding(make, dev, n=64):
    """DELTA probes with weights 0.1, 1/3, -2.5e-3 and 1e17 over differences whose products are not
    representable: the reward and its sum into a non-zero reward array are bit-equal to the model."""
    before, after = rounding_inputs(n)
    emu = make(n)

    def put(vals):
        ram = np.zeros((n, 24), np.uint8)
        for j in range(6):
            for b in range(3):
                ram[:, 4 * j + b] = (vals[:, j] >> (8 * b)) & 0xFF
        emu.set_ram(0xC100, dev(ram, np.uint8))

    put(before)
    tw = Twin(emu, [P.Probe(0xC100 + 4 * j, 3, op="delta", weight=w) for j, w in enumerate(ROUND_WEIGHTS)], dev)
    tw.eval(rebase_only=True)
    put(after)
    start = tw.rew.copy()
    r, _, v, _ = tw.eval()
    assert np.array_equal(v, after)
    want = np.zeros(n)
    for j, w in enumerate(ROUND_WEIGHTS):
        want = want + np.float64(w) * (after[:, j] - before[:, j]).astype(np.float64)
    assert np.array_equal(bits64(r), bits64(want)) and np.array_equal(bits64(tw.rew), bits64(start + want))
    emu.close()


def check_state(make, dev, n=64):
    """NEWMAX pays only for new maxima across ups and downs, DELTA goes negative, CHANGE fires once; a
    rebase by mask and by REBASE_ONLY gives reward 0 afterwards and leaves rew and term alone; SET
    contrasts with add and OR; a NONE probe shows in the features only."""
    emu = make(n)
    prog = [P.u8(0xC000, op="newmax", weight=2.0), P.u8(0xC001, op="delta", weight=0.5),
            P.u8(0xC002, op="change", weight=7.0), P.u8(0xC003, weight=5.0, done=("ge", 200))]
    ram = np.zeros((n, 4), np.uint8)

    def put(a, b, c, d):
        ram[:] = (a, b, c, d)
        ram[:, 0] += (np.arange(n) % 3).astype(np.uint8)                 # not the same in every env
        emu.set_ram(0xC000, dev(ram, np.uint8))

    put(0, 0, 0, 0)
    tw = Twin(emu, prog, dev)
    tw.eval(rebase_only=True)                                            # from the values, not from zero
    pays = []
    for a, b, c, d in ((5, 9, 1, 10), (3, 4, 1, 20), (9, 4, 1, 250), (9, 6, 1, 30), (2, 0, 1, 40), (12, 0, 2, 50)):
        put(a, b, c, d)
        r, done, v, _ = tw.eval(what=(a, b, c, d))
        pays.append(r[0])
        assert (done == (d >= 200)).all() and (v[:, 3] == d).all()
    #        newmax       delta       change
    assert pays == [2.0 * 5 + 0.5 * 9 + 7.0, 0.5 * -5, 2.0 * 4, 0.5 * 2, 0.5 * -6, 2.0 * 3 + 7.0]
    # a NONE probe alone moves nothing: the same RAM but for its byte
    put(12, 0, 2, 77)
    r, _, v, _ = tw.eval()
    assert (r == 0).all() and (v[:, 3] == 77).all()
    # rebase by mask: the masked envs' outputs stay, and their next evaluation pays nothing
    mask = np.zeros(n, np.uint8)
    mask[[0, 5, 63]] = (1, 0x80, 0xFF)
    put(40, 30, 9, 0)
    before = tw.rew.copy(), tw.term.copy()
    r, _, _, ev = tw.eval(mask)
    assert not ev[[0, 5, 63]].any() and ev.sum() == n - 3 and (r[ev] != 0).all()
    assert np.array_equal(bits64(tw.rew[~ev]), bits64(before[0][~ev])) and np.array_equal(tw.term[~ev], before[1][~ev])
    r, _, _, _ = tw.eval(what="after the rebase by mask")
    assert (r == 0).all()
    # REBASE_ONLY: only the masked envs move, nothing is paid, the others still owe their difference
    put(50, 10, 3, 0)
    before = tw.rew.copy(), tw.term.copy(), tw.feat.copy()
    tw.eval(mask, rebase_only=True)
    assert np.array_equal(bits64(tw.rew), bits64(before[0])) and np.array_equal(tw.term, before[1])
    assert np.array_equal(tw.feat[mask == 0], before[2][mask == 0]) and not np.array_equal(tw.feat[mask != 0], before[2][mask != 0])
    r, _, _, _ = tw.eval(what="after REBASE_ONLY")
    assert (r[mask != 0] == 0).all() and (r[mask == 0] != 0).all()
    tw.eval(rebase_only=True, set=True)                                  # no mask: every env; SET changes nothing here
    # SET against add and OR on the same pre-filled arrays
    put(60, 0, 3, 201)
    a0, t0 = tw.rew.copy(), tw.term.copy()
    r, done, _, _ = tw.eval()
    assert done.all() and np.array_equal(tw.rew, a0 + r) and np.array_equal(tw.term, t0 | 1) and (tw.term & 0x40).any()
    put(61, 0, 3, 0)
    r, done, _, _ = tw.eval(set=True)
    assert not done.any() and np.array_equal(tw.rew, r) and not tw.term.any()
    # optional outputs: each may be absent, the state moves all the same
    put(70, 1, 3, 0)
    tw.eval(rew=False, term=False, feat=False)
    tw.eval(feat=False)
    put(80, 2, 4, 0)
    tw.eval(rew=False)
    tw.eval(term=False)
    emu.close()


def check_ranges(make, dev, streams=None, n=192):
    """192 envs: a range [64, 100) writes those envs only, outputs and state (the evaluation of every
    env that follows proves the state); ranges [0, 64) and [64, 192) together equal one call (streams =
    a function (first, second) that runs them on two streams)."""
    emu = make(n)
    put_ram(emu, dev, 30)
    tw = Twin(emu, FULL, dev)
    mask = (np.arange(n) % 5 == 0).astype(np.uint8)
    tw.eval(rebase_only=True)
    put_ram(emu, dev, 31)
    tw.eval(mask, env0=64, count=36)
    put_ram(emu, dev, 32)
    tw.eval(mask, rebase_only=True, env0=128, count=64)
    tw.eval()
    put_ram(emu, dev, 33)
    run = streams if streams is not None else (lambda first, second: (first(), second()))

    def both(md, kw):
        run(lambda: emu.probes_eval(md, env0=0, count=64, **kw), lambda: emu.probes_eval(md, env0=64, count=128, **kw))

    tw.eval(mask, call=both)
    put_ram(emu, dev, 34)
    tw.eval(call=both)
    emu.close()


def raw(addr=0xC000, length=1, count=1, stride=0, kind=0, reduce=0, op=1, cmp=0, arg=0, weight=1.0):
    p = _native.PkProbe()
    p.addr, p.len, p.count, p.stride, p.kind, p.reduce, p.op, p.cmp, p.arg, p.weight = (
        addr, length, count, stride, kind, reduce, op, cmp, arg, weight)
    return p


BAD_PROBES = (
    dict(kind=4), dict(reduce=2), dict(op=4), dict(cmp=5), dict(length=0), dict(length=4), dict(kind=1, length=4),
    dict(kind=2, length=4), dict(kind=3, length=513), dict(kind=3, length=0), dict(count=0), dict(count=65),
    dict(weight=float("inf")), dict(weight=float("-inf")), dict(weight=float("nan")),
    dict(addr=0xBFFF), dict(addr=0x0000), dict(addr=0xDFFF, length=2), dict(addr=0xFDFF, length=2), dict(addr=0xFE00),
    dict(addr=0xFF7F), dict(addr=0xFFFE, length=2), dict(addr=0xFFFF), dict(addr=0xFF80, count=2, stride=0x7F),
    dict(addr=0xFFF0, count=2, stride=0x20), dict(addr=0xC000, count=64, stride=0x0100),
    dict(addr=0xDE00, kind=3, length=512, count=2, stride=0x100), dict(addr=0xFDF0, count=2, stride=0x10),
)


def check_guards(make, dev, n=192):
    """Every rejected argument is a negative code with a message and writes nothing; a handle on which
    creates failed still takes a correct one."""
    emu = make(n)
    L, h = emu._L, emu._h
    put_ram(emu, dev, 40)
    rew, term = dev(np.full(n, 0.25), np.float64), dev(np.full(n, 2), np.uint8)
    feat = dev(np.full((n, len(FULL)), -7), np.int32)

    def untouched():
        return ((rew.cpu().numpy() == 0.25).all() and (term.cpu().numpy() == 2).all() and (feat.cpu().numpy() == -7).all())

    def said(text):     # the failed call itself set the message: each is told apart by its own words
        return text in L.pk_last_error().decode(errors="replace")

    assert L.pk_probe_count(h) == 0
    assert L.pk_probe_eval(h, None, 0, 0, n, rew.data_ptr(), term.data_ptr(), feat.data_ptr(), None) < 0     # no program
    assert said("no probe program") and untouched()
    good = P.pack(FULL)
    for m in (0, 65):
        assert L.pk_probe_create(h, (_native.PkProbe * 65)(*[raw() for _ in range(65)]), m) < 0
        assert said("not %u" % m)
        assert L.pk_probe_count(h) == 0
    assert L.pk_probe_create(h, None, 1) < 0 and said("null argument") and L.pk_probe_count(h) == 0
    for bad in BAD_PROBES:
        for arr in ((_native.PkProbe * 1)(raw(**bad)), (_native.PkProbe * 3)(raw(), raw(addr=0xFF80), raw(**bad))):
            assert L.pk_probe_create(h, arr, len(arr)) < 0, bad
            assert said("probe %u" % (len(arr) - 1)) and L.pk_probe_count(h) == 0, bad
    for bad in ([], [P.u8(0xC000)] * 65, [raw()], "program"):
        with pytest.raises(ValueError):
            emu.probes_create(bad)
    for kw in (dict(addr=0xBFFF), dict(addr=0xC000, len=4), dict(addr=0xC000, kind="hex"), dict(addr=0xC000, op="sum"),
               dict(addr=0xC000, done=("lt", 3)), dict(addr=0xC000, weight=float("nan")), dict(addr=0xC000, count=65),
               dict(addr=0xDFFF, len=2), dict(addr=0xC000, reduce="min")):
        with pytest.raises(ValueError):
            P.Probe(**kw)
    assert L.pk_probe_count(h) == 0 and emu.probe_count == 0
    # the edges that are legal: the last bytes of WRAM, of the echo range and of HRAM
    edge = [P.Probe(0xDFFD, 3), P.Probe(0xFDFF, 1), P.Probe(0xFFFE, 1), P.Probe(0xFE00 - 512, 512, kind="bits"),
            P.Probe(0xC000, 1, 64, 0x7F)]
    assert ctypes.sizeof(_native.PkProbe) == 24 and len(P.pack(edge)) == 5
    tw = Twin(emu, FULL, dev)                                            # a correct create after the failures
    tw.eval(rebase_only=True)
    assert L.pk_probe_create(h, good, len(good)) < 0 and said("already has a probe program")
    assert L.pk_probe_count(h) == len(FULL)
    with pytest.raises(_native.PkError):
        emu.probes_create(edge)
    put_ram(emu, dev, 41)
    for mask, flags, env0, count in ((None, 4, 0, n), (None, 0x80000000, 0, n), (None, 0, 32, 8), (None, 0, 128, 65),
                                     (None, 0, 192, 1), (None, 0, 0, 0), (None, REBASE_ONLY | 8, 0, n)):
        assert L.pk_probe_eval(h, mask, flags, env0, count, rew.data_ptr(), term.data_ptr(), feat.data_ptr(), None) < 0
        assert said("unknown flags 0x%x" % flags if flags else "env range [%u, +%u)" % (env0, count)), (flags, env0, count)
        assert untouched(), (flags, env0, count)
    tw.eval(what="the failed calls left the state alone")                # pays the whole difference since the rebase
    put_ram(emu, dev, 42)
    tw.eval(env0=128, count=64)                                          # the last group is a legal range
    emu.close()
    other = make(64)
    other.probes_create(edge)
    assert other.probe_count == 5
    other.probes_eval()
    other.close()


def move_script(steps, n, seed=11):
    """Actions that walk: each env holds one direction (0..3: down, left, right, up) for a few steps, then
    another; now and then a button."""
    rng = np.random.default_rng(seed)
    acts = np.repeat(rng.integers(0, 4, (steps // 4 + 1, n)), 4, axis=0)[:steps]
    press = rng.integers(0, 16, (steps, n)) == 0
    return np.where(press, rng.integers(4, 8, (steps, n)), acts).astype(np.uint8)


def check_with_emulator(make, dev, n=64, steps=40):
    """The benchmark ROM under pkbench_program(): after every step the reward, the done flag and the
    features equal the model applied to get_ram reads of a twin emulator stepped by hand; the player
    does move, so CHANGE and DELTA pay."""
    prog = P.pkbench_program()
    emu, twin = make(n), make(n)
    emu.probes_create(prog)
    emu.reset()
    twin.reset()
    emu.probes_eval(rebase_only=True)
    state = np.zeros((n, len(prog)), np.uint32)
    P.model(prog, reader(twin), state, rebase_only=True)
    acts = move_script(steps, n)
    rew, term, feat = dev(np.zeros(n), np.float64), dev(np.zeros(n), np.uint8), dev(np.zeros((n, len(prog))), np.int32)
    changes = walked = 0
    for t in range(steps):
        emu.step(dev(acts[t], np.uint8))
        twin.step(dev(acts[t], np.uint8))
        emu.probes_eval(set=True, rewards=rew, terminals=term, features=feat)
        before = state.copy()
        r, done, v, _, _ = P.model(prog, reader(twin), state)
        assert np.array_equal(bits64(rew.cpu().numpy()), bits64(r)), t
        assert np.array_equal(term.cpu().numpy() != 0, done) and np.array_equal(feat.cpu().numpy(), v), t
        changes += int((v[:, 0] != before[:, 0]).sum())
        walked += int(((v[:, 1].astype(np.int64) - before[:, 1]) > 0).sum())
    assert changes >= n and walked >= n                                  # not a comparison of zeros
    emu.close()
    twin.close()


def vec_program(done_steps):
    """pkbench's position and step count, the episode ending once `done_steps` tiles were walked."""
    s = P.pkbench_symbols()
    return [P.le16(s["wPlayerX"], op="change", weight=1.0),
            P.u8(s["wStepCount"], op="delta", weight=0.01, done=("ge", done_steps)),
            P.u8(s["hJoyHeld"])]


def feature_reader(program, v):
    """A ram_reader over probe values: the probes of vec_program are single little-endian elements."""
    at = {p.addr: j for j, p in enumerate(program)}

    def read(addr, length):
        x = v[:, at[addr]].astype(np.int64)
        return np.stack([(x >> (8 * b)) & 0xFF for b in range(length)], axis=1).astype(np.uint8)

    return read


def _vec_run(env, dev, prog, steps, pipeline, base=None):
    """Drive env for `steps` steps of move_script and compare every returned reward and terminal with the
    model fed with probe_values: the state of an env that finished restarts from the values of the
    reset state.  probe_values are the kernel's own features, so this is independent of the kernel only
    for the reward, done and state logic, which is what VecEnv adds; the values themselves are checked
    against get_ram reads in check_model and check_with_emulator.  base: per step, the rewards and terminals of a twin without probes (reward=True)."""
    n = env.num_envs
    acts = move_script(steps, n, seed=29)
    env.reset() if not pipeline else env.async_reset()
    v0 = env.probe_values.cpu().numpy()
    assert (v0 == v0[0]).all()                                           # every env starts from the same machine
    state = v0.astype(np.uint32).copy()
    finished, paid, total = 0, 0, np.zeros(n)
    for t in range(steps):
        if pipeline:
            rew, term = np.zeros(n), np.zeros(n, bool)
            for _ in range(env.num_batches):
                _, _, _, _, _, _, _ = env.recv()
                sl = env.current_envs()
                env.send(dev(acts[t, sl], np.uint8))
            env._join_streams()
            for b in range(env.num_batches):
                r_b, t_b, _ = env._pending[b]
                rew[env._range(b)], term[env._range(b)] = r_b.cpu().numpy(), t_b.cpu().numpy()
        else:
            _, rew, term, _, _ = env.step(dev(acts[t], np.uint8))
            rew, term = rew.cpu().numpy(), term.cpu().numpy()
        v = env.probe_values.cpu().numpy()
        r, done, _, _, _ = P.model(prog, feature_reader(prog, v), state)
        b_rew, b_term = (np.zeros(n), np.zeros(n, bool)) if base is None else base[t]
        assert np.array_equal(bits64(rew), bits64(b_rew + r)), t
        assert np.array_equal(term, done | b_term), t
        state[term] = v0[term]                                           # measured from the reset state from here on
        finished += int(term.sum())
        paid += int((r != 0).sum())
        total += r
    return finished, paid, total


def check_vecenv(make_env, dev, reward, pipeline):
    """VecEnv(48, batch_size=24) on a 128-env emulator: step() or the recv() / send() pipeline return the
    probe reward; a probe's done ends the episode, resets the env and enters the episode statistics;
    the step after the reset is measured from the reset state."""
    prog = vec_program(200 if reward else 3)                             # with the twin: never done, so it stays in step
    env = make_env(reward=reward, probes=prog, probe_features=True)
    assert env.emu.n == 128 and env.emu.probe_count == 3 and tuple(env.probe_space.shape) == (3,)
    steps = 36
    base = None
    if reward:      # the reward stack's own rewards: a twin without probes, whose episodes never end here
        twin = make_env(reward=True)
        twin.reset()
        base = []
        for t in range(steps):
            _, r, d, _, _ = twin.step(dev(move_script(steps, 48, seed=29)[t], np.uint8))
            base.append((r.cpu().numpy(), d.cpu().numpy()))
        assert not any(d.any() for _, d in base)
        twin.emu.close()
    finished, paid, total = _vec_run(env, dev, prog, steps, pipeline, base)
    assert paid >= 48
    if reward:
        assert finished == 0
    else:
        assert finished >= 24
        if not pipeline:
            env._join_streams()
            summary = env.stats.summary.sum(dim=0).cpu().numpy()
            assert summary[1] == finished and summary[0] > 0 and abs(summary[3] - total.sum()) < 1e-9
    env.emu.close()


def check_vecenv_done_with_reward(make_env, dev):
    """reward=True and a probe's done: the episode ends, the env resets, and the probes are measured
    from the reset state (the model's rewards are the returned ones minus the reward stack's, which a
    finished env's twin no longer follows, so only terminals and features are compared)."""
    prog = vec_program(3)
    env = make_env(reward=True, probes=prog, probe_features=True)
    acts = move_script(30, 48, seed=29)
    env.reset()
    v0 = env.probe_values.cpu().numpy()
    state = v0.astype(np.uint32).copy()
    finished = 0
    for t in range(30):
        _, rew, term, _, _ = env.step(dev(acts[t], np.uint8))
        v = env.probe_values.cpu().numpy()
        _, done, _, _, _ = P.model(prog, feature_reader(prog, v), state)
        assert np.array_equal(term.cpu().numpy(), done), t
        state[done] = v0[done]
        finished += int(done.sum())
    assert finished >= 24
    env.emu.close()


def check_vecenv_bank(make_env, dev):
    """resume_from_bank, fork, load_from_bank, archive_explore and load_state rebase the envs whose
    machine they replaced, and only those: their next step pays what a model rebased to the values
    they hold now pays; every other env still pays its own difference."""
    prog = vec_program(200)
    env = make_env(reward=True, probes=prog, probe_features=True, bank_slots=2, bank_episodes=True, fork_slots=2,
                   archive_cells=4, max_episode_steps=1000)
    twin = make_env(reward=True, bank_slots=2, bank_episodes=True, fork_slots=2, archive_cells=4, max_episode_steps=1000)
    rng = np.random.default_rng(19)
    acts = move_script(64, 48, seed=31)
    clock = [0]
    env.reset()
    twin.reset()
    state = env.probe_values.cpu().numpy().astype(np.uint32)

    def step(k=1):
        for _ in range(k):
            a = dev(acts[clock[0]], np.uint8)
            clock[0] += 1
            _, rew, _, _, _ = env.step(a)
            _, base, _, _, _ = twin.step(a)
            v = env.probe_values.cpu().numpy()
            r, _, _, _, _ = P.model(prog, feature_reader(prog, v), state)
            assert np.array_equal(bits64(rew.cpu().numpy()), bits64(base.cpu().numpy() + r)), clock[0]

    def rebased(envs):
        """The model's state of the envs takes what they hold now: the values the rebase wrote."""
        v = env.probe_values.cpu().numpy()
        state[list(envs)] = v[list(envs)]

    def on_both(fn):
        return fn(env), fn(twin)

    step(4)
    on_both(lambda e: e.checkpoint_to_bank([3], [0]))
    on_both(lambda e: e.save_to_bank([4], [1]))
    step(4)
    on_both(lambda e: e.resume_from_bank([7, 30, 9], [0, 0, 1]))            # slot 1 holds no episode: env 9 is rejected
    assert env.emu.bank_rejects() == 1
    rebased([7, 30])
    step(3)
    on_both(lambda e: e.fork([11, 40], [2, 2]))
    rebased([11, 40])
    step(3)
    on_both(lambda e: e.load_from_bank([5, 47], [1, 1]))
    rebased([5, 47])
    step(3)
    on_both(lambda e: e.archive_update())
    step(3)
    mask = np.zeros(48, np.uint8)
    mask[[0, 25, 46]] = 1
    drawn = on_both(lambda e: e.archive_explore(dev(mask, np.uint8)).cpu().numpy())
    assert np.array_equal(*drawn) and (drawn[0][[0, 25, 46]] >= 0).all()
    rebased([0, 25, 46])
    step(3)
    snap = env.save_state(2)
    on_both(lambda e: e.load_state(33, snap))
    rebased([33])
    step(3)
    assert len(np.unique(state[:, 0])) > 4
    env.emu.close()
    twin.emu.close()


def check_vecenv_load_state(make_env, dev):
    """reward=False: load_state rebases the env it loads."""
    prog = vec_program(200)
    env = make_env(reward=False, probes=prog, probe_features=True)
    acts = move_script(16, 48, seed=37)
    env.reset()
    state = env.probe_values.cpu().numpy().astype(np.uint32)
    for t in range(16):
        if t == 8:
            env.load_state(33, env.save_state(2))
            v = env.probe_values.cpu().numpy()
            assert np.array_equal(v[33], v[2])
            state[33] = v[33]
        _, rew, _, _, _ = env.step(dev(acts[t], np.uint8))
        r, _, _, _, _ = P.model(prog, feature_reader(prog, env.probe_values.cpu().numpy()), state)
        assert np.array_equal(bits64(rew.cpu().numpy()), bits64(r)), t
    env.emu.close()


def check_vecenv_off(make_env, dev):
    """probes=None: no program, no calls — a handle whose probe entry points all fail steps as before."""
    for reward in (True, False):
        env, twin = make_env(reward=reward, probes=None), make_env(reward=reward)
        assert env.emu.probe_count == 0 and env.probes is None and env.probe_space is None

        def forbidden(*a, **k):
            raise AssertionError("probes=None must not call the probe entry points")

        env.emu.probes_eval = env.emu.probes_create = forbidden
        with pytest.raises(RuntimeError):
            env.probe_values
        a, b = env.reset()[0], twin.reset()[0]
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
        acts = move_script(4, 48)
        for t in range(4):
            x, y = env.step(dev(acts[t], np.uint8)), twin.step(dev(acts[t], np.uint8))
            for i in range(4):
                assert np.array_equal(x[i].cpu().numpy(), y[i].cpu().numpy())
        env.emu.close()
        twin.emu.close()


BAD_KEYWORDS = ({"probes": []}, {"probes": [P.u8(0xC000)] * 65}, {"probes": "pkbench"}, {"probes": [(0xC000, 1)]},
                {"probe_features": True}, {"probes": None, "probe_features": True})
