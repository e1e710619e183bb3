"""RAM probe programs (pk_probe_*, include/pokegym_amd.h): a reward, a done flag and a feature vector
read from every env's RAM by a small table, on any cartridge.

A program is a list of Probe records; pack() makes the C array pk_probe_create takes, and model() is
the header's model restated in numpy — what the documents quote and what the tests compare the
kernel with, bit for bit.  pkbench_program() is a program for the benchmark ROM (testrom/game.py);
pokemon_red_program() is an example over the Pokémon Red addresses this project already cites."""
from __future__ import annotations

import math
import re
from dataclasses import dataclass

import numpy as np

from . import _native
from ._native import (PK_PC_EQ, PK_PC_GE, PK_PC_LE, PK_PC_NE, PK_PC_NONE, PK_PO_CHANGE, PK_PO_DELTA, PK_PO_NEWMAX,
                      PK_PO_NONE, PK_PR_MAX, PK_PR_SUM, PK_PV_BCD, PK_PV_BE, PK_PV_BITS, PK_PV_LE)

KINDS = {"le": PK_PV_LE, "be": PK_PV_BE, "bcd": PK_PV_BCD, "bits": PK_PV_BITS}
REDUCES = {"sum": PK_PR_SUM, "max": PK_PR_MAX}
OPS = {None: PK_PO_NONE, "none": PK_PO_NONE, "delta": PK_PO_DELTA, "newmax": PK_PO_NEWMAX, "change": PK_PO_CHANGE}
CMPS = {None: PK_PC_NONE, "none": PK_PC_NONE, "eq": PK_PC_EQ, "ne": PK_PC_NE, "ge": PK_PC_GE, "le": PK_PC_LE}
MAX_PROBES = _native.PK_PROBE_MAX


@dataclass(frozen=True)
class Probe:
    """One probe: `count` elements of `len` bytes, `stride` bytes apart from guest address `addr`, read
    as `kind` ("le", "be", "bcd", "bits") and reduced by `reduce` ("sum", "max") to the value v; `op`
    (None, "delta", "newmax", "change") and `weight` turn v into reward, `done` = (cmp, arg) with cmp
    "eq", "ne", "ge" or "le" into a termination condition."""
    addr: int
    len: int = 1
    count: int = 1
    stride: int = 0
    kind: str = "le"
    reduce: str = "sum"
    op: str | None = None
    weight: float = 0.0
    done: tuple | None = None

    def __post_init__(self):
        if self.kind not in KINDS:
            raise ValueError(f"probe kind must be one of {sorted(KINDS)}")
        if self.reduce not in REDUCES:
            raise ValueError("probe reduce must be 'sum' or 'max'")
        if self.op not in OPS:
            raise ValueError("probe op must be None, 'delta', 'newmax' or 'change'")
        if self.done is not None and (len(self.done) != 2 or self.done[0] not in CMPS
                                      or not 0 <= int(self.done[1]) < 1 << 32):
            raise ValueError("probe done must be (cmp, arg) with cmp 'eq', 'ne', 'ge' or 'le' and a u32 arg")
        if not 1 <= self.len <= (512 if self.kind == "bits" else 3):
            raise ValueError("probe len must be 1..3 (1..512 for 'bits')")
        if not 1 <= self.count <= MAX_PROBES:
            raise ValueError(f"probe count must be 1..{MAX_PROBES}")
        if not 0 <= self.stride < 1 << 16 or not 0 <= self.addr < 1 << 16:
            raise ValueError("probe addr and stride are 16-bit")
        if not math.isfinite(self.weight):
            raise ValueError("probe weight must be finite")
        for k in range(self.count):
            a = self.addr + k * self.stride
            wram = a >= 0xC000 and a + self.len <= 0xFE00 and (a & 0x1FFF) + self.len <= 0x2000
            hram = a >= 0xFF80 and a + self.len <= 0xFFFF
            if not (wram or hram):
                raise ValueError(f"probe element {k} [0x{a:04x}, +{self.len}) is not inside WRAM/echo or HRAM")

    @property
    def cmp(self) -> int:
        return CMPS[self.done[0]] if self.done is not None else PK_PC_NONE

    @property
    def arg(self) -> int:
        return int(self.done[1]) if self.done is not None else 0


def u8(addr, op=None, weight=0.0, done=None):
    """One byte."""
    return Probe(addr, 1, op=op, weight=weight, done=done)


def le16(addr, op=None, weight=0.0, done=None):
    """A little-endian 16-bit word."""
    return Probe(addr, 2, op=op, weight=weight, done=done)


def be(addr, length=2, op=None, weight=0.0, done=None):
    """A big-endian unsigned number of 1..3 bytes."""
    return Probe(addr, length, kind="be", op=op, weight=weight, done=done)


def bcd(addr, length=3, op=None, weight=0.0, done=None):
    """A big-endian packed BCD number of 1..3 bytes."""
    return Probe(addr, length, kind="bcd", op=op, weight=weight, done=done)


def bits(addr, length=1, op=None, weight=0.0, done=None):
    """The number of set bits in 1..512 bytes."""
    return Probe(addr, length, kind="bits", op=op, weight=weight, done=done)


def array_sum(addr, count, stride, length=1, kind="le", op=None, weight=0.0, done=None):
    """The sum over `count` elements `stride` bytes apart."""
    return Probe(addr, length, count, stride, kind, "sum", op, weight, done)


def array_max(addr, count, stride, length=1, kind="le", op=None, weight=0.0, done=None):
    """The maximum over `count` elements `stride` bytes apart."""
    return Probe(addr, length, count, stride, kind, "max", op, weight, done)


def _program(program) -> list:
    program = list(program)
    if not 1 <= len(program) <= MAX_PROBES or not all(isinstance(p, Probe) for p in program):
        raise ValueError(f"a probe program is 1..{MAX_PROBES} Probe records")
    return program


def pack(program):
    """The program as the C array pk_probe_create takes (a ctypes array of pk_probe)."""
    program = _program(program)
    arr = (_native.PkProbe * len(program))()
    for c, p in zip(arr, program):
        c.addr, c.len, c.count, c.stride = p.addr, p.len, p.count, p.stride
        c.kind, c.reduce, c.op, c.cmp = KINDS[p.kind], REDUCES[p.reduce], OPS[p.op], p.cmp
        c.arg, c.weight = p.arg, float(p.weight)
    return arr


def values(program, ram_reader) -> np.ndarray:
    """The probe values v, int64 (n, m).  ram_reader(addr, length) returns uint8 (n, length): the bytes of
    every env at [addr, addr + length)."""
    cols = []
    for p in _program(program):
        elems = []
        for k in range(p.count):
            b = np.asarray(ram_reader(p.addr + k * p.stride, p.len), np.uint8).astype(np.int64)
            if p.kind == "bits":
                x = np.unpackbits(b.astype(np.uint8), axis=1).sum(axis=1, dtype=np.int64)
            else:
                x = np.zeros(len(b), np.int64)
                for i in range(p.len):
                    if p.kind == "le":
                        x |= b[:, i] << (8 * i)
                    elif p.kind == "be":
                        x = x << 8 | b[:, i]
                    else:
                        x = (x * 10 + (b[:, i] >> 4)) * 10 + (b[:, i] & 15)
            elems.append(x)
        e = np.stack(elems)
        cols.append(e.max(axis=0) if p.reduce == "max" else e.sum(axis=0))
    return np.stack(cols, axis=1)


def model(program, ram_reader, state, mask=None, rebase_only=False):
    """One pk_probe_eval over every env, in numpy.  state: uint32 (n, m), updated in place.  mask and
    rebase_only are the call's.  Returns (r, done, v, evaluated, took): the reward float64 (n,), the
    done flag bool (n,), the values int32 (n, m), which envs evaluated and which took part (bool (n,));
    an env that took part without evaluating rebased, and has r = +0.0 and done = False.  The caller
    applies rew += r / rew = r and term |= done / term = done to the evaluating envs and takes the
    rows of v of the envs that took part."""
    program = _program(program)
    v = values(program, ram_reader)
    n = len(v)
    m = np.zeros(n, bool) if mask is None else np.asarray(mask) != 0
    if rebase_only:
        took = np.ones(n, bool) if mask is None else m
        rebase = took
    else:
        took, rebase = np.ones(n, bool), m
    ev = took & ~rebase
    r = np.zeros(n, np.float64)
    done = np.zeros(n, bool)
    for j, p in enumerate(program):
        vj, s = v[:, j], state[:, j].astype(np.int64)
        a = p.arg
        if p.cmp:
            done |= {PK_PC_EQ: vj == a, PK_PC_NE: vj != a, PK_PC_GE: vj >= a, PK_PC_LE: vj <= a}[p.cmp]
        if OPS[p.op] == PK_PO_NONE:
            continue
        w = np.float64(p.weight)
        if p.op == "delta":
            c, sn = w * (vj - s).astype(np.float64), vj          # one rounded product
        elif p.op == "newmax":
            c, sn = np.where(vj > s, w * (vj - s).astype(np.float64), 0.0), np.maximum(s, vj)
        else:
            c, sn = np.where(vj != s, w, 0.0), vj
        r = r + np.where(ev, c, 0.0)                             # one rounded sum per probe
        state[:, j] = np.where(rebase, vj, np.where(ev, sn, s)).astype(np.uint32)
    return np.where(ev, r, 0.0), done & ev, v.astype(np.int32), ev, took


def pkbench_symbols() -> dict:
    """The `equ` addresses of the benchmark ROM's source: w* names are WRAM addresses, h* names HRAM
    offsets from 0xFF00."""
    from .testrom import game
    out = {}
    for name, val in re.findall(r"^(\w+) equ \$([0-9a-fA-F]+)\s*$", game.SRC, re.M):
        out[name] = int(val, 16) + (0xFF00 if name.startswith("h") else 0)
    return out


def pkbench_program() -> list:
    """A program for the benchmark ROM: 1.0 for every step that changes the player's position (wPlayerX,
    wPlayerY read as one word), 0.01 per tile walked (wStepCount's difference; the byte wraps at 256),
    and the episode ends at the first battle: the ROM loads wBattleHP with 40 when one starts, and it
    is 0 from power-on until then.  The enemy's HP is a feature only."""
    s = pkbench_symbols()
    return [le16(s["wPlayerX"], op="change", weight=1.0),
            u8(s["wStepCount"], op="delta", weight=0.01),
            u8(s["wBattleHP"], done=("ge", 1)),
            u8(s["wBattleEnemyHP"])]


def pokemon_red_program() -> list:
    """An EXAMPLE over Pokémon Red's WRAM, from the addresses reward_tables.py and oracle/reward.py cite;
    it is not PK_F_REWARD's reward (no exploration, healing, or event weights) and does not replace it.
    Badges (the set bits of 0xD356) and the sum of the six party levels (0xD18C, 0x2C apart) pay for
    new maxima, as do the event flags 0xD747-0xD885 (319 bytes, one bit count); the money (3 BCD bytes
    at 0xD347) and the highest party level are features; eight badges end the episode."""
    return [bits(0xD356, 1, op="newmax", weight=10.0, done=("ge", 8)),
            array_sum(0xD18C, 6, 0x2C, op="newmax", weight=1.0),
            bits(0xD747, 0xD886 - 0xD747, op="newmax", weight=1.0),
            bcd(0xD347, 3),
            array_max(0xD18C, 6, 0x2C)]
