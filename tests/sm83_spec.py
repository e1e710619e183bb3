"""SM83 (Game Boy CPU) instruction semantics as the published CPU documentation states them (Pan
Docs, "CPU Instruction Set"; the GBCPUman flag tables) — TEST INFRASTRUCTURE ONLY.

An independent statement of what each tested instruction does to A, F (Z N H C in bits 7-4, the low
nibble always 0), HL and SP, written from the documentation, not from PyBoy or from
oracle/gbcore.c.  tests/test_sm83_kat.py runs pokegym_amd/testrom/kat.py's known-answer ROM on the
oracle (and on the HIP kernel) and compares its per-block checksums with the ones computed here, so
the oracle's per-instruction semantics are pinned to the documented CPU, not only to the builder's
own restatement of PyBoy (PyBoy itself is absent, so CPU trajectories stay unpinned).

step() states the whole architectural effect (A F B C D E H L SP PC and the memory writes) of every
legal base opcode and every CB opcode; tests/test_sm83_matrix.py folds it over the instruction
streams of pokegym_amd/testrom/kat_matrix.py's blocks.  Not stated by step():
  HALT (76)      its wake-up depends on interrupt timing, which follows PyBoy, not the documentation
  STOP (10)      stops the clocks until a button is pressed: a machine state, not a register effect
  DI / EI (F3/FB) only change IME, which shows through interrupt dispatch alone (PyBoy's timing)
  RETI's IME side same reason; its return (PC, SP) is stated, and the ROM runs it with IE = 0
  the eleven illegal opcodes (D3 DB DD E3 E4 EB EC ED F4 FC FD) hang the CPU: nothing to state
"""
from __future__ import annotations

Z, N, H, C = 0x80, 0x40, 0x20, 0x10


def _f(z, n, h, c):
    return (Z if z else 0) | (N if n else 0) | (H if h else 0) | (C if c else 0)


def alu(op: str, a: int, v: int, cy: int):
    """8-bit ALU A,v with carry-in cy: (A', F')."""
    if op == "add":
        r = a + v
        return r & 0xFF, _f((r & 0xFF) == 0, 0, (a & 0xF) + (v & 0xF) > 0xF, r > 0xFF)
    if op == "adc":
        r = a + v + cy
        return r & 0xFF, _f((r & 0xFF) == 0, 0, (a & 0xF) + (v & 0xF) + cy > 0xF, r > 0xFF)
    if op in ("sub", "cp"):
        r = a - v
        res = (r & 0xFF, _f((r & 0xFF) == 0, 1, (a & 0xF) < (v & 0xF), a < v))
        return (a, res[1]) if op == "cp" else res
    if op == "sbc":
        r = a - v - cy
        return r & 0xFF, _f((r & 0xFF) == 0, 1, (a & 0xF) < (v & 0xF) + cy, a < v + cy)
    if op == "and":
        r = a & v
        return r, _f(r == 0, 0, 1, 0)
    if op == "xor":
        r = a ^ v
        return r, _f(r == 0, 0, 0, 0)
    if op == "or":
        r = a | v
        return r, _f(r == 0, 0, 0, 0)
    raise ValueError(op)


def inc_dec(op: str, a: int, f: int):
    """INC A / DEC A: carry kept."""
    if op == "inc":
        r = (a + 1) & 0xFF
        return r, _f(r == 0, 0, (a & 0xF) == 0xF, f & C)
    r = (a - 1) & 0xFF
    return r, _f(r == 0, 1, (a & 0xF) == 0, f & C)


def daa(a: int, f: int):
    """DAA after an addition (N clear) or a subtraction (N set), Pan Docs' statement."""
    n, h, c = f & N, f & H, f & C
    if not n:
        if c or a > 0x99:
            a += 0x60
            c = 1
        if h or (a & 0x0F) > 0x09:
            a += 0x06
    else:
        if c:
            a -= 0x60
        if h:
            a -= 0x06
    a &= 0xFF
    return a, _f(a == 0, n, 0, c)


def cb_rot(op: str, a: int, cy: int):
    """CB-prefixed rotate/shift/swap on A: Z from the result, N = H = 0."""
    if op == "rlc":
        c = a >> 7
        r = ((a << 1) | c) & 0xFF
    elif op == "rrc":
        c = a & 1
        r = (a >> 1) | (c << 7)
    elif op == "rl":
        c = a >> 7
        r = ((a << 1) | cy) & 0xFF
    elif op == "rr":
        c = a & 1
        r = (a >> 1) | (cy << 7)
    elif op == "sla":
        c = a >> 7
        r = (a << 1) & 0xFF
    elif op == "sra":
        c = a & 1
        r = (a >> 1) | (a & 0x80)
    elif op == "swap":
        c = 0
        r = ((a << 4) | (a >> 4)) & 0xFF
    elif op == "srl":
        c = a & 1
        r = a >> 1
    else:
        raise ValueError(op)
    return r, _f(r == 0, 0, 0, c)


def acc_rot(op: str, a: int, cy: int):
    """RLCA / RRCA / RLA / RRA: as the CB forms, but Z always clear."""
    r, f = cb_rot({"rlca": "rlc", "rrca": "rrc", "rla": "rl", "rra": "rr"}[op], a, cy)
    return r, f & ~Z & 0xFF


def bit(b: int, a: int, f: int):
    return a, _f(not ((a >> b) & 1), 0, 1, f & C)


def misc(op: str, a: int, f: int):
    """CPL / SCF / CCF: Z kept."""
    if op == "cpl":
        return a ^ 0xFF, (f & (Z | C)) | N | H
    if op == "scf":
        return a, (f & Z) | C
    if op == "ccf":
        return a, (f & Z) | (0 if f & C else C)
    raise ValueError(op)


def add_hl(hl: int, rr: int, f: int):
    """ADD HL,rr: Z kept, N = 0, H from bit 11, C from bit 15."""
    r = hl + rr
    return r & 0xFFFF, (f & Z) | (H if (hl & 0xFFF) + (rr & 0xFFF) > 0xFFF else 0) | (C if r > 0xFFFF else 0)


def sp_plus(sp: int, e: int):
    """ADD SP,e and LD HL,SP+e: result, F = 0 | H / C from the unsigned low-byte sum."""
    se = e - 256 if e & 0x80 else e
    r = (sp + se) & 0xFFFF
    return r, (H if (sp & 0xF) + (e & 0xF) > 0xF else 0) | (C if (sp & 0xFF) + (e & 0xFF) > 0xFF else 0)


class Fletcher:
    """The ROM's running hash (pokegym_amd/testrom/kat.py acc1): h = rotl16(h, 5) + byte, mod 2^16;
    pair() = (low byte, high byte) as the ROM stores them."""

    def __init__(self):
        self.h = 0

    def add(self, *bs):
        for b in bs:
            self.h = ((((self.h << 5) | (self.h >> 11)) & 0xFFFF) + b) & 0xFFFF

    def pair(self):
        return self.h & 0xFF, self.h >> 8


# ---- instruction timing (T-states, Pan Docs / the opcode tables): (not taken, taken) ----
ILLEGAL = {0xD3, 0xDB, 0xDD, 0xE3, 0xE4, 0xEB, 0xEC, 0xED, 0xF4, 0xFC, 0xFD}
# opcodes step() does not state (they raise NotImplementedError there)
OUT_OF_SCOPE = {0x76, 0x10, 0xF3, 0xFB}


def cycles(op: int):
    """T-states of base opcode op as (cycles, cycles when a condition holds) — equal for the
    unconditional ones; None for the illegal opcodes and the CB prefix (see cb_cycles)."""
    if op in ILLEGAL or op == 0xCB:
        return None
    hi, lo = op >> 6, op & 7
    if 0x40 <= op < 0x80:                       # LD r,r' / LD r,(HL) / LD (HL),r / HALT
        if op == 0x76:
            return (4, 4)
        return (8, 8) if (lo == 6 or (op >> 3) & 7 == 6) else (4, 4)
    if 0x80 <= op < 0xC0:                       # ALU A,r / A,(HL)
        return (8, 8) if lo == 6 else (4, 4)
    fixed = {
        0x00: 4, 0x10: 4, 0x76: 4, 0xF3: 4, 0xFB: 4, 0x27: 4, 0x2F: 4, 0x37: 4, 0x3F: 4,
        0x07: 4, 0x0F: 4, 0x17: 4, 0x1F: 4,
        0x02: 8, 0x12: 8, 0x22: 8, 0x32: 8, 0x0A: 8, 0x1A: 8, 0x2A: 8, 0x3A: 8,
        0x08: 20, 0xE0: 12, 0xF0: 12, 0xE2: 8, 0xF2: 8, 0xEA: 16, 0xFA: 16,
        0xF8: 12, 0xF9: 8, 0xE8: 16, 0x36: 12, 0x34: 12, 0x35: 12,
        0xC3: 16, 0xE9: 4, 0x18: 12, 0xCD: 24, 0xC9: 16, 0xD9: 16,
    }
    if op in fixed:
        return (fixed[op], fixed[op])
    if hi == 0:
        if lo == 1:
            return (12, 12) if op & 0x08 == 0 else (8, 8)          # LD rr,nn / ADD HL,rr
        if lo == 3:
            return (8, 8)                                           # INC / DEC rr
        if lo in (4, 5):
            return (4, 4)                                           # INC / DEC r
        if lo == 6:
            return (8, 8)                                           # LD r,n
        if lo == 0 and op in (0x20, 0x28, 0x30, 0x38):
            return (8, 12)                                          # JR cc,e
    if hi == 3:
        if lo == 6:
            return (8, 8)                                           # ALU A,n
        if lo == 7:
            return (16, 16)                                         # RST
        if lo == 5:
            return (16, 16)                                         # PUSH
        if lo == 1:
            return (12, 12)                                         # POP
        if op in (0xC2, 0xCA, 0xD2, 0xDA):
            return (12, 16)                                         # JP cc,nn
        if op in (0xC4, 0xCC, 0xD4, 0xDC):
            return (12, 24)                                         # CALL cc,nn
        if op in (0xC0, 0xC8, 0xD0, 0xD8):
            return (8, 20)                                          # RET cc
    raise KeyError(f"no documented timing for {op:02X}")


def cb_cycles(op: int) -> int:
    """T-states of CB-prefixed op: 8 on a register, 16 on (HL), BIT n,(HL) 12."""
    if op & 7 != 6:
        return 8
    return 12 if 0x40 <= op < 0x80 else 16


# ---- the whole instruction: registers, PC, SP and memory writes ----
R8_NAMES = ("B", "C", "D", "E", "H", "L", None, "A")           # operand field 6 is (HL)
R16_NAMES = (("B", "C"), ("D", "E"), ("H", "L"))               # pair field 3 is SP (or AF for PUSH / POP)
ALU_NAMES = ("add", "adc", "sub", "sbc", "and", "xor", "or", "cp")
CB_NAMES = ("rlc", "rrc", "rl", "rr", "sla", "sra", "swap", "srl")
_LEN3 = {0x01, 0x11, 0x21, 0x31, 0x08, 0xC3, 0xC2, 0xCA, 0xD2, 0xDA, 0xCD, 0xC4, 0xCC, 0xD4, 0xDC, 0xEA, 0xFA}
_LEN2 = ({0x06 | (r << 3) for r in range(8)} | {0xC6 | (f << 3) for f in range(8)}
         | {0x18, 0x20, 0x28, 0x30, 0x38, 0xE0, 0xF0, 0xE8, 0xF8, 0x10, 0xCB})


def length(op: int) -> int:
    """Bytes of the instruction that starts with base opcode op (CB-prefixed: 2)."""
    return 3 if op in _LEN3 else 2 if op in _LEN2 else 1


def step(regs: dict, mem, op_bytes):
    """One instruction, as the documentation states it.  regs: A F B C D E H L (bytes), SP, PC (PC the
    instruction's own address); mem[addr] reads a byte; op_bytes the instruction's length(op) bytes.
    Returns (regs', writes, cycles_taken): writes the (addr, value) byte writes in bus order —
    not applied to mem: the caller does that."""
    r = dict(regs)
    writes = []
    op = op_bytes[0]
    if op in ILLEGAL or op in OUT_OF_SCOPE:
        raise NotImplementedError(f"opcode {op:02X} is not stated")
    n = op_bytes[1] if len(op_bytes) > 1 else 0
    nn = n | (op_bytes[2] << 8) if len(op_bytes) > 2 else 0
    nxt = (regs["PC"] + length(op)) & 0xFFFF
    r["PC"] = nxt
    taken = False

    def rd(a):
        for wa, wv in reversed(writes):
            if wa == a & 0xFFFF:
                return wv
        return mem[a & 0xFFFF]

    def wr(a, v):
        writes.append((a & 0xFFFF, v & 0xFF))

    def get16(p):
        if p == 3:
            return r["SP"]
        h, l = R16_NAMES[p]
        return (r[h] << 8) | r[l]

    def set16(p, v):
        if p == 3:
            r["SP"] = v & 0xFFFF
        else:
            h, l = R16_NAMES[p]
            r[h], r[l] = (v >> 8) & 0xFF, v & 0xFF

    def get8(i):
        return rd(get16(2)) if i == 6 else r[R8_NAMES[i]]

    def set8(i, v):
        if i == 6:
            wr(get16(2), v)
        else:
            r[R8_NAMES[i]] = v & 0xFF

    def push(v):
        r["SP"] = (r["SP"] - 2) & 0xFFFF
        wr(r["SP"] + 1, v >> 8)
        wr(r["SP"], v & 0xFF)

    def pop():
        v = rd(r["SP"]) | (rd(r["SP"] + 1) << 8)
        r["SP"] = (r["SP"] + 2) & 0xFFFF
        return v

    def cond(k):                                   # NZ Z NC C
        flag = r["F"] & (Z if k < 2 else C)
        return bool(flag) == bool(k & 1)

    hi, mid, lo = op >> 6, (op >> 3) & 7, op & 7
    cy = 1 if r["F"] & C else 0
    if op == 0xCB:
        v = get8(n & 7)
        b = (n >> 3) & 7
        if n < 0x40:
            res, r["F"] = cb_rot(CB_NAMES[b], v, cy)
            set8(n & 7, res)
        elif n < 0x80:
            _, r["F"] = bit(b, v, r["F"])
        elif n < 0xC0:
            set8(n & 7, v & ~(1 << b))             # RES b
        else:
            set8(n & 7, v | (1 << b))              # SET b
        return r, writes, cb_cycles(n)
    if hi == 1:                                    # LD r,r' / LD r,(HL) / LD (HL),r
        set8(mid, get8(lo))
    elif hi == 2:                                  # ALU A,r / A,(HL)
        r["A"], r["F"] = alu(ALU_NAMES[mid], r["A"], get8(lo), cy)
    elif hi == 0:
        if op == 0x00:
            pass
        elif op == 0x08:                           # LD (nn),SP
            wr(nn, r["SP"] & 0xFF)
            wr(nn + 1, r["SP"] >> 8)
        elif op == 0x18 or (lo == 0 and mid >= 4):  # JR e / JR cc,e
            taken = op == 0x18 or cond(mid - 4)
            if taken:
                r["PC"] = (nxt + (n - 256 if n & 0x80 else n)) & 0xFFFF
        elif lo == 1 and not mid & 1:              # LD rr,nn
            set16(mid >> 1, nn)
        elif lo == 1:                              # ADD HL,rr
            v, r["F"] = add_hl(get16(2), get16(mid >> 1), r["F"])
            set16(2, v)
        elif lo == 2:                              # LD (BC/DE/HL+/HL-),A and LD A,(..)
            p = min(mid >> 1, 2)
            a = get16(p)
            if mid & 1:
                r["A"] = rd(a)
            else:
                wr(a, r["A"])
            if mid >> 1 == 2:
                set16(2, a + 1)                    # (HL+)
            if mid >> 1 == 3:
                set16(2, a - 1)                    # (HL-)
        elif lo == 3:                              # INC rr / DEC rr: no flags
            set16(mid >> 1, get16(mid >> 1) + (-1 if mid & 1 else 1))
        elif lo in (4, 5):                         # INC r / DEC r / (HL)
            v, r["F"] = inc_dec("inc" if lo == 4 else "dec", get8(mid), r["F"])
            set8(mid, v)
        elif lo == 6:                              # LD r,n / LD (HL),n
            set8(mid, n)
        elif mid < 4:
            r["A"], r["F"] = acc_rot(("rlca", "rrca", "rla", "rra")[mid], r["A"], cy)
        elif mid == 4:
            r["A"], r["F"] = daa(r["A"], r["F"])
        else:
            r["A"], r["F"] = misc(("cpl", "scf", "ccf")[mid - 5], r["A"], r["F"])
    else:
        if lo == 0 and mid < 4:                    # RET cc
            taken = cond(mid)
            if taken:
                r["PC"] = pop()
        elif op == 0xE0:                           # LDH (n),A
            wr(0xFF00 + n, r["A"])
        elif op == 0xF0:                           # LDH A,(n)
            r["A"] = rd(0xFF00 + n)
        elif op == 0xE8:                           # ADD SP,e
            r["SP"], r["F"] = sp_plus(r["SP"], n)
        elif op == 0xF8:                           # LD HL,SP+e
            v, r["F"] = sp_plus(r["SP"], n)
            set16(2, v)
        elif lo == 1 and not mid & 1:              # POP rr / POP AF: F's low nibble reads 0
            v = pop()
            if mid >> 1 == 3:
                r["A"], r["F"] = v >> 8, v & 0xF0
            else:
                set16(mid >> 1, v)
        elif op in (0xC9, 0xD9):                   # RET / RETI (IME not stated)
            r["PC"] = pop()
        elif op == 0xE9:                           # JP HL
            r["PC"] = get16(2)
        elif op == 0xF9:                           # LD SP,HL
            r["SP"] = get16(2)
        elif lo == 2 and mid < 4:                  # JP cc,nn
            taken = cond(mid)
            if taken:
                r["PC"] = nn
        elif op == 0xE2:                           # LD (C),A
            wr(0xFF00 + r["C"], r["A"])
        elif op == 0xF2:                           # LD A,(C)
            r["A"] = rd(0xFF00 + r["C"])
        elif op == 0xEA:                           # LD (nn),A
            wr(nn, r["A"])
        elif op == 0xFA:                           # LD A,(nn)
            r["A"] = rd(nn)
        elif op == 0xC3:                           # JP nn
            r["PC"] = nn
        elif op == 0xCD or (lo == 4 and mid < 4):  # CALL nn / CALL cc,nn
            taken = op == 0xCD or cond(mid)
            if taken:
                push(nxt)
                r["PC"] = nn
        elif lo == 5:                              # PUSH rr / PUSH AF: high byte first, at SP-1
            push((r["A"] << 8) | r["F"] if mid >> 1 == 3 else get16(mid >> 1))
        elif lo == 6:                              # ALU A,n
            r["A"], r["F"] = alu(ALU_NAMES[mid], r["A"], n, cy)
        elif lo == 7:                              # RST
            push(nxt)
            r["PC"] = mid * 8
        else:
            raise NotImplementedError(f"opcode {op:02X}")
    c0, c1 = cycles(op)
    return r, writes, c1 if taken else c0
