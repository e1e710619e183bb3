"""Opcode-matrix known-answer ROM for the SM83 (TEST CONTENT): every legal opcode but HALT / STOP /
DI / EI, one block per (opcode, path variant), each block run over V seeded input vectors.

A block is a few bytes of code around one opcode.  The driver loads a vector — A, F's high nibble, B,
C, D, E, H, L and the eight bytes of the scratch window wScr (its first two also seed the HRAM bytes
$FF90 and $FFC0) — and enters the block by popping the registers and the block's address off a WRAM
frame, so no register is touched after the load.  The block sets SP (into the scratch window: PUSH /
CALL / RST write it, POP reads it), points the pair a memory form goes through at the window and
reaches the opcode
  primary  through a taken `jp`: a control transfer never lets its successor run as a fused
           secondary op, so the step kernel's primary table entry runs it;
  fused    through `jp` / `nop`: the nop runs as a primary and the opcode, directly behind a fusable
           register instruction, as its fused secondary op (only for opcodes the kernel has a
           secondary entry for: FUSED_OPS).
What follows the opcode jumps to a capture routine: `cap` (marker left as it is: 0, or what an RST
stub wrote), `cap1` (fell through: marker $5A) or `cap2` (a jump / call / return landed: $A5).  The
capture stores SP, pushes AF BC DE HL into a save area and folds the ten register bytes, the
scratch window, the marker and the two HRAM bytes into the block's 16-bit hash (kat.py's acc1:
h = rotl16(h, 5) + byte); after V vectors the hash goes to wOut + 2 * block.  The conditional JP /
JR / CALL / RET blocks are taken or not with the vector's flags (the fixed vectors hold every combination of Z and C), JR
runs forward and backward, RET / RETI pop a return address from ROM, the RST stubs at $00..$38
write marker $10 + n and return.

tests/sm83_spec.py step() states what the documented CPU does with the same bytes; the tests fold
it over each block's instruction stream (tests/test_sm83_matrix.py) and compare the hashes for the
oracle, the host-simulated step kernel and the HIP kernel.

Group selection as in kat.py: a pressed button runs the blocks of its group (block k: group k % 8),
none runs all.  Blocks alternate, eight at a time, between bank 0 and one switchable bank: bank 1 of
a 2-bank cartridge, bank HIGH_BANK of a 64-bank one (above the banks the step kernel stages in LDS:
fetched from the global ROM)."""
from __future__ import annotations

import math
import random

from .kat import GROUP_ACTION, W_DONE, W_GRP, W_S1, W_S2  # noqa: F401  (GROUP_ACTION re-exported)
from .sm83asm import build_rom

HIGH_BANK = 37
W_SAVE, W_SAVESP, W_SCR, W_MARK, W_H0, W_H1 = 0xC0F2, 0xC0FA, 0xC0FC, 0xC104, 0xC105, 0xC106   # hashed, in order
HASHED = W_H1 + 1 - W_SAVE
W_REGS, W_ENTRY = 0xC010, 0xC018          # the frame the block is entered from: F A C B E D L H, entry
W_GIDX, W_LIST, W_OUTP, W_VEC = 0xC006, 0xC008, 0xC00A, 0xC00C
W_OUT = 0xC200
TEST_SP = W_SCR + 4                       # $C100: pushes land in the window's bytes 2-3, pops read 4-5
HRAM_LO, HRAM_HI = 0x90, 0xC0             # inside / above the step kernel's LDS mirror of $FF80-$FF9F
MARK_FELL, MARK_LANDED, MARK_RST = 0x5A, 0xA5, 0x10
ILLEGAL = {0xD3, 0xDB, 0xDD, 0xE3, 0xE4, 0xEB, 0xEC, 0xED, 0xF4, 0xFC, 0xFD}
OUT_OF_SCOPE = {0x76, 0x10, 0xF3, 0xFB}   # HALT STOP DI EI
# opcodes the step kernel's secondary table implements (tests/test_sm83_matrix.py checks this list
# against the table the host simulation builds): NOP, LD r,r', LD r,n, INC/DEC r, INC/DEC BC/DE/HL,
# ALU A,r / A,n, CPL, SCF, JR (cc)
FUSED_OPS = sorted({0x00, 0x2F, 0x37, 0x18, 0x20, 0x28, 0x30, 0x38}
                   | {op for op in range(0x40, 0x80) if op & 7 != 6 and (op >> 3) & 7 != 6}
                   | {0x06 | (r << 3) for r in range(8) if r != 6}
                   | {b | (r << 3) for r in range(8) if r != 6 for b in (0x04, 0x05)}
                   | {0x03, 0x0B, 0x13, 0x1B, 0x23, 0x2B}
                   | {op for op in range(0x80, 0xC0) if op & 7 != 6}
                   | {0xC6 | (f << 3) for f in range(8)})

_R8 = ("b", "c", "d", "e", "h", "l", "[hl]", "a")
_R16 = ("bc", "de", "hl", "sp")
_ALU = ("add", "adc", "sub", "sbc", "and", "xor", "or", "cp")
_CB = ("rlc", "rrc", "rl", "rr", "sla", "sra", "swap", "srl")
_CC = ("nz", "z", "nc", "c")


def mnemonic(op: int, cb: bool = False) -> str:
    """A name for test ids (the ROM emits the opcode bytes themselves, not through the assembler)."""
    hi, mid, lo = op >> 6, (op >> 3) & 7, op & 7
    if cb:
        return f"{_CB[mid]} {_R8[lo]}" if hi == 0 else f"{('bit', 'res', 'set')[hi - 1]} {mid},{_R8[lo]}"
    if hi == 1:
        return f"ld {_R8[mid]},{_R8[lo]}"
    if hi == 2:
        return f"{_ALU[mid]} a,{_R8[lo]}"
    if hi == 0:
        if lo == 0:
            return {0: "nop", 1: "ld [nn],sp", 3: "jr e"}.get(mid) or f"jr {_CC[mid - 4]},e"
        if lo == 1:
            return f"add hl,{_R16[mid >> 1]}" if mid & 1 else f"ld {_R16[mid >> 1]},nn"
        if lo == 2:
            m = ("[bc]", "[de]", "[hl+]", "[hl-]")[mid >> 1]
            return f"ld a,{m}" if mid & 1 else f"ld {m},a"
        if lo == 3:
            return f"{'dec' if mid & 1 else 'inc'} {_R16[mid >> 1]}"
        if lo in (4, 5):
            return f"{'inc' if lo == 4 else 'dec'} {_R8[mid]}"
        if lo == 6:
            return f"ld {_R8[mid]},n"
        return ("rlca", "rrca", "rla", "rra", "daa", "cpl", "scf", "ccf")[mid]
    if lo == 0:
        return f"ret {_CC[mid]}" if mid < 4 else {4: "ldh [n],a", 5: "add sp,e", 6: "ldh a,[n]", 7: "ld hl,sp+e"}[mid]
    if lo == 1:
        return {1: "ret", 3: "reti", 5: "jp hl", 7: "ld sp,hl"}.get(mid) or f"pop {('bc', 'de', 'hl', 'af')[mid >> 1]}"
    if lo == 2:
        return f"jp {_CC[mid]},nn" if mid < 4 else {4: "ld [c],a", 5: "ld [nn],a", 6: "ld a,[c]", 7: "ld a,[nn]"}[mid]
    if lo == 3:
        return "jp nn"
    if lo == 4:
        return f"call {_CC[mid]},nn"
    if lo == 5:
        return "call nn" if op == 0xCD else f"push {('bc', 'de', 'hl', 'af')[mid >> 1]}"
    if lo == 6:
        return f"{_ALU[mid]} a,n"
    return f"rst {mid * 8:02x}h"


# ---- input vectors: (F, A, C, B, E, D, L, H) in the frame's order, then the eight scratch bytes ----
# the first eight are fixed: the edge values 00 FF 0F 10 7F 80 (and 01) rotated through the seven
# registers, so every register sees every one of them and the seven are pairwise distinct, then one
# vector with all registers equal ($80: results of zero); every combination of Z and C; scratch byte
# 4 (what POP AF loads into F) with a low nibble != 0.  The rest come from a seeded generator,
# registers pairwise distinct.
EDGES = (0x00, 0xFF, 0x0F, 0x10, 0x7F, 0x80, 0x01)
_FLAGS = (0x00, 0xF0, 0x80, 0x10, 0x90, 0x60, 0xA0, 0x50)
_SCRATCH = [
    (0x00, 0xFF, 0x0F, 0x10, 0x7F, 0x80, 0x01, 0xFE),
    (0xFF, 0x00, 0xF0, 0x0F, 0x8F, 0x7F, 0xFE, 0x01),
    (0x0F, 0x10, 0x00, 0xFF, 0x35, 0x0F, 0x80, 0x7F),
    (0x10, 0x0F, 0xFF, 0x00, 0xCA, 0xF0, 0x7F, 0x80),
    (0x7F, 0x80, 0x55, 0xAA, 0x1F, 0x00, 0xFF, 0x0F),
    (0x80, 0x7F, 0xAA, 0x55, 0xE1, 0xFF, 0x00, 0x10),
    (0x01, 0xFE, 0x00, 0x00, 0x0F, 0x00, 0x00, 0x00),
    (0xFE, 0x01, 0xFF, 0xFF, 0xF1, 0xFF, 0xFF, 0xFF),
]
_HAND = ([(_FLAGS[j], *(EDGES[(i + j) % 7] for i in range(7)), *_SCRATCH[j]) for j in range(7)]
         + [(_FLAGS[7], *([0x80] * 7), *_SCRATCH[7])])


def vectors(v: int, seed: int = 83) -> list[tuple[int, ...]]:
    if v < len(_HAND):
        raise ValueError(f"at least {len(_HAND)} vectors")
    rng = random.Random(seed)
    out = list(_HAND)
    while len(out) < v:
        regs = rng.sample(range(256), 7)
        out.append((rng.randrange(16) << 4, regs[0], *regs[1:], *(rng.randrange(256) for _ in range(8))))
    return out


# ---- blocks ----
class Block:
    """name: the test id; op: the opcode (0x100 | second byte for CB); fused: the path variant;
    pre: (pair, value or label) loads before the opcode; body: the lines from `.t:` on; head: lines
    in front of the entry (a backward JR's landing); k / group / high: index, group, bank half;
    entry / op_pc / out: addresses, filled in by matrix()."""

    def __init__(self, op, tag, fused, pre, body, head=()):
        self.op, self.fused, self.pre, self.body, self.head = op, fused, list(pre), list(body), list(head)
        cb = op >= 0x100
        self.name = (f"{'cb' if cb else ''}{op & 0xFF:02x} {mnemonic(op & 0xFF, cb)}{' ' + tag if tag else ''}"
                     f"-{'fused' if fused else 'primary'}").replace(" ", "_")
        self.k = self.group = self.high = self.entry = self.op_pc = self.out = None


def _imm(op: int) -> int:
    return (0x3B + op * 0x35) & 0xFF or 0x5C


def _variants(op: int):
    """(tag, pre, body lines, head lines) of base opcode op: usually one, more where one form
    is not enough (JR both ways, LDH / LD [C] inside and above the mirrored HRAM, SP + e both signs)."""
    hi, mid, lo = op >> 6, (op >> 3) & 7, op & 7
    plain = ["jp cap"]
    land = ["jp cap1", ".a: jp cap2"]
    hlmem = (hi == 1 and (lo == 6 or mid == 6)) or (hi == 2 and lo == 6) or op in (0x34, 0x35, 0x36)
    if op in (0x22, 0x2A):
        return [("", [("hl", W_SCR + 3)], [f"db ${op:02x}"] + plain, [])]        # $C0FF -> $C100
    if op in (0x32, 0x3A):
        return [("", [("hl", W_SCR + 4)], [f"db ${op:02x}"] + plain, [])]        # $C100 -> $C0FF
    if op in (0x02, 0x0A):
        return [("", [("bc", W_SCR + 1)], [f"db ${op:02x}"] + plain, [])]
    if op in (0x12, 0x1A):
        return [("", [("de", W_SCR + 6)], [f"db ${op:02x}"] + plain, [])]
    if op == 0x36:
        return [("", [("hl", W_SCR + 5)], [f"db $36, ${_imm(op):02x}"] + plain, [])]
    if hlmem:
        return [("", [("hl", W_SCR + 5)], [f"db ${op:02x}"] + plain, [])]
    if op == 0x08:
        return [("", [], [f"db $08, ${(W_SCR + 1) & 0xFF:02x}, ${(W_SCR + 1) >> 8:02x}"] + plain, [])]
    if op in (0xEA, 0xFA):
        return [("", [], [f"db ${op:02x}, ${(W_SCR + 7) & 0xFF:02x}, ${(W_SCR + 7) >> 8:02x}"] + plain, [])]
    if op in (0xE0, 0xF0):
        return [(t, [], [f"db ${op:02x}, ${n:02x}"] + plain, []) for t, n in (("lo", HRAM_LO), ("hi", HRAM_HI))]
    if op in (0xE2, 0xF2):
        return [(t, [("c", n)], [f"db ${op:02x}"] + plain, []) for t, n in (("lo", HRAM_LO), ("hi", HRAM_HI))]
    if op in (0xE8, 0xF8):
        return [(t, [("sp", 0xC0FB)], [f"db ${op:02x}, ${e:02x}"] + plain, []) for t, e in (("plus", 0x07), ("minus", 0xF9))]
    if op == 0x31:
        return [("", [], ["db $31, $fe, $c0"] + plain, [])]
    if hi == 0 and lo == 1 and not mid & 1:
        return [("", [], [f"db ${op:02x}, ${_imm(op):02x}, ${_imm(op + 1):02x}"] + plain, [])]
    if (hi == 0 and lo == 6) or (hi == 3 and lo == 6):
        return [("", [], [f"db ${op:02x}, ${_imm(op):02x}"] + plain, [])]
    if op == 0x18 or (hi == 0 and lo == 0 and mid >= 4):
        return [("fwd", [], [f"db ${op:02x}, .a - .t - 2"] + land, []),
                ("back", [], [f"db ${op:02x}, .a - .t - 2", "jp cap1"], [".a: jp cap2"])]
    if op == 0xC3 or (hi == 3 and lo == 2 and mid < 4) or op == 0xCD or (hi == 3 and lo == 4 and mid < 4):
        return [("", [], [f"db ${op:02x}", "dw .a"] + land, [])]
    if op in (0xC9, 0xD9) or (hi == 3 and lo == 0 and mid < 4):
        return [("", [("sp", ".ptr")], [f"db ${op:02x}"] + land + [".ptr: dw .a"], [])]
    if op == 0xE9:
        return [("", [("hl", ".a")], ["db $e9"] + land, [])]
    return [("", [], [f"db ${op:02x}"] + plain, [])]


def blocks() -> list[Block]:
    out = []
    for op in range(256):
        if op in ILLEGAL or op in OUT_OF_SCOPE or op == 0xCB:
            continue
        for fused in ((False, True) if op in FUSED_OPS else (False,)):
            out += [Block(op, tag, fused, pre, body, head) for tag, pre, body, head in _variants(op)]
    for cb in range(256):
        pre = [("hl", W_SCR + 5)] if cb & 7 == 6 else []
        out.append(Block(0x100 | cb, "", False, pre, [f"db $cb, ${cb:02x}", "jp cap"]))
    for k, b in enumerate(out):
        b.k, b.group, b.high, b.out = k, k % 8, (k // 8) % 2 == 1, W_OUT + 2 * k
    return out


def _block_source(b: Block) -> list[str]:
    L = [f"b{b.k}:"] + b.head + [".e:"]
    if not any(p == "sp" for p, _ in b.pre):
        L.append(f"ld sp, ${TEST_SP:04x}")
    for p, v in b.pre:
        L.append(f"ld {p}, {v if isinstance(v, str) else f'${v:04x}' if len(p) == 2 else f'${v:02x}'}")
    L += ["jp .p", ".p: nop"] if b.fused else ["jp .t"]
    body = list(b.body)
    body[0] = ".t: " + body[0]
    return L + body


class Matrix:
    """rom; blocks (with entry / op_pc / out filled in); vectors; caps {address: marker or None};
    bank: the ROM bank mapped at $4000-$7FFF while the blocks run; n_banks; fetch(addr) reads it."""

    def fetch(self, a: int) -> int:
        return self.rom[a] if a < 0x4000 else self.rom[self.bank * 0x4000 + a - 0x4000]


def matrix(n_banks: int = 2, vectors_n: int = 13) -> Matrix:
    if n_banks not in (2, 64):
        raise ValueError("n_banks: 2 or 64")
    # A wrong selector changes the same hashed byte by the same amount d in every vector; the hash
    # then moves by d * sum of 2^(5 * HASHED * v mod 16) (mod 2^16 - 1, up to carries), which is 0 for
    # every d when the sum is 0xFFFF (V = 16).  Only a V whose sum is invertible is accepted.
    mult = sum(1 << (5 * HASHED * v) % 16 for v in range(vectors_n))
    if math.gcd(mult, 0xFFFF) != 1:
        raise ValueError(f"{vectors_n} vectors: a constant difference can cancel in the hash (try 13, 15 or 17)")
    bank = 1 if n_banks == 2 else HIGH_BANK
    vs, bs = vectors(vectors_n), blocks()
    L = [f"wS1 equ ${W_S1:04x}", f"wS2 equ ${W_S2:04x}", "section 0"]
    for n in range(8):   # RST stubs: marker $10 + n, every register kept (AF through the test stack)
        L += [f"org ${8 * n:04x}", "push af", f"ld a, ${MARK_RST + n:02x}", f"ld [${W_MARK:04x}], a", "pop af", "ret"]
    for a in (0x40, 0x48, 0x50, 0x58, 0x60):
        L += [f"org ${a:04x}", "reti"]
    L += ["org $0100", "nop", "jp start", "org $0150",
          "start:", "di", "ld sp, $dff0", "xor a", "ldh [$ff], a", f"ld [${W_DONE:04x}], a", f"ld [${W_GIDX:04x}], a",
          f"ld a, {bank}", "ld [$2000], a",
          # the pressed button's JOYP bit, as kat.py
          "ld a, $20", "ldh [$00], a", "ldh a, [$00]", "ldh a, [$00]", "cpl", "and $0f", "ld b, a",
          "ld a, $10", "ldh [$00], a", "ldh a, [$00]", "ldh a, [$00]", "cpl", "and $0f", "swap a", "or b",
          f"ld [${W_GRP:04x}], a",
          "next_group:", f"ld a, [${W_GIDX:04x}]", "cp 8", "jp z, finished", "inc a", f"ld [${W_GIDX:04x}], a",
          "ld b, a", "ld a, $80", ".r:", "rlca", "dec b", "jr nz, .r",            # a = 1 << group
          "ld b, a", f"ld a, [${W_GRP:04x}]", "and a", "jr z, .do", "and b", "jr z, next_group",
          ".do:", f"ld a, [${W_GIDX:04x}]", "dec a", "add a, a", "ld l, a", "ld h, 0", "ld de, gtab", "add hl, de",
          "ld a, [hl+]", "ld h, [hl]", "ld l, a",
          "store_list:", "ld a, l", f"ld [${W_LIST:04x}], a", "ld a, h", f"ld [${W_LIST + 1:04x}], a",
          # next block of the list: entry address (0 ends the list), output address
          "next_block:", f"ld a, [${W_LIST:04x}]", "ld l, a", f"ld a, [${W_LIST + 1:04x}]", "ld h, a",
          "ld a, [hl+]", "ld e, a", "ld a, [hl+]", "ld d, a", "or e", "jp z, next_group",
          "ld a, e", f"ld [${W_ENTRY:04x}], a", "ld a, d", f"ld [${W_ENTRY + 1:04x}], a",
          "ld a, [hl+]", f"ld [${W_OUTP:04x}], a", "ld a, [hl+]", f"ld [${W_OUTP + 1:04x}], a",
          "ld a, l", f"ld [${W_LIST:04x}], a", "ld a, h", f"ld [${W_LIST + 1:04x}], a",
          "xor a", "ld [wS1], a", "ld [wS2], a", f"ld [${W_VEC:04x}], a",
          # vector wVec: registers into the frame, scratch bytes into the window and HRAM, marker 0
          "vloop:", f"ld a, [${W_VEC:04x}]", "swap a", "ld l, a", "and $0f", "ld h, a", "ld a, l", "and $f0", "ld l, a",
          "ld de, vtab", "add hl, de",
          f"ld de, ${W_REGS:04x}", "ld b, 8", ".c1:", "ld a, [hl+]", "ld [de], a", "inc de", "dec b", "jr nz, .c1",
          f"ld de, ${W_SCR:04x}", "ld b, 8", ".c2:", "ld a, [hl+]", "ld [de], a", "inc de", "dec b", "jr nz, .c2",
          f"ld a, [${W_SCR:04x}]", f"ldh [${HRAM_LO:02x}], a", f"ld a, [${W_SCR + 1:04x}]", f"ldh [${HRAM_HI:02x}], a",
          "xor a", f"ld [${W_MARK:04x}], a",
          f"ld sp, ${W_REGS:04x}", "pop af", "pop bc", "pop de", "pop hl", "ret",     # ret: into the block
          "finished:", "ld a, 1", f"ld [${W_DONE:04x}], a", "spin:", "jr spin"]
    save = [f"ld [${W_SAVESP:04x}], sp", f"ld sp, ${W_SAVE + 8:04x}", "push af", "push bc", "push de", "push hl",
            "ld sp, $dff0"]
    L += (["cap1:"] + save + [f"ld a, ${MARK_FELL:02x}", "jr capm"]
          + ["cap2:"] + save + [f"ld a, ${MARK_LANDED:02x}", "jr capm"]
          + ["cap:"] + save + ["jr caph"]
          + ["capm:", f"ld [${W_MARK:04x}], a",
             "caph:", f"ldh a, [${HRAM_LO:02x}]", f"ld [${W_H0:04x}], a", f"ldh a, [${HRAM_HI:02x}]", f"ld [${W_H1:04x}], a",
             f"ld hl, ${W_SAVE:04x}", f"ld b, {HASHED}", ".h:", "ld a, [hl+]", "call acc1", "dec b", "jr nz, .h",
             f"ld a, [${W_VEC:04x}]", "inc a", f"ld [${W_VEC:04x}], a", f"cp {len(vs)}", "jp nz, vloop",
             f"ld a, [${W_OUTP:04x}]", "ld l, a", f"ld a, [${W_OUTP + 1:04x}]", "ld h, a",
             "ld a, [wS1]", "ld [hl+], a", "ld a, [wS2]", "ld [hl], a", "jp next_block",
             # kat.py's acc1: h = rotl16(h, 5) + a over wS2:wS1 (bc, de, hl kept)
             "acc1:", "push bc", "push hl", "ld c, a", "ld a, [wS1]", "ld l, a", "ld a, [wS2]", "ld h, a"]
          + ["add hl, hl", "ld a, l", "adc a, 0", "ld l, a"] * 5
          + ["ld b, 0", "add hl, bc", "ld a, l", "ld [wS1], a", "ld a, h", "ld [wS2], a", "pop hl", "pop bc", "ret"])
    L += ["vtab:"] + ["db " + ", ".join(f"${x:02x}" for x in v) for v in vs]
    L += ["gtab:", "dw " + ", ".join(f"glist{g}" for g in range(8))]
    for g in range(8):
        L += [f"glist{g}:"] + [f"dw b{b.k}.e, ${b.out:04x}" for b in bs if b.group == g] + ["dw 0"]
    for b in bs:
        if not b.high:
            L += _block_source(b)
    L += [f"section {bank}", "org $4000"]
    for b in bs:
        if b.high:
            L += _block_source(b)
    m = Matrix()
    m.rom = build_rom("\n".join(L), n_banks=n_banks, title="SM83MATRIX")
    sym = build_rom.symbols
    for b in bs:
        b.entry, b.op_pc = sym[f"b{b.k}.e"], sym[f"b{b.k}.t"]
    m.blocks, m.vectors, m.bank, m.n_banks = bs, vs, bank, n_banks
    m.caps = {sym["cap"]: None, sym["cap1"]: MARK_FELL, sym["cap2"]: MARK_LANDED}
    return m


def kat_matrix_rom(n_banks: int = 2, vectors: int = 13) -> bytes:
    return matrix(n_banks, vectors).rom
