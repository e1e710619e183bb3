"""The stage ROM: labelled fragments that tests/state_cases.py points PC at — TEST INFRASTRUCTURE.

One cartridge, built at 2, 8 and 64 banks.  Nothing here reads the joypad: a case sets the registers
a fragment takes its parameters from and starts the CPU at the fragment's label, from an LCD phase
an oracle stopped mid-frame at (`boot` spins so that the oracle can be stopped anywhere).

Bank 0
  0000            nop / nop / jp landing (PC wrapping through IE lands here)
  0040..0060      the five interrupt vectors, each `jp` to its handler
  landing         sums WRAM C000-C0FF into DFF0, counts its passes in DFF1, for ever; it uses A, B,
                  HL and F, so a fragment's result must end in C, D, E, SP or memory
  h0..h4          handlers: count in C010+8k, then LY STAT DIV TIMA IF as read on entry, reti
  boot            `jr boot`
  copy_a / copy_b CopyData and its B/C twin; poll_N the LY poll for each N of POLL_NS;
  dec_rom         dec a / jr nz,-3 — each followed by jp landing
  probe           24 passes: LY STAT DIV TIMA IF into the ring C100..; on pass B writes register
                  PROBE_REGS[D & 7] with C (LCDC: toggles bit 7)
  s_halt, s_ei_halt, s_ei_di, s_ei_ret, s_di_halt    the HALT and IME sites
  mbc             writes E to address D << 8 (D in 00..7F), then reads 4000 7FFF A000 BFFF into
                  C0E0..C0E3
  dma             OAM DMA from page A, then the 40-pass wait loop
  bank-0 end      2 banks: copy_a at 3FF8 (ends with the bank); 8 banks: the fetch seam 3FFD
                  (inc a / ld de,nn at 3FFE / ld c,n at 3FFF: a 3-byte and a 2-byte instruction
                  across 3FFF|4000); 64 banks: poll_144 at 3FFA (ends with the bank)
Every switchable bank b
  4000            ld c,r (48 + b % 6: differs between neighbours), 4001 jp landing; bank 2 of the 8-
                  and 64-bank ROMs: F8 00 (ld hl,sp+0), jp landing
  4100..          the same loop fragments as bank 0 (SW[...] offsets)
  bank end        per bank (END_FRAGMENTS): loops ending at, and one byte past, the offsets K1 tests,
                  `halt` as the bank's last byte in the last bank, the 7FFF|8000 fetch seam
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

from pokegym_amd.testrom.sm83asm import build_rom

POLL_NS = (0, 1, 2, 142, 143, 144, 145, 152, 153, 154, 200)
PROBE_REGS = (0x41, 0x45, 0x40, 0x07, 0x05, 0x04, 0x0F, 0xFF)   # STAT LYC LCDC TAC TIMA DIV IF IE
PROBE_PASSES = 24
COPY_A = bytes([0x2A, 0x12, 0x13, 0x0B, 0x79, 0xB0, 0x20, 0xF8])
COPY_B = bytes([0x2A, 0x12, 0x13, 0x0B, 0x78, 0xB1, 0x20, 0xF8])
DEC = bytes([0x3D, 0x20, 0xFD])
W_SUM, W_PASSES, W_MBC, W_RING, W_HAND = 0xDFF0, 0xDFF1, 0xC0E0, 0xC100, 0xC010


def poll(n: int) -> bytes:
    return bytes([0xF0, 0x44, 0xFE, n & 0xFF, 0x20, 0xFA])


def _src() -> str:
    polls = "\n".join(f"poll_{n}:\n    db $F0,$44,$FE,{n},$20,$FA\n    jp landing" for n in POLL_NS)
    hand = "\n".join(f"""
h{k}:
    push af
    push hl
    ld hl, {W_HAND + 8 * k}
    inc [hl]
    inc hl
    ldh a, [$44]
    ld [hl+], a
    ldh a, [$41]
    ld [hl+], a
    ldh a, [$04]
    ld [hl+], a
    ldh a, [$05]
    ld [hl+], a
    ldh a, [$0F]
    ld [hl+], a
    pop hl
    pop af
    reti""" for k in range(5))
    vecs = "\n".join(f"    org ${0x40 + 8 * k:04X}\n    jp h{k}" for k in range(5))
    return f"""
section 0
    org $0000
    nop
    nop
    jp landing
{vecs}
    org $0068
landing:
    ld hl, $C000
    ld b, 0
.l:
    ld a, [hl]
    add a, b
    ld b, a
    inc l
    jr nz, .l
    ld a, b
    ld [{W_SUM}], a
    ld hl, {W_PASSES}
    inc [hl]
    jr landing
    org $0100
    nop
    jp boot
    org $0150
boot:
    jr boot
copy_a:
    db $2A,$12,$13,$0B,$79,$B0,$20,$F8
    jp landing
copy_b:
    db $2A,$12,$13,$0B,$78,$B1,$20,$F8
    jp landing
dec_rom:
    db $3D,$20,$FD
    jp landing
{polls}
probe:
    ld hl, {W_RING}
    ld e, 0
.pass:
    ldh a, [$44]
    ld [hl], a
    inc l
    ldh a, [$41]
    ld [hl], a
    inc l
    ldh a, [$04]
    ld [hl], a
    inc l
    ldh a, [$05]
    ld [hl], a
    inc l
    ldh a, [$0F]
    ld [hl], a
    inc l
    ld a, e
    cp b
    jr nz, .next
    ld a, d
    and 7
    cp 2
    jr nz, .reg
    ldh a, [$40]
    xor $80
    ldh [$40], a
    jr .next
.reg:
    push bc
    push hl
    ld hl, probe_regs
    add a, l
    ld l, a
    ld a, [hl]
    ld b, c
    ld c, a
    ld a, b
    ldh [c], a
    pop hl
    pop bc
.next:
    inc e
    ld a, e
    cp {PROBE_PASSES}
    jr nz, .pass
    jp landing
    org $0300
probe_regs:
    db {", ".join(str(r) for r in PROBE_REGS)}
s_halt:
    halt
    inc c
    jp landing
s_ei_halt:
    ei
    halt
    inc c
    jp landing
s_ei_di:
    ei
    di
    inc c
    jp landing
s_ei_ret:
    ei
    ret
s_di_halt:
    di
    halt
    inc c
    jp landing
mbc:
    ld h, d
    ld l, 0
    ld [hl], e
    ld a, [$4000]
    ld [{W_MBC}], a
    ld a, [$7FFF]
    ld [{W_MBC + 1}], a
    ld a, [$A000]
    ld [{W_MBC + 2}], a
    ld a, [$BFFF]
    ld [{W_MBC + 3}], a
    jp landing
dma:
    ldh [$46], a
    ld a, $28
.w:
    dec a
    jr nz, .w
    jp landing
{hand}
section 1
    org $4000
    db $49
    jp landing
    org $4100
sw_copy_a:
    db $2A,$12,$13,$0B,$79,$B0,$20,$F8
    jp landing
sw_copy_b:
    db $2A,$12,$13,$0B,$78,$B1,$20,$F8
    jp landing
sw_dec:
    db $3D,$20,$FD
    jp landing
sw_poll_144:
    db $F0,$44,$FE,144,$20,$FA
    jp landing
sw_poll_200:
    db $F0,$44,$FE,200,$20,$FA
    jp landing
sw_halt:
    halt
    inc c
    jp landing
"""


# what the end of switchable bank b holds, 8 and 64 banks: (offset in the bank, bytes)
END_FRAGMENTS = {
    1: (0x3FF9, COPY_A),          # one byte past: its last byte is VRAM 8000
    2: (0x3FFA, poll(144)),       # ends with the bank
    3: (0x3FFB, poll(144)),       # one byte past
    4: (0x3FF8, COPY_B),          # ends with the bank
    5: (0x3FFD, DEC),             # ends with the bank
    6: (0x3FF8, COPY_A),          # ends with the bank; 8 and 64 banks: a bank K1 does not stage
}
SEAM = bytes([0x3C, 0x11, 0x0E])   # inc a / ld de,nn (3 bytes from xFFE) / ld c,n (2 bytes from xFFF)
SEAM_BANK = 8                      # 64 banks: the 7FFF|8000 seam's bank


@functools.lru_cache(maxsize=None)
def stage_rom(n_banks: int = 2) -> SimpleNamespace:
    """rom (bytes), sym (label -> address), hi (the last bank: `halt` is its last byte; 8 and 64
    banks: not staged by K1), n_banks."""
    assert n_banks in (2, 8, 64)
    rom = bytearray(build_rom(_src(), n_banks, title="PKSTAGE"))
    sym = dict(build_rom.symbols)
    hi = n_banks - 1
    bank1 = bytes(rom[0x4000:0x8000])
    for b in range(1, n_banks):
        o = b * 0x4000
        rom[o:o + 0x4000] = bank1
        rom[o] = 0x48 + b % 6
        rom[o + 0x3FFF] = b ^ 0xA5
        if n_banks > 2 and b in END_FRAGMENTS:
            off, code = END_FRAGMENTS[b]
            rom[o + off:o + 0x4000] = code[:0x4000 - off]
    rom[hi * 0x4000 + 0x3FFF] = 0x76
    if n_banks > 2:
        # bank 2 begins with F8 (ld hl,sp+0 / jp landing): K1 stages it in the LDS slot behind bank
        # 1's, so a copy-loop test that read past bank 1's end would find the loop's last byte there
        rom[2 * 0x4000:2 * 0x4000 + 5] = bytes([0xF8, 0x00, 0xC3, sym["landing"] & 0xFF, sym["landing"] >> 8])
    if n_banks == 64:
        rom[SEAM_BANK * 0x4000 + 0x3FFD:SEAM_BANK * 0x4000 + 0x4000] = SEAM
    end0 = {2: (0x3FF8, COPY_A), 8: (0x3FFD, SEAM), 64: (0x3FFA, poll(144))}[n_banks]
    rom[end0[0]:0x4000] = end0[1]
    return SimpleNamespace(rom=bytes(rom), sym=sym, hi=hi, n_banks=n_banks)
