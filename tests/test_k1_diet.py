"""K1's fused-pair decision from the carried pav value (pk_step.hip: pav_at, PK_PF_TAIL) against
the oracle: whole v9 state and screen, on the CPU through the host simulation (16 and 32 envs per
wave, 2- and 64-bank cartridges) and, marked gpu, through both gfx950 kernels.

pav says how many fetched bytes an instruction pair may take where the code lives and whether a
write can change that code; pav_edge_rom below runs code across every boundary it encodes:
  * the end of ROM bank 0 (0x3FF8-0x3FFF, seven entry points): pairs ending 3, 2 and 1 bytes before
    the bank end and exactly at it, and an instruction at 0x3FFF whose successor lies in the
    switchable bank — alternately bank 1 and another bank whose first bytes differ, so a pair that
    read on past the bank end (the LDS slot behind bank 0) would take the wrong bank's bytes;
  * the end of the switchable bank (0x7FF6-0x7FFF): a 2 + 2 byte pair ending 3 bytes before the end
    and a pair in the last three bytes;
  * WRAM code: a 2 + 2 byte pair (RAM code has 3 bytes: the successor's immediate is not fetched),
    and a primary that stores A into the immediate of its fusable successor (the fetched bytes are
    stale: must not fuse), followed by a pair that may fuse;
  * HRAM code at 0xFF80 (the LDS mirror's first bytes), at 0xFF98-0xFF9F (its last rows: the last
    fetches leave the mirror) and a storing primary with a fusable successor at 0xFF88.
Every pass feeds the joypad and a pass counter into the registers, so stale bytes change the state."""
import numpy as np
import pytest

from pokegym_amd.testrom.fuzz import fuzz_rom, hram_code_rom, io_edge_rom, irq_bank_rom
from pokegym_amd.testrom.sm83asm import build_rom

LOOP = "$04, $78, $81, $4f, $15, $20, $f9, $c9"   # inc b; ld a,b; add a,c; ld c,a; dec d; jr nz,-7; ret
# 0xFF88: ldh [$8b],a (the next instruction's immediate); ld c,N; add a,c; ret
HSTORE = "$e0, $8b, $0e, $00, $81, $c9"
# 0xD000: ld b,$12; add a,$34 | ld hl,$d009; ld [hl],a; ld c,N (N at 0xD009); add a,c; inc b; ret
WCODE = "$06, $12, $c6, $34, $21, $09, $d0, $77, $0e, $00, $81, $04, $c9"


def pav_edge_rom(n_banks: int = 2) -> bytes:
    other = min(5, n_banks - 1)
    L = ["section 0", "org $0040", "reti", "org $0048", "reti", "org $0050", "reti", "org $0058", "reti",
         "org $0060", "reti", "org $0100", "nop", "jp start", "org $0150",
         "start:", "di", "ld sp, $dff0", "xor a", "ld [$c010], a"]
    for src, dst, n in (("r_loop", 0xFF80, 8), ("r_hstore", 0xFF88, 6), ("r_loop", 0xFF98, 8), ("r_wcode", 0xD000, 13)):
        lbl = f"cp_{dst:04x}"
        L += [f"ld hl, {src}", f"ld de, ${dst:04x}", f"ld b, {n}", f"{lbl}:", "ld a, [hl+]", "ld [de], a", "inc de",
              "dec b", f"jr nz, {lbl}"]
    L += ["ld a, $e3", "ldh [$40], a", "ld bc, $0102", "ld de, $0304",
          "main:",
          "ld a, $10", "ldh [$00], a", "ldh a, [$00]", "ldh a, [$00]", "add a, c", "ld e, a",
          "ld hl, $c010", "inc [hl]", "add a, [hl]",
          "call $d000",
          "ld d, 3", "call $ff80", "call $ff88", "ld d, 2", "call $ff98",
          # the switchable bank for this pass: bank 1 or the other one
          "ld a, [$c010]", "and $01", "jr z, .b1", f"ld a, ${other:02x}", "jr .set", ".b1:", "ld a, $01", ".set:",
          "ld [$2100], a", "ld a, e"]
    for entry in (0x3FF8, 0x3FFA, 0x3FFB, 0x3FFC, 0x3FFD, 0x3FFE, 0x3FFF):
        L += [f"call ${entry:04x}"]
    L += ["call $7ff6",
          "ld hl, $c000", "ld [hl+], a", "ld a, b", "ld [hl+], a", "ld a, c", "ld [hl+], a", "ld a, d", "ld [hl+], a",
          "jp main",
          "r_loop:", f"db {LOOP}", "r_hstore:", f"db {HSTORE}", "r_wcode:", f"db {WCODE}",
          # the end of bank 0: execution runs on into the switchable bank at 0x4000
          "org $3ff8", "ld a, $21", "inc b", "add a, b", "inc c", "xor c", "inc d", "add a, d"]
    for b in sorted({1, other}):
        L += [f"section {b}", "org $4000", f"add a, ${0xB0 + b:02x}" if b == 1 else f"sub ${b:02x}", "ld c, a", "ret",
              "org $7ff6", "ld a, $33", "add a, b", f"ld b, ${b:02x}", "add a, $44", "inc c", "add a, c", "ret"]
    return build_rom("\n".join(L), n_banks=n_banks, title="PAVEDGE")


ROMS = {
    "fuzz3": lambda nb: fuzz_rom(3, n_banks=nb),
    "fuzz21": lambda nb: fuzz_rom(21, n_banks=nb),
    "hram_code": hram_code_rom,
    "irq_bank": irq_bank_rom,
    "io_edges": io_edge_rom,
    "pav_edge": pav_edge_rom,
}
_roms = {}


def _rom(name, n_banks):
    if (name, n_banks) not in _roms:
        _roms[name, n_banks] = ROMS[name](n_banks)
    return _roms[name, n_banks]


def test_pav_edge_rom_layout():
    """The generator's code sits where the cases above say (the assembler placed what was meant)."""
    for nb in (2, 64):
        rom = pav_edge_rom(nb)
        other = min(5, nb - 1)
        assert rom[0x3FF8:0x4000] == bytes([0x3E, 0x21, 0x04, 0x80, 0x0C, 0xA9, 0x14, 0x82])
        assert rom[0x4000:0x4004] == bytes([0xC6, 0xB1, 0x4F, 0xC9])
        assert rom[0x4000 + 0x3FF6:0x8000] == bytes([0x3E, 0x33, 0x80, 0x06, 0x01, 0xC6, 0x44, 0x0C, 0x81, 0xC9])
        if other != 1:
            assert rom[other * 0x4000:other * 0x4000 + 4] == bytes([0xD6, other, 0x4F, 0xC9])


@pytest.mark.parametrize("lanes", ["16", "32"])
@pytest.mark.parametrize("n_banks", [2, 64])
@pytest.mark.parametrize("name", sorted(ROMS))
def test_hostsim_diet(name, n_banks, lanes, monkeypatch):
    """8 envs, 2 env-steps in the host simulation (pk_check_lane's pav invariant at every loop top)."""
    from tests.hostsim.check import check
    monkeypatch.setenv("PK_WAVE_LANES", lanes)
    assert check(_rom(name, n_banks), 8, 2, 7) == []


def test_hostsim_pav_edge_fuses_at_the_bank_end():
    """The pairs the cases are about did fuse: the host simulation's trace holds fused successors
    (record type 0x2000) at 0x3FFC, 0x3FFD, 0x3FFE and 0x3FFF, at 0x7FFB and 0x7FFE, in WRAM at
    0xD00B and in HRAM — and none where the bytes are missing or stale (0xD002, 0xD008, 0xFF8A,
    0x4000)."""
    import ctypes
    from tests.hostsim import sim
    from tests.hostsim.sim import SimEmulator
    rom = _rom("pav_edge", 64)
    L = sim.lib()
    L.pk_sim_trace_enable.argtypes = [ctypes.c_uint32, ctypes.c_uint64]
    L.pk_sim_trace_get.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
    L.pk_sim_trace_get.restype = ctypes.c_uint64
    cap = 1 << 21
    L.pk_sim_trace_enable(0, cap)
    emu = SimEmulator(rom, 1)
    emu.step(np.array([2], np.uint8))
    buf = np.zeros((cap, 6), np.uint32)
    k = L.pk_sim_trace_get(buf.ctypes.data, cap)
    L.pk_sim_trace_enable(0xFFFFFFFF, 0)
    emu.close()
    assert k < cap
    rec = buf[:k]                                   # pc, w0, w1, sp, op, 0
    fused = set(rec[(rec[:, 4] & 0x3000) == 0x2000][:, 0].tolist())
    for pc in (0x3FFC, 0x3FFD, 0x3FFE, 0x3FFF, 0x7FFB, 0x7FFE, 0xD00B, 0xFF81, 0xFF99):
        assert pc in fused, hex(pc)
    for pc in (0xD002, 0xD008, 0xFF8A, 0x4000):
        assert pc not in fused, hex(pc)


@pytest.mark.gpu
@pytest.mark.parametrize("small", [False, True])
def test_gpu_diet(small, monkeypatch):
    """The same ROMs through pk_step_kernel and pk_step_kernel_small: 64 envs, 2 env-steps."""
    import torch
    from oracle import oracle
    from pokegym_amd.emulator import BatchedEmulator
    if small:
        monkeypatch.setenv("PK_K1_SMALL", "1")
        monkeypatch.setenv("PK_WAVE_LANES", "32")
        monkeypatch.setenv("PK_K1_BLOCK", "256")
    n, steps = 64, 2
    actions = np.random.default_rng(7).integers(0, 9, size=(steps, n), dtype=np.uint8)
    for name in sorted(ROMS):
        for nb in (2, 64):
            rom = _rom(name, nb)
            emu = BatchedEmulator(rom, n)
            for s in range(steps):
                emu.step(torch.from_numpy(actions[s]).to(emu.device))
            torch.cuda.synchronize()
            gpu = [emu.snapshot(e) for e in range(n)]
            emu.close()
            ref, _ = oracle.batch_run(rom, None, actions, want_screens=False)
            bad = [e for e in range(n) if gpu[e] != ref[e].tobytes()]
            assert not bad, (name, nb, bad[:8])
