"""K1's re-encoded flag units and right-shift / SWAP unit (pk_step.hip pk_exec "flags" and "right-shift
unit", the fused-secondary-op block; pk_ucode.h K / U / CI words and the in-place secondary masks)
and its address unit against the oracle: whole v9 state and screen, on the CPU through the host
simulation (16 and 32 envs per wave, 2- and 64-bank cartridges) and, marked gpu, through both gfx950
kernels at the smallest shapes that reach them (64 envs: the small-LDS kernel with 16- and 32-env
waves, the 512-thread kernel).  2 env-steps = 48 frames.

addr_edge_rom: every pass mixes the joypad and a pass counter into the operands and
  * reads and writes one byte on both sides of every region boundary with ld a,[hl+] / ld [hl-],a
    (0x7FFF/0x8000, 0x9FFF/0xA000, 0xBFFF/0xC000, 0xDFFF/0xE000, 0xFDFF/0xFE00, 0xFE9F/0xFEA0,
    0xFEFF/0xFF00, 0xFF7F/0xFF80, 0xFFFE/0xFFFF) and a plain 512-byte block boundary in WRAM
    (0xC1FF/0xC200), with the cartridge RAM enabled on odd passes;
  * takes two-byte accesses across them in both directions: push / pop / call / ret with SP = 0x8001,
    0xA001, 0xC001, 0xC201, 0xE001, 0xFE01, 0xFF01, 0xFF81, 0xFF82 (pushes descend across the
    boundary, the pop reads back upward), pop with SP = 0xFFFD and 0xFFFE (reaching IE), and
    ld [nn],sp with nn one below each boundary;
  * ldh and ld [c] at 0xFF00, 0xFF7F, 0xFF80, 0xFFFE and 0xFFFF.
IE only ever receives values with its low five bits clear and interrupts stay disabled, so the run
has no dispatch; test_roms_run_clean checks the oracle does not reach its crash state.

flag_shift_rom: RRCA RRA, RRC RR SRA SRL SWAP on a register and on [hl], each with carry in 0 and 1;
POP AF with low-nibble garbage; ADD HL,rr, ADD SP,e, LD HL,SP+e; SCF CCF CPL; every kind of fusable
secondary op directly after a flag-setting primary and directly before a jr cc.  The whole block
runs twice per pass: in ROM, where the successors fuse, and copied to WRAM behind storing
primaries (ld [de],a before each probe's secondary op), where those may not (the same block with the
stores also runs from ROM, where a secondary op fuses behind a plain-RAM store)."""
import numpy as np
import pytest

from pokegym_amd.testrom.sm83asm import build_rom

HEAD = ["section 0", "org $0040", "reti", "org $0048", "reti", "org $0050", "reti", "org $0058", "reti",
        "org $0060", "reti", "org $0100", "nop", "jp start", "org $0150",
        "start:", "di", "ld sp, $dff0", "xor a", "ld [$c010], a", "ld a, $e3", "ldh [$40], a"]
# the pass's mix value in A (and E): joypad nibble + pass counter
MIX = ["ld a, $10", "ldh [$00], a", "ldh a, [$00]", "ldh a, [$00]", "ld hl, $c010", "inc [hl]", "add a, [hl]", "ld e, a"]

BOUNDS = (0x8000, 0xA000, 0xC000, 0xC200, 0xE000, 0xFE00, 0xFEA0, 0xFF00, 0xFF80, 0xFFFF)


def addr_edge_rom(n_banks: int = 2) -> bytes:
    L = HEAD + ["main:"] + MIX
    # cartridge RAM on odd passes (MBC3: 0x0A at 0x0000), RAM bank 0
    L += ["ld a, [$c010]", "and $01", "jr z, .off", "ld a, $0a", ".off:", "ld [$0000], a", "xor a", "ld [$4000], a", "ld a, e"]
    for k, b in enumerate(BOUNDS):
        # one-byte reads stepping up over the boundary, writes stepping down over it
        L += [f"ld hl, ${b - 1:04x}", "ld a, [hl+]", "add a, e", "ld d, a", "ld a, [hl+]", "xor d", "ld e, a"]
        if b == 0xFFFF:
            L += ["and $e0"]      # IE keeps its low five bits clear
        if b == 0xFF00:
            L += ["and $30"]      # the joypad select
        L += [f"ld hl, ${b:04x}", "ld [hl-], a", "inc a", "ld [hl-], a", "ld a, e"]
    # two-byte accesses: push then pop across the boundary, call / ret with SP there
    for k, sp in enumerate((0x8001, 0xA001, 0xC001, 0xC201, 0xE001, 0xFE01, 0xFF01, 0xFF81, 0xFF82)):
        L += [f"ld sp, ${sp:04x}", "ld b, e", "ld c, a", "push bc", "pop hl", "ld a, h", "xor l", "add a, e", "ld e, a",
              f"call f_ret{k}", "add a, e", "ld e, a"]
    for sp in (0xFFFD, 0xFFFE):
        L += [f"ld sp, ${sp:04x}", "pop bc", "ld a, b", "add a, c", "add a, e", "ld e, a"]
    # ld [nn],sp one below each boundary (SP's high byte has its low five bits clear: IE)
    for b in BOUNDS:
        L += ["ld h, $e0", "ld l, e", "ld sp, hl", f"ld [${b - 1:04x}], sp"]
    L += ["ld sp, $dff0"]
    for lo in (0x00, 0x7F, 0x80, 0xFE, 0xFF):
        L += [f"ld c, ${lo:02x}", "ld a, [c]", "add a, e", "ld e, a", f"ldh a, [${lo:02x}]", "xor e", "ld e, a"]
        L += ["and $e0" if lo == 0xFF else "and $30" if lo == 0x00 else "nop"]
        L += ["ld [c], a", "inc a" if lo not in (0xFF, 0x00) else "nop", f"ldh [${lo:02x}], a", "ld a, e"]
    L += ["ld hl, $c000", "ld [hl+], a", "ld a, b", "ld [hl+], a", "ld a, d", "ld [hl+], a", "jp main"]
    for k in range(9):
        L += [f"f_ret{k}:", "ld a, e", "rlca", "ret"]
    return build_rom("\n".join(L), n_banks=n_banks, title="ADDREDGE")


def _flag_block(store: bool) -> list:
    """The probes; store: a storing primary (ld [de],a, DE = 0xC020: it changes no flag) before each
    and, in the pairs, between the flag-setting primary and the secondary op — which then fuses
    behind a storing primary in ROM code and may not fuse in RAM code."""
    S = ["ld [de], a"] if store else []
    P = []

    def acc():   # fold A and the flags into B
        return ["push af", "pop hl", "ld a, l", "xor h", "add a, b", "ld b, a", "ld a, h"]

    for cy in ("scf", "and a"):                       # carry in 1, 0
        for op in ("rrca", "rra"):
            P += S + [cy, op] + acc()
        for op in ("rrc", "rr", "sra", "srl", "swap"):
            P += S + ["ld c, a", cy, f"{op} c", "ld a, c"] + acc()
            P += S + ["ld hl, $c030", "ld [hl], a", cy, f"{op} [hl]", "ld a, [hl]"] + acc()
    # POP AF with low-nibble garbage
    P += S + ["ld h, a", "ld l, $ff", "push hl", "pop af"] + acc()
    P += S + ["ld h, b", "ld l, $0f", "push hl", "pop af"] + acc()
    # 16-bit adds
    for rr in ("bc", "de", "hl", "sp"):
        P += S + ["ld h, a", "ld l, b", f"add hl, {rr}", "ld c, l"] + acc() + ["xor c"]
    for e in ("$7f", "$80", "$01", "$ff"):
        P += S + [f"ld hl, sp+{e}" if not e.startswith("$8") and e != "$ff" else f"ld hl, sp-{256 - int(e[1:], 16)}", "ld c, l"] + acc()
    P += S + ["add sp, $11"] + acc() + ["add sp, -$11"] + acc()
    for op in ("scf", "ccf", "cpl"):
        P += S + ["add a, b", op] + acc() + S + ["sub $35", op] + acc()
    # every kind of secondary op right after a flag-setting primary and right before a jr cc
    n = [0]

    def pair(prim, sec, cc):
        n[0] += 1
        lbl = f".s{int(store)}_{n[0]}"
        return [prim] + S + [sec, f"jr {cc}, {lbl}", "inc b", f"{lbl}:"] + acc()

    for prim in ("add a, b", "sub c", "and $3c", "cp b", "inc [hl]", "add hl, hl"):
        for sec, cc in (("inc c", "z"), ("dec c", "nz"), ("ld c, a", "c"), ("ld c, $55", "nc"), ("inc bc", "z"),
                        ("dec hl", "c"), ("add a, c", "c"), ("adc a, $0f", "nc"), ("sub b", "z"), ("sbc a, $81", "c"),
                        ("and c", "z"), ("xor $5a", "nz"), ("or b", "z"), ("cp $40", "c"), ("cpl", "nz"), ("scf", "nc"),
                        ("nop", "c")):
            P += ["ld hl, $c030"] + pair(prim, sec, cc)
    return P


def flag_shift_rom(n_banks: int = 2) -> bytes:
    L = HEAD + ["main:"] + MIX + ["ld b, a", "ld de, $c020", "call r_block"]
    # the same probes from WRAM behind storing primaries: copy, then run
    L += ["ld hl, w_block", "ld de, $d000", "ld bc, w_end - w_block", ".cp:", "ld a, [hl+]", "ld [de], a", "inc de", "dec bc",
          "ld a, b", "or c", "jr nz, .cp",
          "ld a, [$c010]", "ld b, a", "ld de, $c020", "call $d000",
          "ld a, [$c010]", "add a, b", "ld b, a", "ld de, $c020", "call s_block",
          "ld hl, $c000", "ld [hl], b", "jp main"]
    L += ["r_block:"] + _flag_block(False) + ["ret"]
    L += ["s_block:"] + [x.replace(".s1_", ".t1_") for x in _flag_block(True)] + ["ret"]
    L += ["w_block:"] + _flag_block(True) + ["ret", "w_end:"]
    return build_rom("\n".join(L), n_banks=n_banks, title="FLAGSHIFT")


ROMS = {"addr_edge": addr_edge_rom, "flag_shift": flag_shift_rom}
_roms = {}


def _rom(name, n_banks):
    if (name, n_banks) not in _roms:
        _roms[name, n_banks] = ROMS[name](n_banks)
    return _roms[name, n_banks]


@pytest.mark.parametrize("name", sorted(ROMS))
def test_roms_run_clean(name):
    """The oracle runs both ROMs for the test's 2 env-steps without reaching its crash state, and
    passes through the main loop (the pass counter at 0xC010 moves)."""
    from oracle import oracle
    g = oracle.GB(_rom(name, 2))
    g.power_on()
    for a in (2, 5):
        g.run_action(a)
    assert not g.crashed
    assert g.read(0xC010) > 2


@pytest.mark.parametrize("lanes", ["16", "32"])
@pytest.mark.parametrize("n_banks", [2, 64])
@pytest.mark.parametrize("name", sorted(ROMS))
def test_hostsim_diet3(name, n_banks, lanes, monkeypatch):
    """8 envs, 2 env-steps in the host simulation against the oracle."""
    from tests.hostsim.check import check
    monkeypatch.setenv("PK_WAVE_LANES", lanes)
    assert check(_rom(name, n_banks), 8, 2, 7) == []


def test_hostsim_flag_shift_fuses_where_it_may():
    """The pairing the ROM is about happened: the host simulation's trace holds every kind of fused
    successor (record type 0x2000) in the ROM blocks, also behind the storing primary ld [de],a,
    and in the WRAM copy none behind a storing primary."""
    import ctypes
    from tests.hostsim import sim
    from tests.hostsim.sim import SimEmulator
    L = sim.lib()
    L.pk_sim_trace_enable.argtypes = [ctypes.c_uint32, ctypes.c_uint64]
    L.pk_sim_trace_get.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
    L.pk_sim_trace_get.restype = ctypes.c_uint64
    cap = 1 << 22
    L.pk_sim_trace_enable(0, cap)
    emu = SimEmulator(_rom("flag_shift", 2), 1)
    emu.step(np.array([2], np.uint8))
    buf = np.zeros((cap, 6), np.uint32)
    k = L.pk_sim_trace_get(buf.ctypes.data, cap)
    L.pk_sim_trace_enable(0xFFFFFFFF, 0)
    emu.close()
    assert k < cap
    rec = buf[:k]
    fused = rec[(rec[:, 4] & 0x3000) == 0x2000]
    ops = set((fused[fused[:, 0] < 0x8000][:, 4] & 0xFF).tolist())
    # each kind of secondary op fused in ROM: INC/DEC r, LD r,r', LD r,n, INC/DEC rr, ALU r / n, CPL, SCF, NOP, JR cc
    for op in (0x0C, 0x0D, 0x4F, 0x0E, 0x03, 0x2B, 0x81, 0xCE, 0x90, 0xDE, 0xA1, 0xEE, 0xB0, 0xFE, 0x2F, 0x37, 0x00,
               0x20, 0x28, 0x30, 0x38):
        assert op in ops, hex(op)
    isf = (rec[:, 4] & 0x3000) == 0x2000
    prev_op = rec[:-1][isf[1:]][:, 4] & 0xFF                      # the primary of each fused record
    at = rec[1:][isf[1:]][:, 0]
    stores = np.isin(prev_op, [0x12, 0x77, 0x34, 0xE5, 0xF5, 0x22, 0x32])
    assert (stores & (at < 0x8000)).any()
    assert (at >= 0xD000).any() and not (stores & (at >= 0xD000)).any()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["small16", "small32", "wide512"])
def test_gpu_diet3(shape, monkeypatch):
    """Both ROMs, 2- and 64-bank, through pk_step_kernel_small (16- and 32-env waves) and the
    512-thread pk_step_kernel: 64 envs, 2 env-steps."""
    import torch
    from oracle import oracle
    from pokegym_amd.emulator import BatchedEmulator
    if shape.startswith("small"):
        monkeypatch.setenv("PK_K1_SMALL", "1")
        monkeypatch.setenv("PK_WAVE_LANES", shape[5:])
        monkeypatch.setenv("PK_K1_BLOCK", "256")
    else:
        monkeypatch.setenv("PK_K1_BLOCK", "512")
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
            scr = emu.screen.cpu().numpy()
            emu.close()
            ref, rscr = oracle.batch_run(rom, None, actions)
            bad = [e for e in range(n) if gpu[e] != ref[e].tobytes()]
            assert not bad, (name, nb, bad[:8])
            grey = np.array([0xFF, 0x99, 0x55, 0x00], np.uint8)
            assert np.array_equal(scr, grey[rscr]), (name, nb)
