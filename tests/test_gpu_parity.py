"""HIP kernel vs the CPU oracle, bit-exact on the whole machine state.

Every env's state after K env-steps is exported from the device as a PyBoy v9 savestate
(pk_snapshot) and compared byte-for-byte with the oracle's own v9 export (CPU registers, IME/HALT,
IE/IF, VRAM, OAM, LCD registers and clocks, per-line scroll params, the 144x160 screen, WRAM,
HRAM, IO, timer, MBC registers, cartridge SRAM)."""
import os

import numpy as np
import pytest

from oracle import oracle
from pokegym_amd.testrom.fuzz import fuzz_rom

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _diff(a: bytes, b: bytes):
    a = np.frombuffer(a, np.uint8)
    b = np.frombuffer(b, np.uint8)
    idx = np.nonzero(a != b)[0]
    return idx[:12].tolist()


def _run_both(rom, state, n, steps, seed, render=True):
    import torch
    from pokegym_amd.emulator import BatchedEmulator
    rng = np.random.default_rng(seed)
    actions = rng.integers(0, 9, size=(steps, n), dtype=np.uint8)
    emu = BatchedEmulator(rom, n, state=state, render=render)
    for s in range(steps):
        emu.step(torch.from_numpy(actions[s]).to(emu.device))
    torch.cuda.synchronize()
    gpu = [emu.snapshot(e) for e in range(n)]
    ref, _ = oracle.batch_run(rom, state, actions, want_screens=False)
    emu.close()
    return gpu, ref


@pytest.mark.parametrize("seed", [0, 1, 3, 4, 6, 8, 9, 11, 21, 33, 47, 58, 71])
def test_fuzz_rom_parity(seed):
    rom = fuzz_rom(seed)
    n, steps = 128, 12
    gpu, ref = _run_both(rom, None, n, steps, seed)
    bad = [(e, _diff(gpu[e], ref[e].tobytes())) for e in range(n) if gpu[e] != ref[e].tobytes()]
    assert not bad, bad[:4]


def test_region_seams_parity():
    """16-bit accesses across the RAM region seams (K1 takes them through the generic bus)."""
    from pokegym_amd.testrom.fuzz import boundary_rom
    n, steps = 64, 4
    gpu, ref = _run_both(boundary_rom(), None, n, steps, 9)
    bad = [(e, _diff(gpu[e], ref[e].tobytes())) for e in range(n) if gpu[e] != ref[e].tobytes()]
    assert not bad, bad[:4]


def test_bulbasaur_state_parity():
    """Start from the reference's Bulbasaur.state (Oak's lab) under a fuzz ROM."""
    st = open(os.path.join(os.path.dirname(GOLD), "..", "pokegym_amd", "states", "Bulbasaur.state"), "rb").read()
    rom = fuzz_rom(21)
    n, steps = 64, 10
    gpu, ref = _run_both(rom, st, n, steps, 5)
    bad = [(e, _diff(gpu[e], ref[e].tobytes())) for e in range(n) if gpu[e] != ref[e].tobytes()]
    assert not bad, bad[:4]


def test_load_snapshot_roundtrip():
    import torch
    from pokegym_amd.emulator import BatchedEmulator
    z = np.load(os.path.join(GOLD, "states.npz"))
    rom = fuzz_rom(2)
    emu = BatchedEmulator(rom, 70)
    for i, st in enumerate(z["states"]):
        emu.load_env(65 - i, st.tobytes())
    torch.cuda.synchronize()
    for i, st in enumerate(z["states"]):
        assert emu.snapshot(65 - i) == st.tobytes()
    emu.close()


@pytest.mark.parametrize("lanes", ["64", "32", "16", "4", "1"])
def test_game_rom_parity_wave_shapes(lanes, monkeypatch):
    """The pkbench game (HALT/VBlank frame loop, HRAM OAM-DMA routine, MBC3 banking, SRAM) under
    every K1 wave shape: 64, 32, 16, 4 or 1 envs per wave (PK_WAVE_LANES), with random actions."""
    from pokegym_amd.testrom.game import game_rom
    monkeypatch.setenv("PK_WAVE_LANES", lanes)
    rom = game_rom()
    n, steps = 96, 6
    gpu, ref = _run_both(rom, None, n, steps, 7)
    bad = [(e, _diff(gpu[e], ref[e].tobytes())) for e in range(n) if gpu[e] != ref[e].tobytes()]
    assert not bad, bad[:4]


# (lanes, render, seed): seed -1 = pkbench, else a fuzz ROM.  The shapes whole-handle launches take:
# 32-env waves (65,536-env handles, rendered; the 4,096-env headless config2 handle), 64-env waves
# (>= 131,072 envs), 16-env waves (32,768-env handles stepped whole); each over pkbench and fuzz ROMs.
WG512_CASES = [("16", True, -1), ("16", False, 21),
               ("32", True, -1), ("32", True, 0), ("32", False, 3), ("32", False, -1),
               ("64", True, 47), ("64", False, -1)]
# PK_PARITY_EXTENDED=1: the whole cross product (3 wave widths x rendered/headless x pkbench and four
# fuzz ROMs, 30 cases) — outside the driver's time-limited suite; one run of it on the final kernel is
# committed under profiles/ 
if os.environ.get("PK_PARITY_EXTENDED") == "1":
    WG512_CASES = [(lanes, render, seed) for lanes in ("16", "32", "64") for render in (True, False)
                   for seed in (-1, 0, 3, 21, 47)]


@pytest.mark.parametrize("lanes,render,seed", WG512_CASES)
def test_fuzz_rom_parity_512_thread_workgroups(seed, render, lanes, monkeypatch):
    """The benchmarked K1 shapes at small n: 512-thread workgroups (PK_K1_BLOCK), 8 waves sharing
    the workgroup's HRAM mirror — 16 envs per wave (configs[3]'s 32,768-env shard: columns up to
    127), 32 (configs[2]'s 65,536-env launch: columns up to 255) and 64 (launches of >= 131,072
    envs: columns up to 511); rendered and headless.  The wide
    shape also selects K1's wave-priority variant (pk_step_kernel<true>), as those launches do."""
    monkeypatch.setenv("PK_K1_BLOCK", "512")
    monkeypatch.setenv("PK_WAVE_LANES", lanes)
    from pokegym_amd.testrom.game import game_rom
    rom = game_rom() if seed < 0 else fuzz_rom(seed)
    n, steps = {"16": 256, "32": 256, "64": 1024}[lanes], 8
    gpu, ref = _run_both(rom, None, n, steps, 100 + seed, render=render)
    g = np.frombuffer(b"".join(gpu), np.uint8).reshape(n, -1)
    a = oracle.state_digests(g, headless=not render)
    b = oracle.state_digests(ref, headless=not render)
    bad = [(e, _diff(gpu[e], ref[e].tobytes())) for e in np.nonzero(a != b)[0][:4]]
    assert not bad, bad


@pytest.mark.parametrize("seed", [2, 13, 40])
@pytest.mark.parametrize("lanes", ["", "64"])
def test_fuzz_rom_parity_64_banks(seed, lanes, monkeypatch):
    """1 MiB fuzz cartridges: code and data in the 58 switchable banks K1 does not stage in LDS
    (global-ROM fetch and read paths); also under 512-thread workgroups of 64-env waves."""
    if lanes:
        monkeypatch.setenv("PK_K1_BLOCK", "512")
        monkeypatch.setenv("PK_WAVE_LANES", lanes)
    rom = fuzz_rom(seed, n_banks=64)
    n, steps = (128 if not lanes else 512), 12
    gpu, ref = _run_both(rom, None, n, steps, 200 + seed)
    bad = [(e, _diff(gpu[e], ref[e].tobytes())) for e in range(n) if gpu[e] != ref[e].tobytes()]
    assert not bad, bad[:4]


@pytest.mark.parametrize("render", [True, False])
def test_game_rom_64_banks_parity(render):
    """pkbench on the 64-bank layout (overworld engine in 60 switchable banks), 512 envs."""
    from pokegym_amd.testrom.game import game_rom
    rom = game_rom(64)
    n, steps = 512, 10
    gpu, ref = _run_both(rom, None, n, steps, 64, render=render)
    g = np.frombuffer(b"".join(gpu), np.uint8).reshape(n, -1)
    a = oracle.state_digests(g, headless=not render)
    b = oracle.state_digests(ref, headless=not render)
    bad = [(e, _diff(gpu[e], ref[e].tobytes())) for e in np.nonzero(a != b)[0][:4]]
    assert not bad, bad


@pytest.mark.parametrize("name", ["game", "lcdtoggle"])
def test_instr_count_parity(name):
    """pk_last_instr_count of the gfx950 build == the oracle's executed instructions per env-step
    (fused pairs, skipped CopyData / LY-poll passes; interrupt dispatch and idle iterations are not
    instructions), 256 envs of pkbench or the watchdog ROM."""
    import torch
    from pokegym_amd.emulator import BatchedEmulator
    from pokegym_amd.testrom.fuzz import lcd_toggle_rom
    from pokegym_amd.testrom.game import game_rom
    from tests import oracle_pool as OP
    rom = game_rom() if name == "game" else lcd_toggle_rom()
    n = 256 if name == "game" else 64
    acts = np.random.default_rng(6).integers(0, 9, size=(3, n), dtype=np.uint8)
    emu = BatchedEmulator(rom, n, render=True)
    got = []
    for t in range(acts.shape[0]):
        emu.step(torch.from_numpy(acts[t]).to(emu.device))
        torch.cuda.synchronize()
        got.append(emu.last_instr_count())
    emu.close()
    assert got == OP.instr_counts(rom, acts)


def test_frame_watchdog_parity():
    """Frames ended by the watchdog budget (the LCD switched off faster than once per frame, with
    timer stretches and TIMA interrupts; fuzz.py lcd_toggle_rom): K1 bounds its tick limit by the
    budget instead of testing it every iteration, so the budget's end must still land on the
    oracle's instruction."""
    from pokegym_amd.testrom.fuzz import lcd_toggle_rom
    n = 128
    gpu, ref = _run_both(lcd_toggle_rom(), None, n, 2, 11)
    bad = [(e, _diff(gpu[e], ref[e].tobytes())) for e in range(n) if gpu[e] != ref[e].tobytes()]
    assert not bad, bad[:4]


@pytest.mark.parametrize("shape", [("", ""), ("512", "32"), ("512", "64")])
def test_hram_code_parity(shape, monkeypatch):
    """Code run from inside, across and outside the HRAM bytes K1 mirrors in LDS (0xFF80-0xFF9F),
    self-modified every pass, under the default shape and 512-thread workgroups of 32/64-env waves."""
    from pokegym_amd.testrom.fuzz import hram_code_rom
    block, lanes = shape
    if block:
        monkeypatch.setenv("PK_K1_BLOCK", block)
        monkeypatch.setenv("PK_WAVE_LANES", lanes)
    n = 1024 if lanes == "64" else 256
    gpu, ref = _run_both(hram_code_rom(), None, n, 4, 31)
    bad = [(e, _diff(gpu[e], ref[e].tobytes())) for e in range(n) if gpu[e] != ref[e].tobytes()]
    assert not bad, bad[:4]


def test_hram_code_parity_64_banks():
    """The same code on a 64-bank cartridge: K1's unstaged-bank instance, whose write stage updates
    the HRAM mirror behind its own rare branch (8- and 16-bit self-modifying writes)."""
    from pokegym_amd.testrom.fuzz import hram_code_rom
    n = 256
    gpu, ref = _run_both(hram_code_rom(64), None, n, 4, 31)
    bad = [(e, _diff(gpu[e], ref[e].tobytes())) for e in range(n) if gpu[e] != ref[e].tobytes()]
    assert not bad, bad[:4]


@pytest.mark.parametrize("n_banks", [2, 64])
def test_io_edges_parity(n_banks):
    """The IO accesses K1 serves first inside its rare branches (one-byte DIV / JOYP reads, sound /
    JOYP writes) beside 16-bit and read-modify-write accesses at the same addresses, the timer
    running and JOYP's select changing every pass (fuzz.py io_edge_rom); 2 banks: the every-bank
    staged instance, 64: the unstaged-bank one."""
    from pokegym_amd.testrom.fuzz import io_edge_rom
    n = 256
    gpu, ref = _run_both(io_edge_rom(n_banks), None, n, 4, 7)
    bad = [(e, _diff(gpu[e], ref[e].tobytes())) for e in range(n) if gpu[e] != ref[e].tobytes()]
    assert not bad, bad[:4]


@pytest.mark.parametrize("n_banks,small", [(8, False), (8, True), (64, False), (64, True)])
def test_irq_bank_parity(n_banks, small, monkeypatch):
    """IF / IE writes and read-modify-writes with IME off, then an IME-on window where what they left
    pending dispatches (K1's cached pending-interrupt bit), the timer on in half of the passes; ROM
    bank switches issued from code in the switchable bank, the next instruction fetched from the new
    bank (K1's prefetch across a slow write) — fuzz.py irq_bank_rom; in the default kernel (8 banks:
    six staged in LDS, 64: the unstaged-bank instance) and in the small-LDS kernel the VecEnv
    sub-batches run (2 slots: most switches go to or from a global-ROM bank)."""
    from pokegym_amd.testrom.fuzz import irq_bank_rom
    if small:
        monkeypatch.setenv("PK_K1_SMALL", "1")
        monkeypatch.setenv("PK_WAVE_LANES", "32")
        monkeypatch.setenv("PK_K1_BLOCK", "256")
    n = 256
    gpu, ref = _run_both(irq_bank_rom(n_banks), None, n, 4, 13)
    bad = [(e, _diff(gpu[e], ref[e].tobytes())) for e in range(n) if gpu[e] != ref[e].tobytes()]
    assert not bad, bad[:4]


@pytest.mark.parametrize("small", [False, True])
def test_vram_midframe_parity(small, monkeypatch):
    """VRAM / OAM / SCY / LCDC writes in the middle of the visible frame, about ten a frame, at map rows
    the pending (latched, not yet rasterised) lines show and rows they do not, tile data, OAM, the
    window's rows and the map not shown (fuzz.py vram_midframe_rom): K1 rasterises pending lines
    before a write only when the write would change one of them (pk_step.hip pend_hit); whole state
    and screen vs the oracle, in the default kernel and in the small-LDS kernel of the VecEnv
    sub-batches."""
    from pokegym_amd.testrom.fuzz import vram_midframe_rom
    if small:
        monkeypatch.setenv("PK_K1_SMALL", "1")
        monkeypatch.setenv("PK_WAVE_LANES", "32")
        monkeypatch.setenv("PK_K1_BLOCK", "256")
    import torch
    from pokegym_amd.emulator import BatchedEmulator
    rom, n, steps = vram_midframe_rom(), 256, 6
    actions = np.random.default_rng(17).integers(0, 9, size=(steps, n), dtype=np.uint8)
    emu = BatchedEmulator(rom, n, render=True)
    for t in range(steps):
        emu.step(torch.from_numpy(actions[t]).to(emu.device))
    torch.cuda.synchronize()
    gpu = [emu.snapshot(e) for e in range(n)]
    scr = emu.screen.cpu().numpy()
    emu.close()
    ref, ref_scr = oracle.batch_run(rom, None, actions)
    grey = np.array([0xFF, 0x99, 0x55, 0x00], np.uint8)
    bad = [(e, _diff(gpu[e], ref[e].tobytes())) for e in range(n) if gpu[e] != ref[e].tobytes()]
    assert not bad, bad[:4]
    assert all(np.array_equal(scr[e], grey[ref_scr[e]]) for e in range(n))


@pytest.mark.parametrize("small", [False, True])
def test_raster_fx_parity(small, monkeypatch):
    """Registers rewritten line by line (fuzz.py raster_fx_rom): a STAT LY=LYC handler changes SCX,
    SCY, WX, WY, the three palettes and LCDC bits 0-6 on env-dependent lines, 40 overlapping objects
    (fourteen on the same lines) switch between 8x8 and 8x16 mid-frame, and every fourth pass HALTs
    until VBlank partway down the frame — K1's per-event line latch and the bulk latch of the HALT
    skip-ahead, with the window line counter they carry; 24/8 steps, whole state and screen vs the
    oracle, in the default kernel and in the small-LDS kernel."""
    from pokegym_amd.testrom.fuzz import raster_fx_rom
    if small:
        monkeypatch.setenv("PK_K1_SMALL", "1")
        monkeypatch.setenv("PK_WAVE_LANES", "32")
        monkeypatch.setenv("PK_K1_BLOCK", "256")
    import torch
    from pokegym_amd.emulator import BatchedEmulator
    rom, n, steps = raster_fx_rom(), 256, 6
    actions = np.random.default_rng(29).integers(0, 9, size=(steps, n), dtype=np.uint8)
    emu = BatchedEmulator(rom, n, render=True)
    for t in range(steps):
        emu.step(torch.from_numpy(actions[t]).to(emu.device))
    torch.cuda.synchronize()
    gpu = [emu.snapshot(e) for e in range(n)]
    scr = emu.screen.cpu().numpy()
    emu.close()
    ref, ref_scr = oracle.batch_run(rom, None, actions)
    grey = np.array([0xFF, 0x99, 0x55, 0x00], np.uint8)
    bad = [(e, _diff(gpu[e], ref[e].tobytes())) for e in range(n) if gpu[e] != ref[e].tobytes()]
    assert not bad, bad[:4]
    assert all(np.array_equal(scr[e], grey[ref_scr[e]]) for e in range(n))


@pytest.mark.gpu
@pytest.mark.parametrize("small", [False, True])
def test_dma_wait_parity(small, monkeypatch):
    """pokered's OAM-DMA wait loop (dec a / jr nz) that K1 runs in whole passes (pk_step.hip
    pk_dec_loop): from HRAM and ROM, A = 0 / 1 / any, carry in or out, timer on/off, STAT / VBlank /
    timer interrupts dispatching inside the loop (fuzz.py dma_wait_rom); whole state vs the oracle
    in the default kernel and in the small-LDS kernel of the VecEnv sub-batches."""
    from pokegym_amd.testrom.fuzz import dma_wait_rom
    if small:
        monkeypatch.setenv("PK_K1_SMALL", "1")
        monkeypatch.setenv("PK_WAVE_LANES", "32")
        monkeypatch.setenv("PK_K1_BLOCK", "256")
    import torch
    from pokegym_amd.emulator import BatchedEmulator
    rom, n, steps = dma_wait_rom(), 256, 6
    actions = np.random.default_rng(23).integers(0, 9, size=(steps, n), dtype=np.uint8)
    emu = BatchedEmulator(rom, n, render=True)
    for t in range(steps):
        emu.step(torch.from_numpy(actions[t]).to(emu.device))
    torch.cuda.synchronize()
    gpu = [emu.snapshot(e) for e in range(n)]
    emu.close()
    ref, _ = oracle.batch_run(rom, None, actions)
    bad = [(e, _diff(gpu[e], ref[e].tobytes())) for e in range(n) if gpu[e] != ref[e].tobytes()]
    assert not bad, bad[:4]


def warp_actions(n, seed=5):
    """Actions (6, n) from the warp fixture's state: columns 0..n/2-1 the recorded actions (they
    walk through a door at step 2: pkbench's map load with the LCD off for ~5 frames), the rest
    seeded random presses."""
    d = np.load(os.path.join(GOLD, "warp_state.npz"))
    acts = np.random.default_rng(seed).integers(0, 9, size=(len(d["actions"]), n), dtype=np.uint8)
    acts[:, :n // 2] = d["actions"][:, None]
    return d["state"].tobytes(), acts


@pytest.mark.parametrize("shape", [("", ""), ("16", "512"), ("32", "512")])
def test_map_load_warp_parity(shape, monkeypatch):
    """pkbench's door warp (DisableLCD, 2 KiB of VRAM and 4 KiB of WRAM copied over ~5 LCD-off
    frames, EnableLCD) from the fixture state, in lockstep and beside diverging envs, at the small
    launch shape and the benchmarked 512-thread shapes; whole v9 state vs the oracle."""
    import torch
    from pokegym_amd.emulator import BatchedEmulator
    from pokegym_amd.testrom.game import game_rom
    lanes, block = shape
    if lanes:
        monkeypatch.setenv("PK_WAVE_LANES", lanes)
        monkeypatch.setenv("PK_K1_BLOCK", block)
    rom, n = game_rom(), 128
    state, acts = warp_actions(n)
    emu = BatchedEmulator(rom, n, state=state, render=True)
    for t in range(len(acts)):
        emu.step(torch.from_numpy(acts[t]).to(emu.device))
    torch.cuda.synchronize()
    gpu = [emu.snapshot(e) for e in range(n)]
    emu.close()
    ref, _ = oracle.batch_run(rom, state, acts, want_screens=False)
    bad = [(e, _diff(gpu[e], ref[e].tobytes())) for e in range(n) if gpu[e] != ref[e].tobytes()]
    assert not bad, bad[:4]


@pytest.mark.parametrize("shape", [("", ""), ("16", "512"), ("32", "512")])
def test_copydata_block_path_parity(shape, monkeypatch):
    """pokered's CopyData loop and its B/C twin, which K1 runs in blocks of whole passes
    (pk_step.hip pk_copy_loop): ROM/WRAM/VRAM sources, VRAM/WRAM/overlapping/HRAM/OAM destinations,
    VBlank/STAT/timer interrupts inside copies, LCD-off copies (fuzz.py copydata_rom); whole v9
    state vs the oracle at the small launch shape and the benchmarked 512-thread shapes."""
    from pokegym_amd.testrom.fuzz import copydata_rom
    lanes, block = shape
    if lanes:
        monkeypatch.setenv("PK_WAVE_LANES", lanes)
        monkeypatch.setenv("PK_K1_BLOCK", block)
    n = 256
    gpu, ref = _run_both(copydata_rom(), None, n, 6, 17)
    bad = [(e, _diff(gpu[e], ref[e].tobytes())) for e in range(n) if gpu[e] != ref[e].tobytes()]
    assert not bad, bad[:4]


@pytest.mark.parametrize("small", [False, True])
def test_sm83_kat_on_device(small, monkeypatch):
    """The HIP K1 runs the known-answer ROM (pokegym_amd/testrom/kat.py, A values stepping by 5), one
    group of blocks per env (64 envs): every block hash == the documented CPU's (tests/sm83_spec.py)
    — the 8-bit ALU with carry clear and set, DAA, INC/DEC, rotates/shifts/SWAP/BIT, CPL/SCF/CCF,
    ADD HL,BC, ADD SP,e and LD HL,SP+e — and the whole state == the oracle's; in the default kernel
    and in the small-LDS kernel of the VecEnv sub-batches."""
    import torch
    from pokegym_amd.emulator import BatchedEmulator
    from pokegym_amd.testrom import kat
    from tests.test_sm83_kat import check_group_outputs, kernel_outputs
    if small:
        monkeypatch.setenv("PK_K1_SMALL", "1")
        monkeypatch.setenv("PK_WAVE_LANES", "32")
        monkeypatch.setenv("PK_K1_BLOCK", "256")
    stride, n, steps = 5, 64, 24
    rom = kat.kat_rom(stride)
    groups = [e % 8 for e in range(n)]
    acts = np.array([kat.GROUP_ACTION[g] for g in groups], np.uint8)
    emu = BatchedEmulator(rom, n, render=True)
    a = torch.from_numpy(acts).to(emu.device)
    for _ in range(steps):
        emu.step(a)
    torch.cuda.synchronize()
    states = emu.snapshot_range(0, n)
    emu.close()
    assert check_group_outputs(kernel_outputs(rom, states), groups, stride) == []
    ref, _ = oracle.batch_run(rom, None, np.repeat(acts[None, :], steps, axis=0), want_screens=False)
    bad = [e for e in range(n) if states[e].tobytes() != ref[e].tobytes()]
    assert not bad, bad[:8]


@pytest.mark.parametrize("small,n_banks", [(False, 2), (True, 2), (False, 64)])
def test_sm83_matrix_on_device(small, n_banks, monkeypatch):
    """The HIP K1 runs the opcode-matrix ROM (pokegym_amd/testrom/kat_matrix.py): every legal opcode
    but HALT / STOP / DI / EI in a block behind a taken jp (K1's primary table entry) and, for the
    opcodes of the secondary table, in a block behind a nop (the fused path), each over V vectors of
    registers, flags and memory; one group of blocks per env (64 envs).  Every block hash == the
    documented CPU's (tests/sm83_spec.py step()), wDone set, and the whole state == the oracle's; in
    the default kernel (2 banks, and 64: half of the blocks fetched from the global ROM) and in the
    small-LDS kernel of the VecEnv sub-batches."""
    import torch
    from pokegym_amd.emulator import BatchedEmulator
    from pokegym_amd.testrom import kat_matrix as KM
    from tests.test_sm83_matrix import check_groups, kernel_block_hashes, matrix
    if small:
        monkeypatch.setenv("PK_K1_SMALL", "1")
        monkeypatch.setenv("PK_WAVE_LANES", "32")
        monkeypatch.setenv("PK_K1_BLOCK", "256")
    n, steps = 64, 8
    m = matrix(n_banks)
    groups = [e % 8 for e in range(n)]
    acts = np.array([KM.GROUP_ACTION[g] for g in groups], np.uint8)
    emu = BatchedEmulator(m.rom, n, render=True)
    a = torch.from_numpy(acts).to(emu.device)
    for _ in range(steps):
        emu.step(a)
    torch.cuda.synchronize()
    states = emu.snapshot_range(0, n)
    emu.close()
    assert check_groups(m, kernel_block_hashes(m, states), groups) == []
    ref, _ = oracle.batch_run(m.rom, None, np.repeat(acts[None, :], steps, axis=0), want_screens=False)
    bad = [e for e in range(n) if states[e].tobytes() != ref[e].tobytes()]
    assert not bad, bad[:8]


# ---------------------------------------------------------------------------------------------
# Every step end, not only the last: per-frame parity (frame_skip=1) and the other values of
# frame_skip / release_frame, the two pk_config fields the tests above never vary.
def _lockstep(rom, state, acts, frame_skip, release_frame, tally=None):
    """BatchedEmulator and n oracle emulators stepped side by side over acts (steps, n): the whole
    v9 state of every env and its screen compared after EVERY step; returns the mismatches
    [(step, env, first differing bytes)] of the first step that has one."""
    import torch
    from pokegym_amd.emulator import BatchedEmulator
    from tests.test_frame_boundary import GREY, OracleBatch
    steps, n = acts.shape
    emu = BatchedEmulator(rom, n, state=state, render=True, frame_skip=frame_skip, release_frame=release_frame)
    ob = OracleBatch(rom, n, state)
    bad = []
    for t in range(steps):
        emu.step(torch.from_numpy(acts[t]).to(emu.device))
        ref, ref_scr = ob.step(acts[t], frame_skip, release_frame)
        gpu = emu.snapshot_range(0, n)              # synchronous
        scr = emu.screen.cpu().numpy()
        if tally is not None:
            tally.add(gpu, t)
        if not np.array_equal(gpu, ref) or not np.array_equal(scr, GREY[ref_scr]):
            bad = [(t, e, _diff(gpu[e].tobytes(), ref[e].tobytes())) for e in range(n)
                   if not np.array_equal(gpu[e], ref[e]) or not np.array_equal(scr[e], GREY[ref_scr[e]])]
            break
    emu.close()
    ob.close()
    return bad


# frames per case: 72 (144 for the warp fixture), halved where the case ran longer than
# test_vram_midframe_parity (1.5-1.6 s) in the same MI355X run — vram_midframe took 6.5 s at 72
# frames (every frame is rendered, so each of its ~10 mid-frame writes per frame flushes the pending
# lines inside K1, lane by lane), the warp fixture 1.6 s at 144 and fuzz3 1.6 s at 72.  vram_midframe
# cannot be halved again: its 3 LCD-off boot frames would be more than 10 % of 18.  The warp
# fixture's first 72 frames hold the recorded door warp (LCD off in frames 57-61) and ten rendered
# frames after it.  raster_fx took 0.6 s at 36 frames (its register rewrites flush nothing: no VRAM
# or OAM write); its 2 LCD-off boot frames keep it from being halved below 36 as well.
PER_FRAME_STEPS = {"pkbench": 72, "fuzz3": 36, "vram_midframe": 36, "warp": 72, "raster_fx": 36}
_per_frame_tallies = {}


def _per_frame(name, small):
    """One per-frame case (cached: the coverage test below reads the tallies of the cases run)."""
    from tests.test_frame_boundary import FrameEndTally, frame_case
    if (name, small) not in _per_frame_tallies:
        rom, state, acts, mult4 = frame_case(name, 96, PER_FRAME_STEPS[name])
        tally = FrameEndTally()
        bad = _lockstep(rom, state, acts, 1, 8, tally)
        _per_frame_tallies[(name, small)] = (tally, bad, mult4)
    return _per_frame_tallies[(name, small)]


@pytest.mark.parametrize("small", [False, True])
@pytest.mark.parametrize("name", ["pkbench", "fuzz3", "vram_midframe", "warp", "raster_fx"])
def test_per_frame_parity(name, small, monkeypatch):
    """frame_skip=1, release_frame=8: every frame is a step end and is rasterised (K1 enters with
    s.render set; the pend_hit / flush_lines filter and K2 run on every frame).  96 envs — one full
    64-env group and a ragged half — of pkbench, fuzz_rom(3), vram_midframe_rom, raster_fx_rom (its
    per-line LCDC / scroll / window / palette rewrites and mid-frame HALTs) and the warp fixture
    (test_map_load_warp_parity's action layout with each action held 24 frames, so the LCD-off
    frames of the map load are rendered and compared), PER_FRAME_STEPS frames; whole v9 state and
    screen vs the oracle after every frame, in the default kernel and in the small-LDS kernel; every
    snapshot satisfies PyBoy's frame-end facts (tests/test_frame_boundary.py check_frame_end), at
    most 10 % of them without evidence (LCD off / off VBlank)."""
    if small:
        monkeypatch.setenv("PK_K1_SMALL", "1")
        monkeypatch.setenv("PK_WAVE_LANES", "32")
        monkeypatch.setenv("PK_K1_BLOCK", "256")
    tally, bad, mult4 = _per_frame(name, small)
    print(name, "small" if small else "default", tally.report())
    assert not bad, bad[:4]
    tally.assert_ok(mult4)


def test_per_frame_parity_covers_halted_and_overshooting_ends():
    """Across the ROM list (default kernel) halted frame ends and running ones whose last
    instruction ran past the boundary were both checked on the device."""
    tallies = [_per_frame(name, False)[0] for name in PER_FRAME_STEPS]
    assert sum(t.halted for t in tallies) > 0
    assert sum(c for t in tallies for o, c in t.overshoot.items() if o > 0) > 0


@pytest.mark.parametrize("name", ["pkbench", "irq_bank"])
@pytest.mark.parametrize("frame_skip,release_frame", [(1, 0), (2, 1), (8, 8), (9, 8), (24, 0), (24, 23), (24, 24),
                                                      (8, 200)])
def test_frame_skip_release_frame_parity(frame_skip, release_frame, name):
    """pk_config's frame_skip and release_frame away from 24 / 8, on pkbench and irq_bank_rom(8) (its
    joypad-interrupt traffic), 96 envs, actions 0..8 (some envs press nothing), whole v9 state and
    screen vs the oracle after every step.  The reference releases the button at the top of loop
    pass i == release_frame (pyboy_binding.py:79-81); with release_frame >= frame_skip — (8,8),
    (24,24), (8,200) — that pass does not exist, the step releases nothing and the button is still
    down when the next step presses."""
    from pokegym_amd.testrom.fuzz import irq_bank_rom
    from pokegym_amd.testrom.game import game_rom
    rom = game_rom() if name == "pkbench" else irq_bank_rom(8)
    n, steps = 96, 24 if frame_skip <= 2 else 6
    if name == "irq_bank" and frame_skip == 24 and release_frame >= 23:
        steps = 3   # 2.7 s at 6 steps (the button held through the whole step), longer than test_vram_midframe_parity
    acts = np.random.default_rng(1000 * frame_skip + release_frame).integers(0, 9, size=(steps, n), dtype=np.uint8)
    bad = _lockstep(rom, None, acts, frame_skip, release_frame)
    assert not bad, bad[:4]
