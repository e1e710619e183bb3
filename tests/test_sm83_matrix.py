"""Every legal SM83 opcode but HALT / STOP / DI / EI, in the step kernel's primary path and, where
its secondary table has an entry, in the fused path, pinned to the documented CPU.

pokegym_amd/testrom/kat_matrix.py runs one block per (opcode, path variant) over V input vectors
and hashes all registers, SP, a scratch window of WRAM, two HRAM bytes and a landing marker;
tests/sm83_spec.py step() states what the documentation says the same bytes do, and expected()
below folds it over each block's instruction stream from the block's entry to the capture routine
it lands in.  The oracle (full ROM, every vector) and the host-simulated K1 (2 and 64 banks, one
joypad group per env) must give the statement's hash for every block; the host simulation's trace
must show each opcode at its block's address as a primary record and, for the fused blocks, as a
record marked 0x2000 (fused secondary op).  The HIP kernel runs the same ROM in
tests/test_gpu_parity.py test_sm83_matrix_on_device."""
import ctypes
import functools
import inspect
import types

import numpy as np
import pytest

from pokegym_amd.testrom import kat_matrix as KM
from tests import sm83_spec as S
from tests.test_ucode_table import table_report  # noqa: F401  (fixture)

V = 13           # vectors per block (kat_matrix.matrix() says why not 16); a group takes 6 env-steps of 24 frames
MAX_STEPS = 48   # env-steps a group may take (a budget: one needs 6)


@functools.lru_cache(maxsize=None)
def matrix(n_banks=2):
    return KM.matrix(n_banks, V)


class _Mem:
    """What a block may touch: the ROM as mapped while the blocks run, the scratch window, the
    marker and the two HRAM bytes; a read anywhere else is an error of the statement."""

    def __init__(self, m, ram):
        self.m, self.ram = m, ram

    def __getitem__(self, a):
        return self.m.fetch(a) if a < 0x8000 else self.ram[a]

    def write(self, a, v):
        if a not in self.ram:
            raise KeyError(f"write outside the window: {a:04X}")
        self.ram[a] = v


def run_vector(m, b, v, spec=S):
    """Block b on vector v by the statement: the hashed bytes, in the ROM's order."""
    f, a, c, bb, e, d, l, h = v[:8]
    regs = dict(A=a, F=f, B=bb, C=c, D=d, E=e, H=h, L=l, SP=KM.W_REGS + 10, PC=b.entry)
    ram = {KM.W_SCR + i: v[8 + i] for i in range(8)}
    ram.update({0xFF00 + KM.HRAM_LO: v[8], 0xFF00 + KM.HRAM_HI: v[9], KM.W_MARK: 0})
    mem = _Mem(m, ram)
    for _ in range(16):
        pc = regs["PC"]
        if pc in m.caps:
            break
        code = [mem[(pc + i) & 0xFFFF] for i in range(spec.length(mem[pc]))]
        regs, writes, _ = spec.step(regs, mem, code)
        for wa, wv in writes:
            mem.write(wa, wv)
    else:
        raise RuntimeError(f"{b.name}: did not reach a capture routine")
    mark = m.caps[regs["PC"]]
    mark = ram[KM.W_MARK] if mark is None else mark
    return ([regs[k] for k in "LHEDCBFA"] + [regs["SP"] & 0xFF, regs["SP"] >> 8]
            + [ram[KM.W_SCR + i] for i in range(8)] + [mark, ram[0xFF00 + KM.HRAM_LO], ram[0xFF00 + KM.HRAM_HI]])


def expected(m, b, spec=S):
    f = spec.Fletcher()
    for v in m.vectors:
        f.add(*run_vector(m, b, v, spec))
    return f.pair()


@functools.lru_cache(maxsize=None)
def expected_all(n_banks=2):
    m = matrix(n_banks)
    return [expected(m, b) for b in m.blocks]


def block_hashes(m, read):
    return [(read(b.out), read(b.out + 1)) for b in m.blocks]


# ---- the ROM covers what it says ----
def test_matrix_covers_every_in_scope_opcode(table_report):  # noqa: F811
    m = matrix()
    prim = {b.op for b in m.blocks if not b.fused}
    want = {op for op in range(256) if op not in S.ILLEGAL and op not in S.OUT_OF_SCOPE and op != 0xCB}
    assert prim == want | {0x100 | cb for cb in range(256)}
    # the fused variants: exactly the opcodes K1's secondary table implements (pk_u2_entry length != 0)
    table = {op for op in range(256) if table_report[f"u2_{op}"] & 3}
    assert {b.op for b in m.blocks if b.fused} == table == set(KM.FUSED_OPS)
    assert len(m.vectors) >= 8
    edge = {0x00, 0xFF, 0x0F, 0x10, 0x7F, 0x80}
    assert all(any(v[i] == x for v in m.vectors) for i in range(1, 8) for x in edge), "every register sees every edge"
    assert {(v[0] >> 7, (v[0] >> 4) & 1) for v in m.vectors} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    distinct = sum(len(set(v[1:8])) == 7 for v in m.vectors)
    assert distinct * 4 >= len(m.vectors) * 3, "registers pairwise distinct in most vectors"
    assert any(v[12] & 0x0F for v in m.vectors), "pop af must see a low nibble != 0"
    for n_banks in (2, 64):
        hi = sum(b.high for b in matrix(n_banks).blocks)
        assert abs(2 * hi - len(m.blocks)) <= 16
    assert matrix(64).bank > 6


def test_conditionals_run_taken_and_not_taken():
    """Every conditional JP / JR / CALL / RET block lands both ways over the vectors, and every RST
    block comes back with its own vector's marker."""
    m = matrix()
    for b in m.blocks:
        cond = b.op in (0x20, 0x28, 0x30, 0x38) or (b.op < 0x100 and b.op >> 6 == 3 and b.op & 7 in (0, 2, 4) and (b.op >> 3) & 7 < 4)
        marks = {run_vector(m, b, v)[18] for v in m.vectors}
        if cond:
            assert marks == {KM.MARK_FELL, KM.MARK_LANDED}, b.name
        elif b.op < 0x100 and b.op & 0xC7 == 0xC7:
            assert marks == {KM.MARK_RST + ((b.op >> 3) & 7)}, b.name
        elif b.op in (0x18, 0xC3, 0xCD, 0xC9, 0xD9, 0xE9):
            assert marks == {KM.MARK_LANDED}, b.name
        else:
            assert marks == {0}, b.name


# ---- the oracle ----
def run_oracle(m, group=None):
    from oracle import oracle as O
    gb = O.GB(m.rom)
    gb.power_on()
    act = 8 if group is None else KM.GROUP_ACTION[group]
    for _ in range(MAX_STEPS * (8 if group is None else 1)):   # no button: all eight groups in one run
        gb.run_action(act)
        if gb.read(KM.W_DONE):
            break
    assert gb.read(KM.W_DONE), "the matrix ROM did not finish"
    return block_hashes(m, gb.read)


@pytest.fixture(scope="module")
def oracle_out():
    return run_oracle(matrix())


@pytest.mark.parametrize("k,name", [(b.k, b.name) for b in KM.blocks()], ids=[b.name for b in KM.blocks()])
def test_oracle_block_matches_documented_cpu(oracle_out, k, name):
    assert oracle_out[k] == expected_all()[k], name


def test_oracle_64_banks_and_group_selection():
    """The 64-bank build (half of the blocks in bank HIGH_BANK) gives the same hashes; a pressed
    button runs its group's blocks only."""
    m = matrix(64)
    assert run_oracle(m) == expected_all(64) == expected_all(2)
    out = run_oracle(matrix(), group=5)
    want = expected_all()
    assert all(out[b.k] == (want[b.k] if b.group == 5 else (0, 0)) for b in matrix().blocks)


# ---- the hash tells single-rule changes of the statement apart ----
def _block(name):
    return next(b for b in matrix().blocks if b.name == name)


MUTATIONS = {
    "ld d,h reads L": ("54_ld_d,h-primary", "        set8(mid, get8(lo))", "        set8(mid, get8(5 if op == 0x54 else lo))"),
    "pop af keeps the low nibble": ("f1_pop_af-primary", 'r["A"], r["F"] = v >> 8, v & 0xF0', 'r["A"], r["F"] = v >> 8, v & 0xFF'),
    "res sets": ("cb91_res_2,c-primary", "set8(n & 7, v & ~(1 << b))", "set8(n & 7, v | (1 << b))"),
    "set n,(hl) bit index off by one": ("cbde_set_3,[hl]-primary", "set8(n & 7, v | (1 << b))              # SET b",
                                        "set8(n & 7, v | (1 << (b + 1 if n & 7 == 6 else b)))"),
    "ret nz polarity": ("c0_ret_nz-primary", "            taken = cond(mid)\n            if taken:\n                r[\"PC\"] = pop()",
                        "            taken = cond(mid ^ (op == 0xC0))\n            if taken:\n                r[\"PC\"] = pop()"),
    "call pushes pc+2": ("cd_call_nn-primary", "                push(nxt)\n                r[\"PC\"] = nn", "                push(nxt - 1)\n                r[\"PC\"] = nn"),
    "jr displacement unsigned": ("20_jr_nz,e_back-fused","r[\"PC\"] = (nxt + (n - 256 if n & 0x80 else n)) & 0xFFFF", "r[\"PC\"] = (nxt + n) & 0xFFFF"),
    "ld (hl-) increments": ("32_ld_[hl-],a-primary", "set16(2, a - 1)", "set16(2, a + 1)"),
    "inc de touches Z": ("13_inc_de-fused", "            set16(mid >> 1, get16(mid >> 1) + (-1 if mid & 1 else 1))",
                         "            set16(mid >> 1, get16(mid >> 1) + (-1 if mid & 1 else 1))\n"
                         "            r[\"F\"] = (r[\"F\"] & ~Z & 0xFF) | (Z if get16(mid >> 1) == 0 else 0)"),
    "ldh uses 0xFE00": ("e0_ldh_[n],a_lo-primary", "wr(0xFF00 + n, r[\"A\"])", "wr(0xFE00 + n, r[\"A\"])"),
    "push order low/high": ("d5_push_de-primary", "        wr(r[\"SP\"] + 1, v >> 8)\n        wr(r[\"SP\"], v & 0xFF)",
                            "        wr(r[\"SP\"] + 1, v & 0xFF)\n        wr(r[\"SP\"], v >> 8)"),
    "jp hl loads (hl)": ("e9_jp_hl-primary", "r[\"PC\"] = get16(2)", "r[\"PC\"] = rd(get16(2)) | (rd(get16(2) + 1) << 8)"),
    "ld [hl],l stores H": ("75_ld_[hl],l-primary", "        set8(mid, get8(lo))", "        set8(mid, get8(4 if op == 0x75 else lo))"),
    "rst 00 goes to 08": ("c7_rst_00h-primary", "r[\"PC\"] = mid * 8", "r[\"PC\"] = mid * 8 + (8 if op == 0xC7 else 0)"),
    "ld sp,hl swaps the bytes": ("f9_ld_sp,hl-primary", "r[\"SP\"] = get16(2)", "r[\"SP\"] = (r[\"L\"] << 8) | r[\"H\"]"),
}


@pytest.mark.parametrize("rule", sorted(MUTATIONS))
def test_hash_detects_a_changed_rule(rule):
    name, a, b = MUTATIONS[rule]
    src = inspect.getsource(S)
    assert src.count(a) == 1, rule
    mutated = types.ModuleType("sm83_spec_mutated")
    exec(compile(src.replace(a, b), "sm83_spec_mutated", "exec"), mutated.__dict__)
    m, blk = matrix(), _block(name)
    want = expected(m, blk)
    try:
        got = expected(m, blk, mutated)
    except (KeyError, RuntimeError):
        got = None   # the changed rule ran off the block or out of its window: seen as well
    assert got != want, f"{rule}: the hash of {name} does not see the change"


# ---- the host-simulated step kernel ----
def kernel_block_hashes(m, states):
    """Per env: (done flag, block hashes) read from the env's v9 state."""
    from oracle import oracle as O
    out = []
    for st in states:
        gb = O.GB(m.rom)
        gb.load_state(bytes(st))
        out.append((gb.read(KM.W_DONE), block_hashes(m, gb.read)))
    return out


def check_groups(m, outs, groups):
    """The blocks whose hash an env of their group did not get right: (env, block name)."""
    assert all(d for d, _ in outs), "the matrix ROM did not finish"
    want = expected_all(m.n_banks)
    return [(e, b.name) for e, ((_, o), g) in enumerate(zip(outs, groups)) for b in m.blocks
            if b.group == g and o[b.k] != want[b.k]]


@pytest.fixture(scope="module")
def hostsim_runs():
    """{n_banks: (group check result, census)} of the host-simulated K1, 8 envs, env e = group e."""
    from tests.hostsim import sim
    L = sim.lib()
    L.pk_sim_census_enable.argtypes = [ctypes.c_int]
    L.pk_sim_census_get.argtypes = [ctypes.c_void_p]
    res = {}
    for n_banks in (2, 64):
        m = matrix(n_banks)
        groups = list(range(8))
        acts = np.array([KM.GROUP_ACTION[g] for g in groups], np.uint8)
        L.pk_sim_census_enable(1)
        emu = sim.SimEmulator(m.rom, len(groups))
        try:
            for steps in range(1, MAX_STEPS + 1):
                emu.step(acts)
                outs = kernel_block_hashes(m, emu.snapshot_range(0, len(groups)))
                if all(d for d, _ in outs):
                    break
            census = np.zeros((4, 65536), np.uint32)
            L.pk_sim_census_get(census.ctypes.data)
        finally:
            emu.close()
            L.pk_sim_census_enable(0)
        res[n_banks] = (m, outs, groups, census, steps)
    return res


@pytest.mark.parametrize("n_banks", [2, 64])
def test_hostsim_kernel_matrix(hostsim_runs, n_banks):
    """K1 (host-simulation build of pk_step.hip), one joypad group per env: every block hash == the
    documented CPU's, within MAX_STEPS env-steps."""
    m, outs, groups, _, steps = hostsim_runs[n_banks]
    print(f"{n_banks} banks: all groups done after {steps} env-steps")
    assert check_groups(m, outs, groups) == []


@pytest.mark.parametrize("n_banks", [2, 64])
def test_census_every_opcode_in_both_paths(hostsim_runs, n_banks):
    """From the host simulation's trace over all groups: every in-scope opcode ran as a primary at
    its primary block's address, every opcode with a secondary entry ran fused (record bit 0x2000)
    at its fused block's address."""
    m, _, _, census, _ = hostsim_runs[n_banks]
    first = lambda b: 0xCB if b.op >= 0x100 else b.op   # noqa: E731  (the trace holds the first byte)
    prim = [b for b in m.blocks if not b.fused]
    fused = [b for b in m.blocks if b.fused]
    no_prim = [b.name for b in prim if not (census[0, b.op_pc] and census[2, b.op_pc] == first(b))]
    no_fused = [b.name for b in fused if not (census[1, b.op_pc] and census[3, b.op_pc] == first(b))]
    got_p = {b.op for b in prim} - {b.op for b in prim if b.name in no_prim}
    got_f = {b.op for b in fused} - {b.op for b in fused if b.name in no_fused}
    print(f"{n_banks} banks: {len(got_p)} opcodes with a primary record, {len(got_f)} with a fused record")
    assert not [b.name for b in prim if census[1, b.op_pc]], "a primary block's opcode ran fused"
    assert not no_prim, no_prim[:10]
    assert not no_fused, no_fused[:10]
    assert len(got_p) == 240 + 256 and len(got_f) == len(KM.FUSED_OPS)
