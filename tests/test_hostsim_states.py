"""K1 (host-simulation build of pk_step.hip, pk_check_lane active) and the oracle side by side from
the injected machine states of tests/state_cases.py: whole v9 state and screen after every step,
each case's loop-skip expectation from the trace, and the census of what the cases exercised.
The gfx950 build runs the same cases in tests/test_gpu_states.py."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

from pokegym_amd.testrom import stage as ST
from tests import state_cases as SC
from tests import state_common as CM

EV_INT, EV_IDLE, EV_EXEC = 1 << 4, 1 << 5, 1 << 0
LOOPS = ("copy", "poll", "dec")


def test_patch_round_trip():
    """patch -> GB.load_state -> save_state is the identity on every field patch() can set."""
    from oracle import oracle as O
    rom = ST.stage_rom(2)
    base = SC.phase(2, 3, 70, 100)[0]
    vals = {"a": 0x12, "f": 0xB0, "b": 0x34, "c": 0x56, "d": 0x78, "e": 0x9A, "hl": 0xBCDE, "sp": 0xFE01, "pc": 0x7FFF,
            "ime": 1, "halted": 1, "queued": 1, "ie": 0xFF, "if_": 0xE5, "div": 0xC3, "tima": 0xFE, "divc": 0xA7, "timac": 0x3FE,
            "tma": 0xF0, "tac": 7, "rombank": 0x7F, "rambank": 3, "ramen": 1, "stat_en": 0x78, "lyc": 0x91}
    ram = {0x8000: b"\x01\x02", 0x9FFF: b"\x03", 0xA000: b"\x04", 0xBFFF: b"\x05\x06", 0xDFFE: b"\x07\x08", 0xFDFF: b"\x09\x0A",
           0xFE9F: b"\x0B\x0C", 0xFEFF: b"\x0D", 0xFF01: b"\x0E\x0F", 0xFF7F: b"\x10\x11", 0xFFFE: b"\x12"}
    assert set(vals) | {"ram"} == set(SC.FIELDS)
    p = SC.patch(base, ram=ram, **vals)
    assert SC.fields_of(p) == vals
    assert SC.lcd_of(p) == {**SC.lcd_of(base), "mode": SC.lcd_of(base)["mode"]}, "the LCD block is the oracle's"
    gb = O.GB(rom.rom, p)
    assert gb.save_state() == p
    for addr, data in ram.items():
        for i, b in enumerate(data):
            a = (addr + i) & 0xFFFF
            assert gb.read(a) == b, f"{a:04X}"
    # one field at a time changes that field only
    for k, v in vals.items():
        q = SC.patch(base, **{k: v})
        f0, f1 = SC.fields_of(base), SC.fields_of(q)
        assert f1[k] == v and {x for x in f0 if f0[x] != f1[x]} <= {k}, k
        assert O.GB(rom.rom, q).save_state() == q, k


def test_phases_are_the_oracles():
    """Every LCD phase the cases use was reached by an oracle stopped mid-frame: modes 2, 3, 0 on the
    visible lines and 1 in VBlank, 0 / 4 / 8 cycles (or the nearest even distance that exists) before
    the next event; run_instrs(n) + run_instrs(m) == run_instrs(n + m)."""
    from oracle import oracle as O
    ph = SC.phases(2)
    for ly in (0, 1, 142, 143):
        for mode in (2, 3, 0):
            assert min(k[2] for k in ph if k[:2] == (mode, ly)) <= 10, (mode, ly)
    for ly in (144, 152, 153):
        assert min(k[2] for k in ph if k[:2] == (1, ly)) <= 10, ly
    assert all(left % 2 == 0 for _, _, left in ph)
    rom = ST.stage_rom(2).rom
    a, b = O.GB(rom), O.GB(rom)
    a.power_on(), b.power_on()
    a.run_instrs(700), a.run_instrs(5300)
    b.run_instrs(6000)
    assert a.save_state() == b.save_state() and SC.lcd_of(a.save_state())["ly"] > 0
    assert not SC.lcd_of(SC.lcd_off_state())["lcdc"] & 0x80


def test_case_list():
    cases = SC.all_cases()
    print({k: v for k, v in SC.family_counts().items()}, len(cases))
    assert 600 <= len(cases) <= 1520
    assert {c[1] for c in cases} == {2, 8, 64}


def _sim_summary():
    from tests.hostsim import sim
    L = sim.lib()
    L.pk_sim_summary_enable.argtypes = [ctypes.c_uint32]
    L.pk_sim_summary_get.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
    return L


def _run_all(reverse=False):
    """(failures, {case name: its env's summary row of the first one-frame step, with the passes each
    loop skipped in the first 24-frame step appended as words 8..10}) over every launch."""
    L = _sim_summary()
    bad, rows = [], {}
    for nb in (2, 8, 64):
        for batch in CM.launches(SC.all_cases(), nb, reverse):
            L.pk_sim_summary_enable(len(batch))

            def grab(r, t, batch=batch):
                if t == 0:
                    out = np.zeros((len(batch), 8), np.uint32)
                    L.pk_sim_summary_get(out.ctypes.data, out.size)
                    for i, c in enumerate(batch):
                        rows[c[0]] = out[i] if r == 0 else np.concatenate([rows[c[0]], out[i][:3]])
                # count afresh for the next step (between steps: no kernel is running)
                L.pk_sim_summary_enable(len(batch) if (r, t) == (0, CM.RUNS[0][2] - 1) else 0)

            bad += CM.run_launch(CM.SimAdapter, batch, grab)
    return bad, rows


@pytest.fixture(scope="module")
def default_run():
    return _run_all()


def test_states_match_the_oracle(default_run):
    bad, _ = default_run
    assert not bad, (len(bad), bad[:12])


def _expect_failures(rows, small):
    out = []
    for name, _, _, _, expect in SC.all_cases():
        if not expect:
            continue
        e = {**expect, **expect.get("small", {})} if small else expect
        for k, loop in enumerate(LOOPS):
            if loop in e and bool(rows[name][k]) != e[loop]:
                out.append((name, loop, int(rows[name][k])))
            # "<loop>_first": skipped, or stood aside, in the env's first iteration (the entry condition
            # at the case's own clock; the loop may still skip later in the frame)
            if loop + "_first" in e and bool(rows[name][6] >> k & 1) != e[loop + "_first"]:
                out.append((name, loop + "_first", int(rows[name][6])))
            # "<loop>_24": the passes skipped in the first step of 24 frames, exactly
            if loop + "_24" in e and int(rows[name][8 + k]) != e[loop + "_24"]:
                out.append((name, loop + "_24", int(rows[name][8 + k]), e[loop + "_24"]))
    return out


def test_loop_skip_expectations(default_run):
    """Each case's `expect`: the loop fast path skipped passes in the first frame, or stood aside."""
    _, rows = default_run
    assert _expect_failures(rows, False) == []


def test_census(default_run):
    """Every loop pattern has a case where it skipped and one where it stood aside (among the cases
    that name it), and every front-end outcome was taken in a case's first iteration: interrupt
    dispatch, pending without IME, wake from HALT (executes while halted was set), idle."""
    _, rows = default_run
    cases = {c[0]: c for c in SC.all_cases()}
    for k, loop in enumerate(LOOPS):
        named = [n for n, c in cases.items() if c[4] and loop in c[4]]
        assert any(rows[n][k] for n in named) and any(not rows[n][k] for n in named), loop
    first = {"dispatch": 0, "pending": 0, "wake": 0, "idle": 0, "run": 0}
    for n, c in cases.items():
        f, ev0 = SC.fields_of(c[2]), int(rows[n][4])
        pend = f["ie"] & f["if_"] & 0x1F
        if ev0 & EV_INT:
            first["dispatch"] += 1
            assert pend and f["ime"] and not f["queued"], n
        elif ev0 & EV_IDLE:
            first["pending" if pend and not f["queued"] else "idle"] += 1
            assert f["halted"] or pend, n
        elif f["halted"]:
            first["wake"] += 1
            assert f["queued"] and ev0 & EV_EXEC, n
        else:
            first["run"] += 1
    print(first, {loop: int(sum(bool(rows[n][k]) for n in cases)) for k, loop in enumerate(LOOPS)})
    assert all(first.values()), first


@pytest.mark.slow
def test_states_default_build_reversed():
    """The default build with the env order reversed: other neighbours in every wave."""
    bad, rows = _run_all(reverse=True)
    assert not bad, (len(bad), bad[:12])
    assert _expect_failures(rows, False) == []


@pytest.mark.slow
@pytest.mark.parametrize("lanes", ["16", "32"])
def test_states_small_lds_kernel(lanes, monkeypatch):
    """The same cases through the small-LDS K1 (PK_K1_SMALL: bank 0 and 1 staged only), 16 and 32
    envs per wave, env order reversed."""
    monkeypatch.setenv("PK_K1_SMALL", "1")
    monkeypatch.setenv("PK_WAVE_LANES", lanes)
    monkeypatch.setenv("PK_K1_BLOCK", "256")
    bad, rows = _run_all(reverse=True)
    assert not bad, (len(bad), bad[:12])
    assert _expect_failures(rows, True) == []


@pytest.mark.slow
@pytest.mark.parametrize("small", [False, True], ids=["default", "small_lds"])
def test_states_under_sanitizers(small, tmp_path):
    """Every case through tests/hostsim/states_main.cpp — the host-simulation sources linked into a
    program of their own with the address and undefined-behaviour sanitizers — as a child process:
    both runs of every case (3 one-frame steps, 2 steps of 24 frames).  The
    sanitizers must report nothing (any report aborts the program)."""
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim")
    subprocess.run(["make", "-s", "-C", here, "states_asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for k in ("PK_K1_SMALL", "PK_WAVE_LANES", "PK_K1_BLOCK"):
        env.pop(k, None)
    if small:
        env.update(PK_K1_SMALL="1", PK_WAVE_LANES="32", PK_K1_BLOCK="256")
    for nb in (2, 8, 64):
        rom = ST.stage_rom(nb).rom
        for k, batch in enumerate(CM.launches(SC.all_cases(), nb)):
            for fs, rel, steps in CM.RUNS:
                path = tmp_path / f"cases_{nb}_{k}_{fs}.bin"
                with open(path, "wb") as f:
                    f.write(struct.pack("<5I", len(rom), len(batch), fs, rel, steps))
                    f.write(rom)
                    for c in batch:
                        f.write(c[2])
                r = subprocess.run([os.path.join(here, "build", "states_asan"), str(path)], env=env,
                                   capture_output=True, text=True, timeout=1500)
                assert r.returncode == 0 and not r.stderr.strip(), (nb, k, fs, r.returncode, r.stderr[-3000:])
                os.unlink(path)
