"""The exploration archive on the savestate bank (pk_archive_*, ABI v9) on the MI355X, through
BatchedEmulator and VecEnv: the scenarios of archive_common.py, which test_hostsim_archive.py runs
on the CPU.  The tests only copy state, do table bookkeeping and step a known-good ROM."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)


def make(n, **kw):
    from pokegym_amd.emulator import BatchedEmulator
    from pokegym_amd.testrom.game import game_rom
    return BatchedEmulator(game_rom(), n, **kw)


def dev(values, dtype=np.int32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(values, dtype)).cuda()


@pytest.mark.parametrize("ilv", ["32", "16"])
def test_model_parity(ilv, monkeypatch):
    import archive_common as ac
    monkeypatch.setenv("PK_ILV", ilv)
    ac.check_model_parity(make, dev)


def test_capacity():
    import archive_common as ac
    ac.check_capacity(make, dev)


def test_continuation():
    import archive_common as ac
    ac.check_continuation(make, dev)


def test_determinism():
    import archive_common as ac
    ac.check_determinism(make, dev)


@pytest.mark.parametrize("ilv", ["64", "32", "16"])
def test_cell_keys(ilv, monkeypatch):
    import archive_common as ac
    monkeypatch.setenv("PK_ILV", ilv)
    ac.check_cell_keys(make, dev)


def test_guards():
    import archive_common as ac
    ac.check_guards(make, dev)


def test_ranges_on_two_streams():
    """update over range 0 on one stream, then over range 64 on another, ordered by an event,
    equals one call over both."""
    import torch
    import archive_common as ac

    def streams(first, second):
        s1, s2, ev = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Event()
        cur = torch.cuda.current_stream()
        s1.wait_stream(cur)
        s2.wait_stream(cur)
        with torch.cuda.stream(s1):
            first()
            ev.record(s1)
        with torch.cuda.stream(s2):
            s2.wait_event(ev)
            second()
        cur.wait_stream(s1)
        cur.wait_stream(s2)

    ac.check_ranges(make, dev, streams)


def test_vecenv():
    import archive_common as ac
    from pokegym_amd.env import VecEnv
    from pokegym_amd.testrom.game import game_rom
    env = VecEnv(48, rom=game_rom(), power_on=True, batch_size=24, max_episode_steps=ac.MAX_STEPS, log_interval=0,
                 bank_episodes=True, archive_cells=8)
    assert env.emu.n == 128 and env.emu.bank_slots == 8 and env.emu.archive_cells == 8
    ac.check_vecenv(env, dev)
    env.close()
