"""The exploration archive on the savestate bank (pk_archive_*, ABI v9) on the CPU: the unmodified
kernels and C ABI in the host-simulation build (tests/hostsim).  The scenarios and the model live in
archive_common.py; the gfx950 build runs them in test_gpu_archive.py (-m gpu)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hostsim"))
sys.path.insert(0, HERE)

import archive_common as ac  # noqa: E402
from emulator import HostsimEmulator  # noqa: E402
from pokegym_amd.testrom.game import game_rom  # noqa: E402


class _NoStream:
    """CPU stand-in for the HIP streams/events of VecEnv's sub-batch pipeline."""
    def __init__(self, *a, **k):
        pass

    def wait_stream(self, other):
        pass

    def wait_event(self, ev):
        pass

    def record(self, stream=None):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def make(n, **kw):
    # 4 frames per step, as in test_hostsim_episodes: nothing here depends on the step's length
    return HostsimEmulator(game_rom(), n, frame_skip=4, release_frame=2, **kw)


def dev(values, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(values, dtype))


@pytest.mark.parametrize("ilv", ["32", "16"])
def test_model_parity(ilv, monkeypatch):
    monkeypatch.setenv("PK_ILV", ilv)
    ac.check_model_parity(make, dev)


def test_capacity():
    ac.check_capacity(make, dev)


def test_continuation():
    ac.check_continuation(make, dev)


def test_determinism():
    ac.check_determinism(make, dev)


@pytest.mark.parametrize("ilv", ["64", "32", "16"])
def test_cell_keys(ilv, monkeypatch):
    monkeypatch.setenv("PK_ILV", ilv)
    ac.check_cell_keys(make, dev)


def test_guards():
    ac.check_guards(make, dev)


def test_ranges():
    ac.check_ranges(make, dev)


def test_vecenv(monkeypatch):
    from pokegym_amd.env import VecEnv
    for name in ("Stream", "Event", "current_stream", "stream"):
        monkeypatch.setattr(torch.cuda, name, _NoStream)
    emu = make(128, reward=True, max_episode_steps=ac.MAX_STEPS)
    env = VecEnv(48, emulator=emu, batch_size=24, log_interval=0, bank_episodes=True, archive_cells=8)
    assert emu.bank_slots == 8 and emu.archive_cells == 8
    ac.check_vecenv(env, dev)
    with pytest.raises(ValueError):
        VecEnv(4, emulator=make(4, reward=True), log_interval=0, bank_slots=1, archive_cells=2)
    plain = VecEnv(4, emulator=make(4, reward=True), log_interval=0, bank_slots=1, bank_episodes=True)
    with pytest.raises(RuntimeError):
        plain.archive_update()
    emu.close()
