"""Action trajectories (pk_traj_*, ABI v10) on the CPU: the unmodified kernels and C ABI in the
host-simulation build (tests/hostsim).  The scenarios live in traj_common.py; the gfx950 build runs
them in test_gpu_traj.py (-m gpu)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hostsim"))
sys.path.insert(0, HERE)

import traj_common as tc  # noqa: E402
from emulator import HostsimEmulator  # noqa: E402
from pokegym_amd.testrom.game import game_rom  # noqa: E402
from test_hostsim_episodes import _NoStream  # noqa: E402


def make(n, frame_skip=2, release_frame=1, **kw):
    # 2 frames per step: the host simulation spends its time in K1, and nothing here depends on
    # the step's length (the GPU tests run the default 24)
    return HostsimEmulator(game_rom(), n, frame_skip=frame_skip, release_frame=release_frame, **kw)


def dev(values, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(values, dtype))


@pytest.mark.parametrize("ilv", ["32", "1"])
def test_recording(ilv, monkeypatch):
    """trajectories() equals the list model — origin, length, flags, action bytes, 0xFF past the
    length — after steps and masked resets from the template, valid slots and a rejected slot."""
    monkeypatch.setenv("PK_ILV", ilv)
    tc.check_recording(make, dev)


def test_travel():
    """A resumed env's trajectory is the source's at the checkpoint plus its own later actions; slots
    hold the source's; non-participants and rejected envs equal a twin handle's."""
    tc.check_travel(make, dev)


def test_replay_oracle():
    tc.check_replay(make, dev)


def test_flags():
    tc.check_flags(make, dev)


def test_overflow():
    tc.check_overflow(make, dev)


def test_archive():
    tc.check_archive(make, dev)


def test_guards():
    tc.check_guards(make, dev)


def test_vecenv_fork(monkeypatch):
    from pokegym_amd.env import VecEnv
    for name in ("Stream", "Event", "current_stream", "stream"):
        monkeypatch.setattr(torch.cuda, name, _NoStream)
    emu = make(128, reward=True, max_episode_steps=tc.MAX_STEPS)
    env = VecEnv(48, emulator=emu, batch_size=24, log_interval=0, bank_slots=1, bank_episodes=True, fork_slots=3,
                 record_trajectories=True)
    assert emu.traj_capacity == tc.CAP
    tc.check_fork(env, dev)
    emu.close()


def test_vecenv_archive_trajectory():
    from pokegym_amd.env import VecEnv
    seed = make(2)
    seed.poke(0, 0xD361, bytes([2, 3]))
    seed.poke(1, 0xD361, bytes([4, 5]))
    pool = [seed.snapshot(0), seed.snapshot(1)]
    seed.close()
    emu = make(tc.N, reward=True, reload_on_reset=True, max_episode_steps=tc.MAX_STEPS)
    env = VecEnv(tc.N, emulator=emu, log_interval=0, state_pool=pool, bank_slots=1, bank_episodes=True, archive_cells=6,
                 record_trajectories=True)
    tc.check_archive_vecenv(env, make, dev)
    emu.close()


def test_vecenv_without_trajectories_records_nothing():
    from pokegym_amd.env import VecEnv
    emu = make(4, reward=True)
    env = VecEnv(4, emulator=emu, log_interval=0, bank_slots=2, bank_episodes=True)
    assert emu.traj_capacity == 0
    with pytest.raises(RuntimeError):
        env.trajectory(0)
    with pytest.raises(RuntimeError):
        env.slot_trajectory(0)
    env.close()
