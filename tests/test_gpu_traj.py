"""Action trajectories (pk_traj_*, ABI v10) on the MI355X, through BatchedEmulator and VecEnv: the
scenarios of traj_common.py, which test_hostsim_traj.py runs on the CPU.  The tests only record,
copy and replay actions on a known-good ROM."""
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


def two_streams(first, second):
    """The two closures on two streams, both ordered after the current stream and joined into it."""
    import torch
    s1, s2, cur = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.current_stream()
    s1.wait_stream(cur)
    s2.wait_stream(cur)
    with torch.cuda.stream(s1):
        first()
    with torch.cuda.stream(s2):
        second()
    cur.wait_stream(s1)
    cur.wait_stream(s2)


@pytest.mark.parametrize("ilv", ["32", "16"])
def test_recording(ilv, monkeypatch):
    """trajectories() equals the list model — origin, length, flags, action bytes, 0xFF past the
    length — after steps and masked resets from the template, valid slots and a rejected slot,
    issued as two sub-batch ranges on two streams."""
    import traj_common as tc
    monkeypatch.setenv("PK_ILV", ilv)
    tc.check_recording(make, dev, par=two_streams)


def test_travel():
    """A resumed env's trajectory is the source's at the checkpoint (lengths 0, 1, 15, 16, 17, 33)
    plus its own later actions; slots hold the source's; non-participants and rejected envs equal a
    twin handle's."""
    import traj_common as tc
    tc.check_travel(make, dev)


def test_replay_oracle():
    """replay() of recorded trajectories on a second handle rebuilds the recorded envs' machine state
    bit for bit, and the rebuilt episodes continue with the originals' rewards, dones, obs and info."""
    import traj_common as tc
    tc.check_replay(make, dev)


def test_flags():
    import traj_common as tc
    tc.check_flags(make, dev)


def test_overflow():
    import traj_common as tc
    tc.check_overflow(make, dev)


def test_archive():
    import traj_common as tc
    tc.check_archive(make, dev)


def test_guards():
    import traj_common as tc
    tc.check_guards(make, dev)


def test_vecenv_fork():
    """fork() between the two sub-batches of a VecEnv(48, batch_size=24) in padded 64-env slots."""
    import traj_common as tc
    from pokegym_amd.env import VecEnv
    from pokegym_amd.testrom.game import game_rom
    env = VecEnv(48, rom=game_rom(), power_on=True, batch_size=24, max_episode_steps=tc.MAX_STEPS, log_interval=0,
                 bank_slots=1, bank_episodes=True, fork_slots=3, record_trajectories=True)
    assert env.emu.n == 128 and env.emu.traj_capacity == tc.CAP
    tc.check_fork(env, dev)
    env.close()


def test_vecenv_archive_trajectory():
    import traj_common as tc
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
    env.close()
