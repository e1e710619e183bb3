"""Episode checkpoints in the savestate bank (pk_bank_checkpoint / pk_bank_resume, ABI v8) on the
CPU: the unmodified kernels and C ABI in the host-simulation build (tests/hostsim).  The scenarios
live in episodes_common.py; the gfx950 build runs them in test_gpu_episodes.py (-m gpu)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hostsim"))
sys.path.insert(0, HERE)

import episodes_common as ec  # noqa: E402
from emulator import HostsimEmulator  # noqa: E402
from pokegym_amd.testrom.game import game_rom  # noqa: E402


def make(n, **kw):
    # 4 frames per step: the host simulation spends its time in K1, and nothing here depends on
    # the step's length (the GPU tests run the default 24)
    return HostsimEmulator(game_rom(), n, frame_skip=4, release_frame=2, **kw)


def dev(values, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(values, dtype))


def every_step_reports(n):
    """Handles whose every step builds the info record (max_episode_steps = 1).  The benchmark ROM
    has an empty party until its map is built, which the record refuses (PK_ERR_EMPTY_PARTY), so
    the game runs 12 steps first; the reset after them reloads nothing (not the envs' first)."""
    sc = ec.Script(12, n, 1, dev)
    emu = make(n, reward=True, max_episode_steps=ec.MAX_STEPS)
    emu.reset()
    for t in range(12):
        sc.step(emu, t)
    emu.set_episode_params(1, 4.0)
    emu.reset()
    return emu


@pytest.mark.parametrize("ilv", ["64", "32", "16", "1"])
def test_twin_continuation(ilv, monkeypatch):
    """A resumed env fed the source's actions returns the source's rewards, dones, observations,
    info records and machine state at every step, across the episode's end; the never-reset
    destination (seen tag 0) takes tag 1; envs taking no part equal a twin that never resumed."""
    monkeypatch.setenv("PK_ILV", ilv)
    ec.check_twin_continuation(make, dev)


def test_plain_load_does_not_continue():
    ec.check_control(make, dev)


def test_rejects_and_guards():
    ec.check_rejects(make, dev)


def test_stale_word_with_the_destinations_tag_is_cleared():
    """The destination has live entries under its current tag at positions where the source has
    none: after the resume they are gone.  max_episode_steps = 1 makes every step build the info
    record, whose exploration term is 0.02 * len(seen_coords)."""
    n, src, dst = 64, 0, 41
    sc = ec.Script(12, n, 8, dev)
    emu = every_step_reports(n)
    ref = every_step_reports(n)                          # what env src returns without any bank call
    emu.bank_create(1)
    emu.bank_enable_episodes()
    for h in (emu, ref):
        sc.step(h, 0)
    emu.bank_checkpoint(dev(ec.slot_map({src: 0}, n)))
    at_checkpoint = float(emu.info[ec.EXPLORATION, src])
    for t in range(1, 9):
        sc.step(emu, t)
    assert float(emu.info[ec.EXPLORATION, dst]) >= at_checkpoint + 4 * 0.02 > 0.0   # dst's own entries
    emu.bank_resume(dev(ec.slot_map({dst: 0}, n)))
    for t in range(1, 4):
        sc.step(ref, t)
        sc.copy_rows(8 + t, [dst], sc, t, [src])
        sc.step(emu, 8 + t)
        assert emu.info_flag[dst] == 1 and ref.info_flag[src] == 1 and emu.errors[dst] == 0
        assert float(emu.info[ec.EXPLORATION, dst]) == float(ref.info[ec.EXPLORATION, src]), t
        assert emu.rewards[dst] == ref.rewards[src], t
        assert torch.equal(emu.obs[dst], ref.obs[src]), t
    emu.close()
    ref.close()


def test_checkpoint_after_the_tag_wraps():
    """255 further resets take a source's seen tag from 1 through 255 back to 1 (the table is
    cleared at the wrap); a checkpoint and resume after that still continues exactly."""
    n, src, dst = 64, 7, 50
    sc = ec.Script(9, n, 12, dev)
    emu = every_step_reports(n)
    emu.bank_create(1)
    emu.bank_enable_episodes()
    only = ec.masked((src,), dev, n)
    for k in range(255):
        if k in (100, 253, 254):     # entries under tags 101, 254 and 255 stay behind in the table
            sc.step(emu, 0)
        emu.reset(only)
    sc.step(emu, 1)
    sc.step(emu, 2)
    emu.bank_checkpoint(dev(ec.slot_map({src: 0}, n)))
    rec = []
    for t in range(3, 6):
        sc.step(emu, t)
        rec.append(ec.outputs(emu, [src]))
    emu.bank_resume(dev(ec.slot_map({dst: 0}, n)))
    assert emu.bank_rejects() == 0
    for t in range(3, 6):
        sc.copy_rows(3 + t, [dst], sc, t, [src])
        sc.step(emu, 3 + t)
        ec.same(ec.outputs(emu, [dst]), rec[t - 3], ("after the wrap", t))
        assert rec[t - 3]["flag"][0] == 1 and rec[t - 3]["info"][ec.EXPLORATION, 0] > 0.0
    emu.close()


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


def test_vecenv_fork(monkeypatch):
    from pokegym_amd.env import VecEnv
    for name in ("Stream", "Event", "current_stream", "stream"):
        monkeypatch.setattr(torch.cuda, name, _NoStream)
    emu = make(128, reward=True, max_episode_steps=ec.MAX_STEPS)
    env = VecEnv(48, emulator=emu, batch_size=24, log_interval=0, bank_slots=1, bank_episodes=True, fork_slots=3)
    assert emu.bank_slots == 4 and emu.bank_has_episodes
    ec.check_fork(env, dev)
    emu.close()


def test_vecenv_pool_slots_travel(monkeypatch):
    for name in ("Stream", "Event", "current_stream", "stream"):
        monkeypatch.setattr(torch.cuda, name, _NoStream)
    ec.check_pool_slots(make, dev)


def test_vecenv_without_episodes_allocates_nothing():
    from pokegym_amd.env import VecEnv
    emu = make(4, reward=True)
    env = VecEnv(4, emulator=emu, log_interval=0, bank_slots=2)
    assert emu.bank_slots == 2 and not emu.bank_has_episodes
    with pytest.raises(RuntimeError):
        env.checkpoint_to_bank([0], [0])
    with pytest.raises(RuntimeError):
        env.fork([1], [0])
    with pytest.raises(ValueError):
        VecEnv(4, emulator=make(4, reward=False), log_interval=0, bank_slots=2, bank_episodes=True)
    with pytest.raises(ValueError):
        VecEnv(4, emulator=make(4, reward=True), log_interval=0, bank_episodes=True)
    env.close()
