"""Episode checkpoints in the savestate bank (pk_bank_checkpoint / pk_bank_resume, ABI v8) on the
MI355X, through BatchedEmulator and VecEnv: the scenarios of episodes_common.py, which
test_hostsim_episodes.py runs on the CPU.  The tests only copy state and step a known-good ROM."""
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
def test_twin_continuation(ilv, monkeypatch):
    """A resumed env fed the source's inputs returns the source's rewards, dones, observations,
    info records and machine state at every step, across the episode's end; the destinations
    hold live entries of their own tags, one was never reset (tag 0); envs taking no part equal
    a twin handle that never resumed."""
    import episodes_common as ec
    monkeypatch.setenv("PK_ILV", ilv)
    ec.check_twin_continuation(make, dev)


def test_plain_load_does_not_continue():
    import episodes_common as ec
    ec.check_control(make, dev)


def test_rejects_and_guards():
    import episodes_common as ec
    ec.check_rejects(make, dev)


def test_ranges_on_two_streams():
    """Checkpoint the envs of range 0 on one stream and resume envs of range 64 from those slots on
    another, ordered by an event: the result is the single-stream result."""
    import torch
    import episodes_common as ec
    n = ec.N
    sc = ec.Script(8, n, 21, dev)
    ck = dev(ec.slot_map({0: 0, 31: 1, 63: 2}))
    rs = dev(ec.slot_map({64: 0, 66: 2, 69: 1, 5: 0}))      # env 5 lies outside the resumed range
    outs = []
    for two in (False, True):
        emu = make(n, reward=True, max_episode_steps=ec.MAX_STEPS)
        emu.bank_create(3)
        emu.bank_enable_episodes()
        emu.reset()
        for t in range(4):
            sc.step(emu, t)
        if two:
            s1, s2, ev = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Event()
            cur = torch.cuda.current_stream()
            s1.wait_stream(cur)
            s2.wait_stream(cur)
            with torch.cuda.stream(s1):
                emu.bank_checkpoint(ck, 0, 64)
                ev.record(s1)
            with torch.cuda.stream(s2):
                s2.wait_event(ev)
                emu.bank_resume(rs, 64, n - 64)
            cur.wait_stream(s1)
            cur.wait_stream(s2)
        else:
            emu.bank_checkpoint(ck, 0, 64)
            emu.bank_resume(rs, 64, n - 64)
        assert emu.bank_rejects() == 0
        snap = emu.snapshot_range(0, n)
        assert bytes(snap[64]) == bytes(snap[0]) and bytes(snap[69]) == bytes(snap[31]) and bytes(snap[5]) != bytes(snap[0])
        for t in range(4, 8):
            sc.copy_rows(t, [64, 66, 69], sc, t, [0, 63, 31])
            sc.step(emu, t)
        outs.append(ec.outputs(emu, range(n)))
        assert torch.equal(emu.rewards[[64, 66, 69]], emu.rewards[[0, 63, 31]])
        assert torch.equal(emu.obs[[64, 66, 69]], emu.obs[[0, 63, 31]])
        emu.close()
    ec.same(outs[0], outs[1], "two streams")


def test_vecenv_fork():
    """fork() between the two sub-batches of a VecEnv(48, batch_size=24) in padded 64-env slots."""
    import episodes_common as ec
    from pokegym_amd.env import VecEnv
    from pokegym_amd.testrom.game import game_rom
    env = VecEnv(48, rom=game_rom(), power_on=True, batch_size=24, max_episode_steps=ec.MAX_STEPS, log_interval=0,
                 bank_slots=1, bank_episodes=True, fork_slots=3)
    assert env.emu.n == 128 and env.emu.bank_slots == 4 and env.emu.bank_has_episodes
    ec.check_fork(env, dev)
    env.close()


def test_vecenv_pool_slots_travel():
    """Start slots, episode return and length through resume, fork and the archive in padded sub-batches."""
    import episodes_common as ec
    ec.check_pool_slots(make, dev)
