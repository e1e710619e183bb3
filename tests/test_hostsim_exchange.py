"""The archive exchange (pk_archive_pack / pk_archive_merge, ABI v11) on the CPU: the unmodified
kernels and C ABI in the host-simulation build (tests/hostsim).  The scenarios and the model live in
exchange_common.py; the gfx950 build runs them in test_gpu_exchange.py (-m gpu)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hostsim"))
sys.path.insert(0, HERE)

import archive_common as ac  # noqa: E402
import exchange_common as xc  # noqa: E402
from emulator import HostsimEmulator  # noqa: E402
from pokegym_amd.testrom.game import game_rom  # noqa: E402
from test_hostsim_archive import _NoStream  # noqa: E402


def make(n, **kw):
    # 4 frames per step, as in test_hostsim_archive: nothing here depends on the step's length
    return HostsimEmulator(game_rom(), n, frame_skip=4, release_frame=2, **kw)


def dev(values, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(values, dtype))


def test_clone(monkeypatch):
    xc.check_clone(make, dev, lambda v: monkeypatch.setenv("PK_ILV", v))


def test_merge_model():
    xc.check_merge_model(make, dev)


def test_capacity():
    xc.check_capacity(make, dev)


def test_delta():
    xc.check_delta(make, dev)


def test_determinism():
    xc.check_determinism(make, dev)


def test_guards():
    xc.check_guards(make, dev)


def test_vecenv(monkeypatch):
    from pokegym_amd.env import VecEnv
    import pytest
    for name in ("Stream", "Event", "current_stream", "stream"):
        monkeypatch.setattr(torch.cuda, name, _NoStream)
    envs = [VecEnv(48, emulator=make(128, reward=True, max_episode_steps=ac.MAX_STEPS), batch_size=24, log_interval=0,
                   bank_episodes=True, archive_cells=8, archive_exchange=True) for _ in range(2)]
    xc.check_vecenv(envs[0], envs[1], dev)
    with pytest.raises(ValueError):
        VecEnv(4, emulator=make(4, reward=True), log_interval=0, bank_slots=1, bank_episodes=True, archive_exchange=True)
    plain = VecEnv(4, emulator=make(4, reward=True), log_interval=0, bank_episodes=True, archive_cells=2)
    for call in (plain.archive_export, plain.archive_sync, lambda: plain.archive_import({})):
        with pytest.raises(RuntimeError):
            call()
    for v in envs:
        v.emu.close()
