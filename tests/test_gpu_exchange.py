"""The archive exchange (pk_archive_pack / pk_archive_merge, ABI v11) on the MI355X, through
BatchedEmulator and VecEnv: the scenarios of exchange_common.py, which test_hostsim_exchange.py runs
on the CPU.  Two handles in one process on one device; the tests only copy state, do table
bookkeeping and step a known-good ROM."""
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


def test_clone(monkeypatch):
    import exchange_common as xc
    xc.check_clone(make, dev, lambda v: monkeypatch.setenv("PK_ILV", v))


def test_merge_model():
    import exchange_common as xc
    xc.check_merge_model(make, dev)


def test_capacity():
    import exchange_common as xc
    xc.check_capacity(make, dev)


def test_delta():
    import exchange_common as xc
    xc.check_delta(make, dev)


def test_determinism():
    import exchange_common as xc
    xc.check_determinism(make, dev)


def test_guards():
    import exchange_common as xc
    xc.check_guards(make, dev)


def test_vecenv():
    import archive_common as ac
    import exchange_common as xc
    from pokegym_amd.env import VecEnv
    from pokegym_amd.testrom.game import game_rom
    envs = [VecEnv(48, rom=game_rom(), power_on=True, batch_size=24, max_episode_steps=ac.MAX_STEPS, log_interval=0,
                   bank_episodes=True, archive_cells=8, archive_exchange=True) for _ in range(2)]
    xc.check_vecenv(envs[0], envs[1], dev)
    for v in envs:
        v.close()
