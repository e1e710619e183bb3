"""Visit counts (pk_counts_*) on the MI355X, through BatchedEmulator and VecEnv: the scenarios of
counts_common.py, which test_hostsim_counts.py runs on the CPU.  The tests count keys they build
themselves and step a known-good ROM."""
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
    return BatchedEmulator(game_rom(), n, frame_skip=4, release_frame=2, **kw)


def dev(values, dtype=np.int32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(values, dtype)).cuda()


def make_env(num, batch_size, **kw):
    from pokegym_amd.env import VecEnv
    emu = make(num if batch_size is None else num // batch_size * 64, max_episode_steps=5)
    return VecEnv(num, emulator=emu, batch_size=batch_size, log_interval=0, **kw)


def test_model_equality():
    import counts_common as cc
    cc.check_model_equality(make, dev)


def test_ranges_mask_nokey():
    import counts_common as cc
    cc.check_ranges(make, dev)


def test_full_table():
    import counts_common as cc
    cc.check_full_table(make, dev)


def test_peek():
    import counts_common as cc
    cc.check_peek(make, dev)


def test_pack_add():
    import counts_common as cc
    cc.check_pack_add(make, dev)


def test_guards():
    import counts_common as cc
    cc.check_guards(make, dev)


def test_run_to_run():
    import counts_common as cc
    cc.check_run_to_run(make, dev)


def test_vecenv():
    import counts_common as cc
    cc.check_vecenv(make_env, dev)


def test_vecenv_ram_keys():
    import counts_common as cc
    cc.check_vecenv_ram_keys(make_env, dev)


def test_abi():
    import counts_common as cc
    from pokegym_amd import _native
    lib = _native.load()
    assert lib.pk_abi_version() == _native.ABI_VERSION == 12
    for name in cc.EXPORTS:
        assert hasattr(lib, name), name
