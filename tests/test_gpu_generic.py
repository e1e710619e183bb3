"""Generic episode parts (pk_bank_enable_generic_episodes) on the MI355X, through BatchedEmulator and
VecEnv: the scenarios of generic_common.py, which test_hostsim_generic.py runs on the CPU."""
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
    # 4 frames per step: nothing here depends on the step's length
    return BatchedEmulator(game_rom(), n, frame_skip=4, release_frame=2, **kw)


def dev(values, dtype=np.int32):
    import torch
    return torch.from_numpy(np.array(values, dtype)).cuda()


def test_guards():
    import generic_common as gc
    gc.check_guards(make, dev)


@pytest.mark.parametrize("stack", [(2, 4, "hwc"), (4, 3, "chw")], ids=lambda s: "s%dD%d%s" % s)
def test_continuation(stack):
    import generic_common as gc
    gc.check_continuation(make, dev, gc.PROBES | gc.STACK, stack)


def test_newmax_keeps_its_maximum():
    import generic_common as gc
    gc.check_newmax(make, dev)


@pytest.mark.parametrize("parts", [1, 0])
def test_only_what_was_asked(parts):
    import generic_common as gc
    gc.check_continuation(make, dev, parts, gc.STACKS[1])


def test_archive():
    import generic_common as gc
    gc.check_archive(make, dev)


def test_trajectories_in_both_orders():
    import generic_common as gc
    gc.check_traj_orders(make, dev)


def test_vecenv():
    import generic_common as gc
    gc.check_vecenv(make, dev)


def test_vecenv_padded_sub_batches():
    import generic_common as gc
    gc.check_vecenv_padded(make, dev)


def test_vecenv_errors_and_the_old_refill():
    import generic_common as gc
    gc.check_vecenv_errors(make, dev)


def test_abi():
    from pokegym_amd import _native
    lib = _native.load()
    assert lib.pk_abi_version() == _native.ABI_VERSION == 12
    for name in ("pk_bank_enable_generic_episodes", "pk_bank_generic_parts", "pk_bank_generic_episode_bytes"):
        assert hasattr(lib, name)
