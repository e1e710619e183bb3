"""Generic episode parts (pk_bank_enable_generic_episodes) on the CPU: the unmodified kernels and C ABI
in the host-simulation build (tests/hostsim).  The scenarios live in generic_common.py; the gfx950
build runs them in test_gpu_generic.py (-m gpu)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hostsim"))
sys.path.insert(0, HERE)

import generic_common as gc  # noqa: E402
from emulator import HostsimEmulator  # noqa: E402
from pokegym_amd.testrom.game import game_rom  # noqa: E402
from test_hostsim_archive import _NoStream  # noqa: E402


def make(n, **kw):
    # 4 frames per step: nothing here depends on the step's length
    return HostsimEmulator(game_rom(), n, frame_skip=4, release_frame=2, **kw)


def dev(values, dtype=np.int32):
    return torch.from_numpy(np.array(values, dtype))


@pytest.fixture
def no_streams(monkeypatch):
    for name in ("Stream", "Event", "current_stream", "stream"):
        monkeypatch.setattr(torch.cuda, name, _NoStream)
    monkeypatch.setattr(torch.Tensor, "record_stream", lambda self, s: None)


def test_guards():
    gc.check_guards(make, dev)


@pytest.mark.parametrize("stack", gc.STACKS, ids=lambda s: "s%dD%d%s" % s)
def test_continuation(stack):
    gc.check_continuation(make, dev, gc.PROBES | gc.STACK, stack)


def test_newmax_keeps_its_maximum():
    gc.check_newmax(make, dev)


@pytest.mark.parametrize("parts", [gc.PROBES, 0])
def test_only_what_was_asked(parts):
    gc.check_continuation(make, dev, parts, gc.STACKS[1])


def test_archive():
    gc.check_archive(make, dev)


def test_trajectories_in_both_orders():
    gc.check_traj_orders(make, dev)


def test_vecenv(no_streams):
    gc.check_vecenv(make, dev)


def test_vecenv_padded_sub_batches(no_streams):
    gc.check_vecenv_padded(make, dev)


def test_vecenv_errors_and_the_old_refill(no_streams):
    gc.check_vecenv_errors(make, dev)


def test_abi():
    """ABI 12 still, and the built gfx950 library and the host-simulation build export the names."""
    import sim
    from pokegym_amd import _native, build
    names = ("pk_bank_enable_generic_episodes", "pk_bank_generic_parts", "pk_bank_generic_episode_bytes")
    assert _native.ABI_VERSION == 12 and (_native.PK_GEP_PROBES, _native.PK_GEP_STACK) == (1, 2)
    for lib in (ctypes.CDLL(build.build()), sim.lib()):
        assert lib.pk_abi_version() == 12
        assert all(hasattr(lib, name) for name in names)
    assert set(names) <= set(_native.EXPORTS)
