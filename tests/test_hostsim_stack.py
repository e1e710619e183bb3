"""Frame stack (pk_fstack_*) on the CPU: the unmodified kernel and C ABI in the host-simulation build
(tests/hostsim).  The scenarios and the model live in stack_common.py; the gfx950 build runs them in
test_gpu_stack.py (-m gpu)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hostsim"))
sys.path.insert(0, HERE)

import stack_common as sc  # noqa: E402
from emulator import HostsimEmulator  # noqa: E402
from pokegym_amd.testrom.game import game_rom  # noqa: E402
from test_hostsim_archive import _NoStream  # noqa: E402


def make(n, **kw):
    # 4 frames per step: nothing here depends on the step's length
    return HostsimEmulator(game_rom(), n, frame_skip=4, release_frame=2, **kw)


def dev(values, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(values, dtype))


def make_env(reward=True, max_episode_steps=5, **kw):
    from pokegym_amd.env import VecEnv
    emu = make(128, reward=reward, max_episode_steps=max_episode_steps)
    return VecEnv(48, emulator=emu, batch_size=24, log_interval=0, **kw)


@pytest.fixture
def no_streams(monkeypatch):
    for name in ("Stream", "Event", "current_stream", "stream"):
        monkeypatch.setattr(torch.cuda, name, _NoStream)
    monkeypatch.setattr(torch.Tensor, "record_stream", lambda self, s: None)


def test_model_random_bytes():
    sc.check_model(make, dev)


def test_rounding_and_edges():
    sc.check_edges(make, dev)


def test_reference_frames():
    sc.check_reference_frames(make, dev)


def test_fill_push_fill_only():
    sc.check_fill_push(make, dev)


def test_ranges():
    sc.check_ranges(make, dev)


def test_screen_source():
    sc.check_screen_source(make, dev)


def test_guards():
    sc.check_guards(make, dev)


def test_with_emulator():
    sc.check_with_emulator(make, dev)


@pytest.mark.parametrize("layout", ["chw", "hwc"])
def test_vecenv_step(no_streams, layout):
    sc.check_vecenv_step(make_env, dev, layout)


def test_vecenv_recv_send(no_streams):
    sc.check_vecenv_pipeline(make_env, dev)


def test_vecenv_bank(no_streams):
    sc.check_vecenv_bank(make_env, dev)


def test_vecenv_off_and_bad_keywords(no_streams):
    from pokegym_amd.env import VecEnv
    sc.check_vecenv_off(make_env, dev)
    for bad in sc.BAD_KEYWORDS:
        emu = make(64)
        with pytest.raises(ValueError):
            VecEnv(64, emulator=emu, log_interval=0, reward=False, **bad)
        emu.close()
    emu = make(64, render=False)
    with pytest.raises(ValueError):
        VecEnv(64, emulator=emu, log_interval=0, reward=False, frame_stack=4)
    emu.close()


def test_abi():
    """ABI 12 still, and the built gfx950 library and the host-simulation build export the names."""
    import sim
    from pokegym_amd import _native, build
    names = ("pk_fstack_create", "pk_fstack_depth", "pk_fstack_scale", "pk_fstack_ptr", "pk_fstack_push")
    assert _native.ABI_VERSION == 12
    for lib in (ctypes.CDLL(build.build()), sim.lib()):
        assert lib.pk_abi_version() == 12
        assert all(hasattr(lib, name) for name in names)
    assert set(names) <= set(_native.EXPORTS)
    assert (_native.PK_FSTACK_CHW, _native.PK_FSTACK_HWC, _native.PK_FSTACK_MEAN, _native.PK_FSTACK_PICK,
            _native.PK_FSTACK_FILL_ONLY) == (0, 1, 0, 1, 1)
