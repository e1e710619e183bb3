"""RAM probes (pk_probe_*) on the CPU: the unmodified kernel and C ABI in the host-simulation build
(tests/hostsim).  The scenarios live in probes_common.py, the model in pokegym_amd/probes.py; the
gfx950 build runs them in test_gpu_probes.py (-m gpu)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hostsim"))
sys.path.insert(0, HERE)

import probes_common as pc  # noqa: E402
from emulator import HostsimEmulator  # noqa: E402
from pokegym_amd.testrom.game import game_rom  # noqa: E402
from test_hostsim_archive import _NoStream  # noqa: E402

# PK_ILV: the handle's own interleave, and the image's lane interleave forced to 1, 16 and 64
ILVS = [None, "1", "16", "64"]


def make(n, **kw):
    # 4 frames per step: nothing here depends on the step's length
    return HostsimEmulator(game_rom(), n, frame_skip=4, release_frame=2, **kw)


def dev(values, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(values, dtype))


def make_env(reward=True, max_episode_steps=1000, **kw):
    from pokegym_amd.env import VecEnv
    emu = make(128, reward=reward, max_episode_steps=max_episode_steps)
    return VecEnv(48, emulator=emu, batch_size=24, log_interval=0, **kw)


@pytest.fixture
def no_streams(monkeypatch):
    for name in ("Stream", "Event", "current_stream", "stream"):
        monkeypatch.setattr(torch.cuda, name, _NoStream)
    monkeypatch.setattr(torch.Tensor, "record_stream", lambda self, s: None)


@pytest.fixture
def ilv(request, monkeypatch):
    if request.param is None:
        monkeypatch.delenv("PK_ILV", raising=False)
    else:
        monkeypatch.setenv("PK_ILV", request.param)
    return request.param


@pytest.mark.parametrize("ilv", ILVS, indirect=True)
def test_model_random_ram(ilv):
    pc.check_model(make, dev)


def test_rounding_inputs_tell_fused_from_unfused():
    pc.check_rounding_is_decidable()


def test_rounding():
    pc.check_rounding(make, dev)


@pytest.mark.parametrize("ilv", ["1", "64"], indirect=True)
def test_state(ilv):
    pc.check_state(make, dev)


@pytest.mark.parametrize("ilv", ILVS, indirect=True)
def test_ranges(ilv):
    pc.check_ranges(make, dev)


def test_guards():
    pc.check_guards(make, dev)


def test_with_emulator():
    pc.check_with_emulator(make, dev)


@pytest.mark.parametrize("reward", [False, True])
def test_vecenv_step(no_streams, reward):
    pc.check_vecenv(make_env, dev, reward, pipeline=False)


@pytest.mark.parametrize("reward", [False, True])
def test_vecenv_recv_send(no_streams, reward):
    pc.check_vecenv(make_env, dev, reward, pipeline=True)


def test_vecenv_done_with_reward(no_streams):
    pc.check_vecenv_done_with_reward(make_env, dev)


def test_vecenv_bank(no_streams):
    pc.check_vecenv_bank(make_env, dev)


def test_vecenv_load_state(no_streams):
    pc.check_vecenv_load_state(make_env, dev)


def test_vecenv_off_and_bad_keywords(no_streams):
    from pokegym_amd.env import VecEnv
    pc.check_vecenv_off(make_env, dev)
    for bad in pc.BAD_KEYWORDS:
        emu = make(64)
        with pytest.raises(ValueError):
            VecEnv(64, emulator=emu, log_interval=0, reward=False, **bad)
        emu.close()


def test_abi():
    """ABI 12 still, and the built gfx950 library and the host-simulation build export the names."""
    import sim
    from pokegym_amd import _native, build, spaces
    names = ("pk_probe_create", "pk_probe_count", "pk_probe_eval")
    assert _native.ABI_VERSION == 12
    for lib in (ctypes.CDLL(build.build()), sim.lib()):
        assert lib.pk_abi_version() == 12
        assert all(hasattr(lib, name) for name in names)
    assert set(names) <= set(_native.EXPORTS)
    assert ctypes.sizeof(_native.PkProbe) == 24
    assert (_native.PK_PV_LE, _native.PK_PV_BE, _native.PK_PV_BCD, _native.PK_PV_BITS) == (0, 1, 2, 3)
    assert (_native.PK_PR_SUM, _native.PK_PR_MAX, _native.PK_PROBE_REBASE_ONLY, _native.PK_PROBE_SET) == (0, 1, 1, 2)
    assert (_native.PK_PO_NONE, _native.PK_PO_DELTA, _native.PK_PO_NEWMAX, _native.PK_PO_CHANGE) == (0, 1, 2, 3)
    assert (_native.PK_PC_NONE, _native.PK_PC_EQ, _native.PK_PC_NE, _native.PK_PC_GE, _native.PK_PC_LE) == (0, 1, 2, 3, 4)
    sp = spaces.probe_space(4)
    assert sp.shape == (4,) and sp.dtype == np.int32
    with pytest.raises(ValueError):
        spaces.probe_space(0)
