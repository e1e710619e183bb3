"""Tile view (pk_tiles_*) on the CPU: the unmodified kernel and C ABI in the host-simulation build
(tests/hostsim).  The scenarios live in tiles_common.py, the model in pokegym_amd/tiles.py; the gfx950
build runs them in test_gpu_tiles.py (-m gpu)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hostsim"))
sys.path.insert(0, HERE)

import tiles_common as tc  # noqa: E402
from emulator import HostsimEmulator  # noqa: E402
from pokegym_amd.testrom.game import game_rom  # noqa: E402
from test_hostsim_archive import _NoStream  # noqa: E402

# PK_ILV: the handle's own interleave, and the image's lane interleave forced to every width a
# 16-env workgroup meets differently: 1 (no run), 16, 32 and 64
ILVS = [None, "1", "16", "32", "64"]


def make(n, **kw):
    # 4 frames per step: nothing here depends on the step's length
    return HostsimEmulator(game_rom(), n, frame_skip=4, release_frame=2, **kw)


def make_game(n, state):
    return HostsimEmulator(game_rom(), n, state=state)


def dev(values, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(values, dtype))


def make_env(n, reward=True, render=True, **kw):
    from pokegym_amd.env import VecEnv
    emu = make(2 * 64, reward=reward, render=render, max_episode_steps=1000)
    return VecEnv(n, emulator=emu, batch_size=n // 2, log_interval=0, **kw)


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


def test_model_equals_pixel_statement():
    tc.check_model_equals_pixels()


def test_states_reach_the_rules():
    tc.check_states_reach_the_rules()


@pytest.mark.parametrize("mode,bits", tc.MODES)
@pytest.mark.parametrize("ilv", ILVS, indirect=True)
def test_kernel_equals_model(ilv, mode, bits):
    tc.check_kernel_equals_model(make, dev, mode, bits)


@pytest.mark.parametrize("ilv", [None, "1"], indirect=True)
def test_ranges_and_masks(ilv):
    tc.check_ranges_and_masks(make, dev)


def test_headless_equals_reward_handle():
    tc.check_headless_equals_reward_handle(make, dev)


def test_follows_the_game():
    tc.check_follows_the_game(make_game, dev)


@pytest.mark.parametrize("pipeline", [False, True], ids=["step", "recv_send"])
def test_vecenv(no_streams, pipeline):
    tc.check_vecenv(make_env, dev, pipeline)


def test_vecenv_archive_key(no_streams):
    tc.check_archive_key(make_env, dev)


def test_lifecycle():
    tc.check_lifecycle(make, dev)


def test_vecenv_off_and_bad_keywords(no_streams):
    from pokegym_amd.env import VecEnv
    tc.check_vecenv_off(make_env, dev)
    for bad in tc.BAD_KEYWORDS:
        emu = make(64, reward=False)
        with pytest.raises(ValueError):
            VecEnv(64, emulator=emu, log_interval=0, reward=False, **bad)
        emu.close()


def test_abi():
    """ABI 12 still, and the built gfx950 library and the host-simulation build export the names."""
    import sim
    from pokegym_amd import _native, build, spaces
    names = ("pk_tiles_create", "pk_tiles_planes", "pk_tiles_ptr", "pk_tiles_eval")
    assert _native.ABI_VERSION == 12
    for lib in (ctypes.CDLL(build.build()), sim.lib()):
        assert lib.pk_abi_version() == 12
        assert all(hasattr(lib, name) for name in names)
    assert set(names) <= set(_native.EXPORTS)
    assert (_native.PK_TILES_ID, _native.PK_TILES_HASH, _native.PK_TILES_OBJ) == (0, 1, 1)
    sp = spaces.tile_space(2)
    assert sp.shape == (2, 18, 20) and sp.dtype == np.int16
    with pytest.raises(ValueError):
        spaces.tile_space(3)
