"""Frame cells (pk_frame_keys / pk_frame_cells, ABI v12) on the CPU: the unmodified kernel and C ABI
in the host-simulation build (tests/hostsim).  The scenarios and the model live in cells_common.py;
the gfx950 build runs them in test_gpu_cells.py (-m gpu)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hostsim"))
sys.path.insert(0, HERE)

import cells_common as cc  # noqa: E402
import episodes_common as ec  # noqa: E402
from emulator import HostsimEmulator  # noqa: E402
from pokegym_amd.testrom.game import game_rom  # noqa: E402
from test_hostsim_archive import _NoStream  # noqa: E402


def make(n, **kw):
    # 4 frames per step: nothing here depends on the step's length
    return HostsimEmulator(game_rom(), n, frame_skip=4, release_frame=2, **kw)


def dev(values, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(values, dtype))


def test_random_bytes():
    cc.check_random(make, dev)


def test_reference_frames():
    cc.check_reference_frames(make, dev)


def test_one_pixel():
    cc.check_one_pixel(make, dev)


def test_ranges():
    cc.check_ranges(make, dev)


def test_salt():
    cc.check_salt(make, dev)


def test_screen_source():
    cc.check_screen_source(make, dev)


def test_guards():
    cc.check_guards(make, dev)


def test_with_emulator():
    cc.check_with_emulator(make, dev)


def test_vecenv(monkeypatch):
    from pokegym_amd.env import VecEnv
    for name in ("Stream", "Event", "current_stream", "stream"):
        monkeypatch.setattr(torch.cuda, name, _NoStream)

    def make_env(**kw):
        emu = make(128, reward=True, max_episode_steps=ec.MAX_STEPS)
        return VecEnv(48, emulator=emu, batch_size=24, log_interval=0, bank_episodes=True, archive_cells=8, **kw)

    cc.check_vecenv(make_env, dev)
    for bad in ({"archive_key": "screen"}, {"archive_frame": (12, 16, 8)}, {"archive_frame": (16, 32, 8)},
                {"archive_frame": (16, 16, 1)}, {"archive_frame": (16, 16, 257)}, {"archive_frame": (16, 16)},
                {"archive_frame": None}):
        emu = make(64, reward=True, max_episode_steps=ec.MAX_STEPS)
        with pytest.raises(ValueError):
            VecEnv(64, emulator=emu, log_interval=0, **bad)
        emu.close()
    emu = make(64, render=False)
    with pytest.raises(ValueError):
        VecEnv(64, emulator=emu, log_interval=0, reward=False, archive_key="frame")
    emu.close()


def test_abi():
    """ABI 12, and the built gfx950 library and the host-simulation build export both names."""
    import sim
    from pokegym_amd import _native, build
    assert _native.ABI_VERSION == 12
    for lib in (ctypes.CDLL(build.build()), sim.lib()):
        assert lib.pk_abi_version() == 12
        assert hasattr(lib, "pk_frame_cells") and hasattr(lib, "pk_frame_keys")
    assert {"pk_frame_cells", "pk_frame_keys"} <= set(_native.EXPORTS)
