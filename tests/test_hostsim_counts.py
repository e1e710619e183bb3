"""Visit counts (pk_counts_*) on the CPU: the unmodified kernels and C ABI in the host-simulation
build (tests/hostsim).  The scenarios and the model live in counts_common.py; the gfx950 build
runs them in test_gpu_counts.py (-m gpu), where the table's atomics race for real."""
import ctypes
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hostsim"))
sys.path.insert(0, HERE)

import counts_common as cc  # noqa: E402
from emulator import HostsimEmulator  # noqa: E402
from pokegym_amd.testrom.game import game_rom  # noqa: E402
from test_hostsim_archive import _NoStream  # noqa: E402


def make(n, **kw):
    return HostsimEmulator(game_rom(), n, frame_skip=4, release_frame=2, **kw)


def dev(values, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(values, dtype))


def test_model_equality():
    cc.check_model_equality(make, dev)


def test_ranges_mask_nokey():
    cc.check_ranges(make, dev)


def test_full_table():
    cc.check_full_table(make, dev)


def test_peek():
    cc.check_peek(make, dev)


def test_pack_add():
    cc.check_pack_add(make, dev)


def test_guards():
    cc.check_guards(make, dev)


def test_run_to_run():
    cc.check_run_to_run(make, dev)


def _make_env(monkeypatch):
    from pokegym_amd.env import VecEnv
    for name in ("Stream", "Event", "current_stream", "stream"):
        monkeypatch.setattr(torch.cuda, name, _NoStream)
    monkeypatch.setattr(torch.Tensor, "record_stream", lambda self, s: None)

    def make_env(num, batch_size, **kw):
        emu = make(num if batch_size is None else num // batch_size * 64, max_episode_steps=5)
        return VecEnv(num, emulator=emu, batch_size=batch_size, log_interval=0, **kw)

    return make_env


def test_vecenv(monkeypatch):
    cc.check_vecenv(_make_env(monkeypatch), dev)


def test_vecenv_ram_keys(monkeypatch):
    cc.check_vecenv_ram_keys(_make_env(monkeypatch), dev)


def test_abi():
    """Still ABI 12, and the built gfx950 library and the host-simulation build export the seven names."""
    import sim
    from pokegym_amd import _native, build
    assert _native.ABI_VERSION == 12
    for lib in (ctypes.CDLL(build.build()), sim.lib()):
        assert lib.pk_abi_version() == 12
        for name in cc.EXPORTS:
            assert hasattr(lib, name), name
    assert set(cc.EXPORTS) <= set(_native.EXPORTS)
