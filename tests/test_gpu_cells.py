"""Frame cells (pk_frame_keys / pk_frame_cells, ABI v12) on the MI355X, through BatchedEmulator and
VecEnv: the scenarios of cells_common.py, which test_hostsim_cells.py runs on the CPU.  The tests
write screens, read keys and cell images and step a known-good ROM."""
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


def test_random_bytes():
    import cells_common as cc
    cc.check_random(make, dev)


def test_reference_frames():
    import cells_common as cc
    cc.check_reference_frames(make, dev)


def test_one_pixel():
    import cells_common as cc
    cc.check_one_pixel(make, dev)


def test_ranges_on_two_streams():
    """Range [0, 64) on one stream and [64, 192) on another, ordered by an event, equal one call."""
    import torch
    import cells_common as cc

    def streams(first, second):
        s1, s2, ev = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Event()
        cur = torch.cuda.current_stream()
        s1.wait_stream(cur)
        s2.wait_stream(cur)
        with torch.cuda.stream(s1):
            first()
            ev.record(s1)
        with torch.cuda.stream(s2):
            s2.wait_event(ev)
            second()
        cur.wait_stream(s1)
        cur.wait_stream(s2)

    cc.check_ranges(make, dev, streams)


def test_salt():
    import cells_common as cc
    cc.check_salt(make, dev)


def test_screen_source():
    import cells_common as cc
    cc.check_screen_source(make, dev)


def test_guards():
    import cells_common as cc
    cc.check_guards(make, dev)


def test_with_emulator():
    import cells_common as cc
    cc.check_with_emulator(make, dev)


def test_vecenv():
    import cells_common as cc
    import episodes_common as ec
    from pokegym_amd.env import VecEnv
    from pokegym_amd.testrom.game import game_rom

    def make_env(**kw):
        return VecEnv(48, rom=game_rom(), power_on=True, batch_size=24, max_episode_steps=ec.MAX_STEPS, log_interval=0,
                      bank_episodes=True, archive_cells=8, **kw)

    cc.check_vecenv(make_env, dev)
    for bad in ({"archive_key": "screen"}, {"archive_frame": (12, 16, 8)}, {"archive_frame": (16, 32, 8)},
                {"archive_frame": (16, 16, 1)}, {"archive_frame": (16, 16, 257)}, {"archive_frame": (16, 16)},
                {"archive_frame": None}):
        emu = make(64, reward=True, max_episode_steps=ec.MAX_STEPS)
        with pytest.raises(ValueError):
            VecEnv(64, emulator=emu, log_interval=0, **bad)
        emu.close()


def test_abi():
    from pokegym_amd import _native
    lib = _native.load()
    assert lib.pk_abi_version() == _native.ABI_VERSION == 12
    assert hasattr(lib, "pk_frame_cells") and hasattr(lib, "pk_frame_keys")
