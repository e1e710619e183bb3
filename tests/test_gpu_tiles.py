"""Tile view (pk_tiles_*) on the MI355X, through BatchedEmulator and VecEnv: the scenarios of
tiles_common.py, which test_hostsim_tiles.py runs on the CPU.  The tests load states, step a known-good
ROM and read the view and the keys back."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

# PK_ILV: the handle's own interleave, and the image's lane interleave forced to every width a
# 16-env workgroup meets differently: 1 (no run), 16, 32 and 64
ILVS = [None, "1", "16", "32", "64"]
MODES = [("id", 12), ("hash", 8), ("hash", 15)]


def make(n, **kw):
    from pokegym_amd.emulator import BatchedEmulator
    from pokegym_amd.testrom.game import game_rom
    # 4 frames per step: nothing here depends on the step's length
    return BatchedEmulator(game_rom(), n, frame_skip=4, release_frame=2, **kw)


def make_game(n, state):
    from pokegym_amd.emulator import BatchedEmulator
    from pokegym_amd.testrom.game import game_rom
    return BatchedEmulator(game_rom(), n, state=state)


def dev(values, dtype=np.int32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(values, dtype)).cuda()


def make_env(n, reward=True, render=True, **kw):
    from pokegym_amd.env import VecEnv
    emu = make(2 * 64, reward=reward, render=render, max_episode_steps=1000)
    return VecEnv(n, emulator=emu, batch_size=n // 2, log_interval=0, **kw)


@pytest.fixture
def ilv(request, monkeypatch):
    if request.param is None:
        monkeypatch.delenv("PK_ILV", raising=False)
    else:
        monkeypatch.setenv("PK_ILV", request.param)
    return request.param


@pytest.mark.parametrize("mode,bits", MODES)
@pytest.mark.parametrize("ilv", ILVS, indirect=True)
def test_kernel_equals_model(ilv, mode, bits):
    import tiles_common as tc
    tc.check_kernel_equals_model(make, dev, mode, bits)


@pytest.mark.parametrize("ilv", [None, "1"], indirect=True)
def test_ranges_and_masks(ilv):
    import tiles_common as tc
    tc.check_ranges_and_masks(make, dev)


def test_headless_equals_reward_handle():
    import tiles_common as tc
    tc.check_headless_equals_reward_handle(make, dev)


def test_follows_the_game_and_the_oracle():
    import tiles_common as tc
    from oracle import oracle

    def oracle_states(rom, state, acts):
        ref, _ = oracle.batch_run(rom, state, acts, want_screens=False)
        return np.stack([np.asarray(r, np.uint8) for r in ref])

    tc.check_follows_the_game(make_game, dev, oracle_states)


@pytest.mark.parametrize("pipeline", [False, True], ids=["step", "recv_send"])
def test_vecenv(pipeline):
    import tiles_common as tc
    tc.check_vecenv(make_env, dev, pipeline)


def test_vecenv_archive_key():
    import tiles_common as tc
    tc.check_archive_key(make_env, dev)


def test_lifecycle():
    import tiles_common as tc
    tc.check_lifecycle(make, dev)


def test_vecenv_off_and_bad_keywords():
    import tiles_common as tc
    from pokegym_amd.env import VecEnv
    tc.check_vecenv_off(make_env, dev)
    for bad in tc.BAD_KEYWORDS:
        emu = make(64, reward=False)
        with pytest.raises(ValueError):
            VecEnv(64, emulator=emu, log_interval=0, reward=False, **bad)
        emu.close()


def test_abi():
    from pokegym_amd import _native
    lib = _native.load()
    assert lib.pk_abi_version() == _native.ABI_VERSION == 12
    for name in ("pk_tiles_create", "pk_tiles_planes", "pk_tiles_ptr", "pk_tiles_eval"):
        assert hasattr(lib, name)
