"""RAM probes (pk_probe_*) on the MI355X, through BatchedEmulator and VecEnv: the scenarios of
probes_common.py, which test_hostsim_probes.py runs on the CPU.  The tests write RAM, read the three
outputs and step a known-good ROM."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

# PK_ILV: the handle's own interleave, and the image's lane interleave forced to 1, 16 and 64
ILVS = [None, "1", "16", "64"]


def make(n, **kw):
    from pokegym_amd.emulator import BatchedEmulator
    from pokegym_amd.testrom.game import game_rom
    # 4 frames per step: nothing here depends on the step's length
    return BatchedEmulator(game_rom(), n, frame_skip=4, release_frame=2, **kw)


def dev(values, dtype=np.int32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(values, dtype)).cuda()


def make_env(reward=True, max_episode_steps=1000, **kw):
    from pokegym_amd.env import VecEnv
    emu = make(128, reward=reward, max_episode_steps=max_episode_steps)
    return VecEnv(48, emulator=emu, batch_size=24, log_interval=0, **kw)


@pytest.fixture
def ilv(request, monkeypatch):
    if request.param is None:
        monkeypatch.delenv("PK_ILV", raising=False)
    else:
        monkeypatch.setenv("PK_ILV", request.param)
    return request.param


@pytest.mark.parametrize("ilv", ILVS, indirect=True)
def test_model_random_ram(ilv):
    import probes_common as pc
    pc.check_model(make, dev)


def test_rounding():
    import probes_common as pc
    pc.check_rounding_is_decidable()
    pc.check_rounding(make, dev)


@pytest.mark.parametrize("ilv", ["1", "64"], indirect=True)
def test_state(ilv):
    import probes_common as pc
    pc.check_state(make, dev)


@pytest.mark.parametrize("ilv", ILVS, indirect=True)
def test_ranges_on_two_streams(ilv):
    """Range [0, 64) on one stream and [64, 192) on another, ordered by an event, equal one call."""
    import torch
    import probes_common as pc

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

    pc.check_ranges(make, dev, streams)


def test_guards():
    import probes_common as pc
    pc.check_guards(make, dev)


def test_with_emulator():
    import probes_common as pc
    pc.check_with_emulator(make, dev)


@pytest.mark.parametrize("reward", [False, True])
def test_vecenv_step(reward):
    import probes_common as pc
    pc.check_vecenv(make_env, dev, reward, pipeline=False)


@pytest.mark.parametrize("reward", [False, True])
def test_vecenv_recv_send(reward):
    import probes_common as pc
    pc.check_vecenv(make_env, dev, reward, pipeline=True)


def test_vecenv_done_with_reward():
    import probes_common as pc
    pc.check_vecenv_done_with_reward(make_env, dev)


def test_vecenv_bank():
    import probes_common as pc
    pc.check_vecenv_bank(make_env, dev)


def test_vecenv_load_state():
    import probes_common as pc
    pc.check_vecenv_load_state(make_env, dev)


def test_vecenv_off_and_bad_keywords():
    import probes_common as pc
    from pokegym_amd.env import VecEnv
    pc.check_vecenv_off(make_env, dev)
    for bad in pc.BAD_KEYWORDS:
        emu = make(64)
        with pytest.raises(ValueError):
            VecEnv(64, emulator=emu, log_interval=0, reward=False, **bad)
        emu.close()


def test_abi():
    from pokegym_amd import _native
    lib = _native.load()
    assert lib.pk_abi_version() == _native.ABI_VERSION == 12
    for name in ("pk_probe_create", "pk_probe_count", "pk_probe_eval"):
        assert hasattr(lib, name)
