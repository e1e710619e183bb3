"""Frame stack (pk_fstack_*) on the MI355X, through BatchedEmulator and VecEnv: the scenarios of
stack_common.py, which test_hostsim_stack.py runs on the CPU.  The tests write screens, read stacks
and step a known-good ROM."""
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
    return torch.from_numpy(np.ascontiguousarray(values, dtype)).cuda()


def make_env(reward=True, max_episode_steps=5, **kw):
    from pokegym_amd.env import VecEnv
    emu = make(128, reward=reward, max_episode_steps=max_episode_steps)
    return VecEnv(48, emulator=emu, batch_size=24, log_interval=0, **kw)


def test_model_random_bytes():
    import stack_common as sc
    sc.check_model(make, dev)


def test_rounding_and_edges():
    import stack_common as sc
    sc.check_edges(make, dev)


def test_reference_frames():
    import stack_common as sc
    sc.check_reference_frames(make, dev)


def test_fill_push_fill_only():
    import stack_common as sc
    sc.check_fill_push(make, dev)


def test_ranges_on_two_streams():
    """Range [0, 64) on one stream and [64, 192) on another, ordered by an event, equal one call."""
    import torch
    import stack_common as sc

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

    sc.check_ranges(make, dev, streams)


def test_screen_source():
    import stack_common as sc
    sc.check_screen_source(make, dev)


def test_guards():
    import stack_common as sc
    sc.check_guards(make, dev)


def test_with_emulator():
    import stack_common as sc
    sc.check_with_emulator(make, dev)


@pytest.mark.parametrize("layout", ["chw", "hwc"])
def test_vecenv_step(layout):
    import stack_common as sc
    sc.check_vecenv_step(make_env, dev, layout)


def test_vecenv_recv_send():
    import stack_common as sc
    sc.check_vecenv_pipeline(make_env, dev)


def test_vecenv_bank():
    import stack_common as sc
    sc.check_vecenv_bank(make_env, dev)


def test_vecenv_off_and_bad_keywords():
    import stack_common as sc
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
    from pokegym_amd import _native
    lib = _native.load()
    assert lib.pk_abi_version() == _native.ABI_VERSION == 12
    for name in ("pk_fstack_create", "pk_fstack_depth", "pk_fstack_scale", "pk_fstack_ptr", "pk_fstack_push"):
        assert hasattr(lib, name)
