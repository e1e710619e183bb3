"""Time the action trajectories on the GPU (profiles/trajectories/measure.jsonl).

Part 1, checkpoint and resume with trajectories on: 4,096 envs at the default episode length, each
to / from its own slot, at trajectory lengths 2,048 and 20,480.  The step counters are driven
there with frame_skip = 0 handles (a step then emulates nothing but still counts, records and runs
the reward stack).  Yardstick, in the same process: pk_bank_checkpoint / pk_bank_resume of a handle
that never enabled trajectories — it makes the launches the ABI v9 build makes — plus a
device-to-device hipMemcpyAsync of the trajectory bytes moved.  Bound 1.5x.

Part 2, recording on the step path: two 4,096-env handles at the default 24 frames per step, one
recording and one not, fed the same actions; blocks of 20 timed steps after 3, alternating.
Bound: recording at most 1 % slower.

HIP events, medians of --reps after --warmup.  There is no CPU fallback: without a GPU this fails.

    python tools/measure_traj.py --out profiles/trajectories/measure.jsonl
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def main():
    import numpy as np
    import torch
    from pokegym_amd import _native
    from pokegym_amd.emulator import BatchedEmulator
    from pokegym_amd.testrom.game import game_rom

    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--max-episode-steps", type=int, default=20480)
    ap.add_argument("--lengths", type=int, nargs="+", default=[2048, 20480])
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-blocks", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.envs
    out = open(a.out, "w") if a.out else None

    def emit(**rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def timed(fn, reps=a.reps, warmup=a.warmup):
        ms = []
        for k in range(warmup + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if k >= warmup:
                ms.append(e0.elapsed_time(e1))
        return ms

    def report(what, ms, **kw):
        med = statistics.median(ms)
        emit(what=what, envs=n, ms_median=med, ms_min=min(ms), ms_max=max(ms), **kw)
        return med

    rom = game_rom()
    rng = np.random.default_rng(0)
    emit(what="abi", version=_native.ABI_VERSION, envs=n, reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_name(0))

    # ---- part 1: the movers ---------------------------------------------------------------------
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    handles = {}
    for name in ("off", "on"):
        emu = BatchedEmulator(rom, n, reward=True, render=False, frame_skip=0, max_episode_steps=a.max_episode_steps)
        if name == "on":
            emu.traj_enable()
        emu.bank_create(n)
        emu.bank_enable_episodes()
        emu.reset()
        handles[name] = emu
    cap = handles["on"].traj_capacity
    src = torch.empty(n * cap, dtype=torch.uint8, device=handles["on"].device).random_(0, 256)
    dst = torch.empty_like(src)
    own = torch.arange(n, dtype=torch.int32, device=src.device)
    emit(what="capacity", bytes_per_env=cap)
    done = 0
    for length in sorted(a.lengths):
        acts = torch.from_numpy(rng.integers(0, 8, (length - done, n), dtype=np.uint8)).cuda()
        for emu in handles.values():
            for t in range(length - done):
                emu.step(acts[t])
        done = length
        torch.cuda.synchronize()
        got = handles["on"].trajectories()
        assert int(got["length"].min()) == int(got["length"].max()) == min(length, cap) and not bool(got["flags"].any())
        nbytes = n * ((min(length, cap) + 15) // 16 * 16)

        def memcpy():
            rc = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, torch.cuda.current_stream().cuda_stream)
            assert rc == 0, rc

        t_cp = report("memcpy_d2d_trajectory_bytes", timed(memcpy), length=length, bytes_one_way=nbytes)
        t = {}
        for name, emu in handles.items():
            t["checkpoint", name] = report("bank_checkpoint", timed(lambda: emu.bank_checkpoint(own)), length=length, trajectories=name)
            t["resume", name] = report("bank_resume", timed(lambda: emu.bank_resume(own)), length=length, trajectories=name)
            emit(what="rejects", trajectories=name, count=emu.bank_rejects())
        for what in ("checkpoint", "resume"):
            yard = t[what, "off"] + t_cp
            emit(what="ratio_" + what, length=length, over="bank_" + what + " without trajectories + memcpy_d2d_trajectory_bytes",
                 yardstick_ms=yard, ratio=t[what, "on"] / yard, bound=1.5, ok=t[what, "on"] / yard <= 1.5,
                 mover_alone_ms=t[what, "on"] - t[what, "off"], memcpy_ms=t_cp)
    slot = handles["on"].bank_trajectories(0, n)
    env = handles["on"].trajectories()
    emit(what="slots_equal_envs", ok=all(bool(torch.equal(slot[k], env[k])) for k in ("origin", "length", "flags", "actions")))
    for emu in handles.values():
        emu.close()
    del src, dst
    torch.cuda.empty_cache()

    # ---- part 2: recording beside the step ------------------------------------------------------
    steps, warm = 20, 3
    acts = torch.from_numpy(rng.integers(0, 8, (warm + steps, n), dtype=np.uint8)).cuda()
    pair = {}
    for name in ("off", "on"):
        emu = BatchedEmulator(rom, n, reward=True, max_episode_steps=a.max_episode_steps)
        if name == "on":
            emu.traj_enable()
        emu.reset()
        pair[name] = emu

    def block(emu):
        for t in range(warm):
            emu.step(acts[t])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for t in range(warm, warm + steps):
            emu.step(acts[t])
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / steps

    ms = {"off": [], "on": []}
    for k in range(a.step_blocks + 1):
        for name in ("off", "on"):
            v = block(pair[name])
            if k:                            # the first round warms both handles up
                ms[name].append(v)
    med = {name: report("step", v, trajectories=name, steps_per_block=steps, blocks=a.step_blocks) for name, v in ms.items()}
    emit(what="ratio_step", on_over_off=med["on"] / med["off"], bound=1.01, ok=med["on"] / med["off"] <= 1.01)
    for emu in pair.values():
        emu.close()
    emit(what="done")


if __name__ == "__main__":
    main()
