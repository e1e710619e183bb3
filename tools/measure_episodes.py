"""Time pk_bank_checkpoint / pk_bank_resume on the GPU (profiles/episodes/measure.jsonl).

4,096 envs of the benchmark ROM at the default episode length, each to / from its own slot.  HIP
events around each call, the median of --reps after --warmup.  Yardsticks taken in the same
process: a plain hipMemcpyAsync device-to-device of the episode parts' byte count, and
pk_bank_save / pk_bank_load for the machine part.  GB/s counts every byte once read and once
written.  There is no CPU fallback: without a GPU this fails.

    python tools/measure_episodes.py --out profiles/episodes/measure.jsonl
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

MACHINE_BYTES = 0xC200 + 20 * 4 + 3 * 144 * 4 + 144 * 160   # pk_layout.h: one slot's machine part
EP_RECORD_BYTES = 68 * 4                                      # pk_reward.h PK_EP_WORDS


def main():
    import numpy as np
    import torch
    from pokegym_amd import _native
    from pokegym_amd.emulator import BatchedEmulator
    from pokegym_amd.env import _seen_cap_log2
    from pokegym_amd.testrom.game import game_rom

    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--max-episode-steps", type=int, default=20480)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
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

    emu = BatchedEmulator(game_rom(), n, reward=True, max_episode_steps=a.max_episode_steps)
    emu.bank_create(n)
    emu.bank_enable_episodes()
    emu.reset()
    acts = torch.from_numpy(np.random.default_rng(0).integers(0, 8, (3, n), dtype=np.uint8)).cuda()
    for t in range(3):
        emu.step(acts[t])
    own = torch.arange(n, dtype=torch.int32, device=emu.device)
    ep_bytes = (4 << _seen_cap_log2(a.max_episode_steps)) + 8448 + EP_RECORD_BYTES
    emit(what="abi", version=_native.ABI_VERSION, envs=n, slots=n, reps=a.reps, warmup=a.warmup,
         device=torch.cuda.get_device_name(0), episode_bytes_per_slot=ep_bytes, machine_bytes_per_slot=MACHINE_BYTES)

    def timed(fn):
        ms = []
        for k in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if k >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return ms

    def report(what, ms, nbytes):
        med = statistics.median(ms)
        emit(what=what, envs=n, ms_median=med, ms_min=min(ms), ms_max=max(ms), bytes_one_way=nbytes,
             gbytes_per_s=2 * nbytes / med / 1e6)
        return med

    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    src = torch.empty(n * (ep_bytes + MACHINE_BYTES), dtype=torch.uint8, device=emu.device).random_(0, 256)
    dst = torch.empty_like(src)

    def memcpy(nbytes):
        def go():
            rc = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, torch.cuda.current_stream().cuda_stream)
            assert rc == 0, rc
        return go

    t_save = report("bank_save", timed(lambda: emu.bank_save(own)), n * MACHINE_BYTES)
    t_load = report("bank_load", timed(lambda: emu.bank_load(own)), n * MACHINE_BYTES)
    t_cp_ep = report("memcpy_d2d_episode_bytes", timed(memcpy(n * ep_bytes)), n * ep_bytes)
    report("memcpy_d2d_total_bytes", timed(memcpy(n * (ep_bytes + MACHINE_BYTES))), n * (ep_bytes + MACHINE_BYTES))
    t_ck = report("bank_checkpoint", timed(lambda: emu.bank_checkpoint(own)), n * (ep_bytes + MACHINE_BYTES))
    t_rs = report("bank_resume", timed(lambda: emu.bank_resume(own)), n * (ep_bytes + MACHINE_BYTES))
    emit(what="rejects", count=emu.bank_rejects())
    for what, t, base in (("checkpoint", t_ck, t_save), ("resume", t_rs, t_load)):
        ratio = t / (t_cp_ep + base)
        emit(what="ratio_" + what, over="memcpy_d2d_episode_bytes + bank_" + ("save" if what == "checkpoint" else "load"),
             yardstick_ms=t_cp_ep + base, ratio=ratio, bound=1.5, ok=ratio <= 1.5)
    emit(what="episode_mover_alone", checkpoint_ms=t_ck - t_save, resume_ms=t_rs - t_load, memcpy_ms=t_cp_ep,
         note="difference of medians; the resume's includes the observation rebuild")
    emu.close()
    emit(what="done")


if __name__ == "__main__":
    main()
