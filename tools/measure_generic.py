"""Time pk_bank_checkpoint / pk_bank_resume with generic episode parts on the GPU (DESIGN.md 7l,
profiles/generic/measure.jsonl).

4,096 and 65,536 envs of the benchmark ROM without the reward stack, pkbench's probes and a frame
stack (2, 4, hwc), parts = probes + stack, each env to / from its own slot.  HIP events around each
call, the median of --reps after --warmup, one process.  Before the timing a resumed env is compared
with what its source held at the checkpoint: stack row, screen, machine state and the next step's
probe reward.  Yardsticks from the same run: pk_bank_save / pk_bank_load of the same envs, and a plain
hipMemcpyAsync device-to-device of the generic parts' byte count; a call may take 1.5 x their sum.
GB/s counts every byte once read and once written.  There is no CPU fallback: without a GPU this fails.

    python tools/measure_generic.py --out profiles/generic/measure.jsonl
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
STACK = (2, 4, "hwc")


def main():
    import numpy as np
    import torch
    from pokegym_amd import _native, probes
    from pokegym_amd.emulator import BatchedEmulator
    from pokegym_amd.testrom.game import game_rom

    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w") if a.out else None

    def emit(**rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    prog = probes.pkbench_program()

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

    for n in a.envs:
        emu = BatchedEmulator(game_rom(), n, reward=False)
        emu.probes_create(prog)
        emu.stack_create(*STACK, "mean")
        emu.bank_create(n)
        emu.bank_enable_generic_episodes(probes=True, stack=True)
        gep = emu.generic_episode_bytes
        emit(what="abi", version=_native.ABI_VERSION, envs=n, slots=n, reps=a.reps, warmup=a.warmup,
             device=torch.cuda.get_device_name(0), parts=emu.generic_parts, stack=list(STACK), probes=len(prog),
             generic_bytes_per_slot=gep, machine_bytes_per_slot=MACHINE_BYTES)
        acts = torch.from_numpy(np.random.default_rng(0).integers(0, 8, (5, n), dtype=np.uint8)).cuda()
        own = torch.arange(n, dtype=torch.int32, device=emu.device)

        def step(t, rew):
            emu.step(acts[t])
            emu.stack_push()
            emu.probes_eval(set=True, rewards=rew)

        # the twin before the timing: env e resumes from the slot of env n - 1 - e and then holds and
        # pays what that env held at the checkpoint and paid in the step after it
        emu.reset()
        emu.stack_push(fill_only=True)
        emu.probes_eval(rebase_only=True)
        r0, r1 = (torch.zeros(n, dtype=torch.float64, device=emu.device) for _ in range(2))
        for t in range(3):
            step(t, r0)
        emu.bank_checkpoint(own)
        held = emu.stack.clone(), emu.screen.clone()
        snap = emu.snapshot_range(0, min(n, 256)).copy()
        step(3, r0)
        emu.bank_resume(own.flip(0))
        ok = bool(torch.equal(emu.stack, held[0].flip(0)) and torch.equal(emu.screen, held[1].flip(0)))
        ok = ok and bytes(emu.snapshot(n - 1)) == bytes(snap[0]) and emu.bank_rejects() == 0
        acts[3] = acts[3].flip(0)
        step(3, r1)
        ok = ok and bool(torch.equal(r1, r0.flip(0)))
        emit(what="twin_check", envs=n, ok=ok)
        assert ok, "a resumed env differs from its source"

        def report(what, ms, nbytes):
            med = statistics.median(ms)
            emit(what=what, envs=n, ms_median=med, ms_min=min(ms), ms_max=max(ms), bytes_one_way=nbytes,
                 gbytes_per_s=2 * nbytes / med / 1e6)
            return med

        src = torch.empty(n * gep, dtype=torch.uint8, device=emu.device).random_(0, 256)
        dst = torch.empty_like(src)

        def memcpy():
            rc = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), n * gep, 3, torch.cuda.current_stream().cuda_stream)
            assert rc == 0, rc

        t_save = report("bank_save", timed(lambda: emu.bank_save(own)), n * MACHINE_BYTES)
        t_load = report("bank_load", timed(lambda: emu.bank_load(own)), n * MACHINE_BYTES)
        t_cp = report("memcpy_d2d_generic_bytes", timed(memcpy), n * gep)
        t_ck = report("bank_checkpoint", timed(lambda: emu.bank_checkpoint(own)), n * (gep + MACHINE_BYTES))
        t_rs = report("bank_resume", timed(lambda: emu.bank_resume(own)), n * (gep + MACHINE_BYTES))
        emit(what="rejects", envs=n, count=emu.bank_rejects())
        for what, t, base in (("checkpoint", t_ck, t_save), ("resume", t_rs, t_load)):
            ratio = t / (t_cp + base)
            emit(what="ratio_" + what, envs=n, over="memcpy_d2d_generic_bytes + bank_" + ("save" if what == "checkpoint" else "load"),
                 yardstick_ms=t_cp + base, ratio=ratio, bound=1.5, ok=ratio <= 1.5)
        emit(what="generic_mover_alone", envs=n, checkpoint_ms=t_ck - t_save, resume_ms=t_rs - t_load, memcpy_ms=t_cp,
             note="difference of medians")
        del src, dst, held
        emu.close()
        torch.cuda.empty_cache()
    emit(what="done")


if __name__ == "__main__":
    main()
