"""Time pk_archive_pack / pk_archive_merge on the GPU (profiles/exchange/measure.jsonl).

Two handles of the benchmark ROM in one process, 4,096 envs and a 4,096-cell archive each at the
default episode length.  HIP events around each call, the median of --reps after --warmup.  A full
pack of 4,096 cells and a merge in which every record wins are set against the yardstick taken in
the same process: pk_bank_checkpoint / pk_bank_resume of 4,096 envs plus a plain hipMemcpyAsync
device-to-device of the payload bytes (bound 1.5x).  A delta pack without a dirty cell and a merge of
records without payloads are reported without a bound.  GB/s counts every byte once read and once
written.  There is no CPU fallback: without a GPU this fails.

    python tools/measure_exchange.py --out profiles/exchange/measure.jsonl
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
    ap.add_argument("--cells", type=int, default=4096)
    ap.add_argument("--max-episode-steps", type=int, default=20480)
    ap.add_argument("--trajectories", action="store_true", help="payloads with a trajectory part")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.cells
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w") if a.out else None

    def emit(**rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def handle():
        emu = BatchedEmulator(game_rom(), n, reward=True, max_episode_steps=a.max_episode_steps)
        emu.bank_create(n)
        emu.bank_enable_episodes()
        if a.trajectories:
            emu.traj_enable()
        emu.archive_create(0, n, 1)
        emu.archive_exchange_enable()
        emu.reset()
        return emu

    src, dst = handle(), handle()
    acts = torch.from_numpy(np.random.default_rng(0).integers(0, 8, (3, n), dtype=np.uint8)).cuda()
    for t in range(3):
        src.step(acts[t])
        dst.step(acts[t])
    own = torch.arange(n, dtype=torch.int32, device=src.device)
    keys = torch.arange(n, dtype=torch.int64, device=src.device)          # every env its own cell
    src.archive_update(keys, torch.ones(n, dtype=torch.float64, device=src.device))
    pb = src.archive_payload_bytes
    emit(what="abi", version=_native.ABI_VERSION, cells=n, reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_name(0),
         payload_bytes=pb, format=src.archive_format, trajectories=bool(a.trajectories))

    def timed(fn, pre=None):
        ms = []
        for k in range(a.warmup + a.reps):
            if pre:
                pre()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if k >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return ms

    def report(what, ms, nbytes=0, **kw):
        med = statistics.median(ms)
        emit(what=what, cells=n, ms_median=med, ms_min=min(ms), ms_max=max(ms), bytes_one_way=nbytes,
             gbytes_per_s=2 * nbytes / med / 1e6, **kw)
        return med

    L, stream = src._L, src._stream
    rec = torch.zeros((n, 48), dtype=torch.uint8, device=src.device)
    pay = torch.zeros((n, pb), dtype=torch.uint8, device=src.device)
    cnt = torch.zeros(1, dtype=torch.int32, device=src.device)
    cell_out = torch.zeros(n, dtype=torch.int32, device=src.device)

    def pack(flags, max_payloads):
        def go():
            rc = L.pk_archive_pack(src._h, flags, 0, n, max_payloads, rec.data_ptr(), pay.data_ptr(), cnt.data_ptr(), stream())
            assert rc == 0, rc
        return go

    t_pack = report("archive_pack_full", timed(pack(0, n)), n * pb)
    assert int(cnt) == n
    full = rec.clone()
    score = full.view(torch.float64)[:, 1]                 # pk_xrec.score

    def merge(records, n_payloads):
        def go():
            rc = L.pk_archive_merge(dst._h, records.data_ptr(), n, pay.data_ptr() if n_payloads else None, n_payloads,
                                    cell_out.data_ptr(), stream())
            assert rc == 0, rc
        return go

    # a strictly better score before every call: every record wins and every payload moves
    t_merge = report("archive_merge_all_winners", timed(merge(full, n), pre=lambda: score.add_(1.0)), n * pb)
    assert int((cell_out >= 0).sum()) == n and dst.bank_rejects() == 0
    pack(_native.PK_XCHG_DELTA, n)()                       # ships every dirty cell; none is dirty after it
    report("archive_pack_delta_nothing_dirty", timed(pack(_native.PK_XCHG_DELTA, n)))
    assert int(cnt) == 0
    bare = full.clone()
    bare.view(torch.int32)[:, 7] = -1                      # pk_xrec.payload: records only
    report("archive_merge_records_only", timed(merge(bare, 0)))
    assert int((cell_out >= 0).sum()) == 0

    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    other = torch.empty_like(pay)

    def memcpy():
        rc = hip.hipMemcpyAsync(other.data_ptr(), pay.data_ptr(), n * pb, 3, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc

    t_cp = report("memcpy_d2d_payload_bytes", timed(memcpy), n * pb)
    t_ck = report("bank_checkpoint", timed(lambda: src.bank_checkpoint(own)), n * pb)
    t_rs = report("bank_resume", timed(lambda: src.bank_resume(own)), n * pb)
    for what, t, base in (("pack", t_pack, t_ck), ("merge", t_merge, t_rs)):
        ratio = t / (t_cp + base)
        emit(what="ratio_" + what, over="memcpy_d2d_payload_bytes + bank_" + ("checkpoint" if what == "pack" else "resume"),
             yardstick_ms=t_cp + base, ratio=ratio, bound=1.5, ok=ratio <= 1.5)
    src.close()
    dst.close()
    emit(what="done")


if __name__ == "__main__":
    main()
