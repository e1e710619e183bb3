"""Time pk_archive_update / pk_archive_explore on the GPU (profiles/archive/measure.jsonl).

pk_archive_update at 4,096 and 65,536 envs of the benchmark ROM against a 4,096-cell archive:
steady state with no winner and with ~1 % winners; and with every env a new cell (4,096 envs; as
an archive cannot be emptied, that regime runs against a 65,536-cell archive, 4,096 fresh keys per
call, so it has fewer repetitions).  pk_archive_explore for 4,096 masked envs.  HIP events around
each call, the median of --reps after --warmup.  Two yardsticks in the same process: (a)
pk_bank_checkpoint / pk_bank_resume of the same winner / destination set alone — the archive call
minus this is the bookkeeping; (b) the same bookkeeping in torch: torch.unique + scatter-reduce
over keys and scores, host sync included.  There is no CPU fallback: without a GPU this fails.

    python tools/measure_archive.py --out profiles/archive/measure.jsonl
"""
from __future__ import annotations

import argparse
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
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--cells", type=int, default=4096)
    ap.add_argument("--max-episode-steps", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "a") if a.out else None

    def emit(**rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def timed(fn, reps=a.reps, before=None):
        ms = []
        for k in range(a.warmup + reps):
            if before:
                before(k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if k >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return statistics.median(ms)

    def torch_update(keys, scores):
        uk, inv = torch.unique(keys, return_inverse=True)
        best = torch.full((uk.numel(),), -float("inf"), dtype=torch.float64, device=keys.device)
        best.scatter_reduce_(0, inv, scores, "amax")
        torch.bincount(inv, minlength=uk.numel())
        torch.cuda.synchronize()

    emit(what="abi", version=_native.ABI_VERSION, cells=a.cells, reps=a.reps, warmup=a.warmup,
         device=torch.cuda.get_device_name(0), max_episode_steps=a.max_episode_steps)
    for n in a.envs:
        new = n == min(a.envs)                 # the all-new regime runs at the smaller size only
        cells = [a.cells] + ([65536] if new else [])
        emu = BatchedEmulator(game_rom(), n, reward=True, max_episode_steps=a.max_episode_steps)
        dev = emu.device
        acts = torch.from_numpy(np.random.default_rng(0).integers(0, 8, (3, n), dtype=np.uint8)).to(dev)
        emu.bank_create(a.cells)
        emu.bank_enable_episodes()
        emu.archive_create(0, a.cells, 1)
        emu.reset()
        for t in range(3):
            emu.step(acts[t])
        env = torch.arange(n, device=dev)
        keys = (env * 2654435761 % a.cells).to(torch.int64)      # every cell, 1 or 16 envs each
        scores = torch.zeros(n, dtype=torch.float64, device=dev)
        slot_out = torch.full((n,), -1, dtype=torch.int32, device=dev)
        emu.archive_update(keys, scores, out=slot_out)            # fills the archive
        low = scores - 1.0

        ms = timed(lambda: emu.archive_update(keys, low, out=slot_out))
        none = torch.full((n,), -1, dtype=torch.int32, device=dev)
        ck = timed(lambda: emu.bank_checkpoint(none))
        tt = timed(lambda: torch_update(keys, low))
        emit(what="update_no_winner", envs=n, cells=a.cells, ms_median=ms, checkpoint_alone_ms=ck, bookkeeping_ms=ms - ck,
             torch_unique_scatter_sync_ms=tt, not_slower_than_torch=ms - ck <= tt)

        # ~1 % winners: another 1 % of the envs, in distinct cells, beats every record each call
        w = max(1, n // 100)
        rise = scores.clone()

        def raise_some(k):
            rise.copy_(low)
            rise[(torch.arange(w, device=dev) * (n // w) + k) % n] = float(k + 1)
        ms = timed(lambda: emu.archive_update(keys, rise, out=slot_out), before=raise_some)
        winners = slot_out.clone()
        ck = timed(lambda: emu.bank_checkpoint(winners))
        tt = timed(lambda: torch_update(keys, rise))
        emit(what="update_1pct_winners", envs=n, cells=a.cells, winners=int((winners >= 0).sum()), ms_median=ms,
             checkpoint_alone_ms=ck, bookkeeping_ms=ms - ck, torch_unique_scatter_sync_ms=tt,
             not_slower_than_torch=ms - ck <= tt)

        if n >= 4096:
            mask = torch.zeros(n, dtype=torch.uint8, device=dev)
            mask[:4096] = 1
            ms = timed(lambda: emu.archive_explore(mask, out=slot_out))
            drawn = slot_out.clone()
            rs = timed(lambda: emu.bank_resume(drawn))
            emit(what="explore", envs=n, masked=4096, cells=a.cells, ms_median=ms, resume_alone_ms=rs, bookkeeping_ms=ms - rs)
        emit(what="rejects", envs=n, count=emu.bank_rejects(), overflow=emu.archive_read()["overflow"])
        emu.close()

        if new:   # every env a new cell: 65,536 cells take 16 calls of 4,096 fresh keys
            reps = 65536 // n - a.warmup - 1
            emu = BatchedEmulator(game_rom(), n, reward=True, max_episode_steps=a.max_episode_steps)
            emu.bank_create(65536)
            emu.bank_enable_episodes()
            emu.archive_create(0, 65536, 1)
            emu.reset()
            fresh = torch.zeros(n, dtype=torch.int64, device=dev)
            slots = torch.zeros(n, dtype=torch.int32, device=dev)

            def next_keys(k):
                fresh.copy_(env + k * n)
                slots.copy_((env + k * n).to(torch.int32))
            ms = timed(lambda: emu.archive_update(fresh, scores, out=slot_out), reps=reps, before=next_keys)
            tt = timed(lambda: torch_update(fresh, scores), reps=reps, before=next_keys)
            emu.close()
            emu = BatchedEmulator(game_rom(), n, reward=True, max_episode_steps=a.max_episode_steps)
            emu.bank_create(65536)
            emu.bank_enable_episodes()
            emu.reset()
            ck = timed(lambda: emu.bank_checkpoint(slots), reps=reps, before=next_keys)
            emit(what="update_all_new", envs=n, cells=65536, reps=reps, ms_median=ms, checkpoint_alone_ms=ck,
                 bookkeeping_ms=ms - ck, torch_unique_scatter_sync_ms=tt, not_slower_than_torch=ms - ck <= tt)
            emu.close()
    emit(what="done")


if __name__ == "__main__":
    main()
