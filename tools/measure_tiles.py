"""Time pk_tiles_eval on the GPU (profiles/tiles/measure.jsonl).

4,096 and 65,536 envs of the benchmark ROM, stepped a few times with random actions so that the envs
differ, then one evaluation of every env: id mode and hash mode (12 bits), with and without the object
plane, with and without keys.  HIP events around each call, the median of --reps after --warmup, one
process.  Before the timing the view and the keys of the first 256 envs are compared with the numpy
model (pokegym_amd/tiles.py) applied to their snapshots.  The yardstick, from the same handle and env
count: pk_frame_keys with (bw, bh, levels) = (8, 8, 4), which reads the 23,040-byte screen where the
tile view reads 720 map bytes, 160 OAM bytes and in hash mode at most 16 x 720 tile bytes.  Expected:
id mode no slower than the yardstick, hash mode within 2 x.  There is no CPU fallback: without a GPU
this fails.

    python tools/measure_tiles.py --out profiles/tiles/measure.jsonl
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
    from pokegym_amd import _native, tiles
    from pokegym_amd.emulator import BatchedEmulator
    from pokegym_amd.testrom.game import game_rom

    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=6)
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

    emit(what="abi", version=_native.ABI_VERSION, reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_name(0),
         yardstick="pk_frame_keys (8, 8, 4)")
    for n in a.envs:
        acts = torch.from_numpy(np.random.default_rng(0).integers(0, 8, (a.steps, n), dtype=np.uint8)).cuda()
        yard = None
        for mode, objects in (("id", True), ("id", False), ("hash", True), ("hash", False)):
            # a handle per variant (a view is created once per handle), stepped alike
            emu = BatchedEmulator(game_rom(), n, reward=False)
            emu.tiles_create(mode, 12, objects)
            emu.reset()
            for t in range(a.steps):
                emu.step(acts[t])
            keys = torch.zeros(n, dtype=torch.int64, device=emu.device)
            emu.tiles_eval(keys=keys)
            k = min(n, 256)
            want = tiles.from_states(emu.snapshot_range(0, k), mode=mode, bits=12, obj=objects)
            got = emu.tiles[:k].cpu().numpy().view(np.uint16)
            ok = bool(np.array_equal(got, want)
                      and np.array_equal(keys[:k].cpu().numpy().view(np.uint64), tiles.key_model(want)))
            distinct = len({v.tobytes() for v in got})
            emit(what="model_check", envs=n, mode=mode, objects=objects, compared=k, distinct_views=distinct, ok=ok)
            assert ok, "the view differs from the model"
            if yard is None:
                fk = torch.zeros(n, dtype=torch.int64, device=emu.device)
                ms = timed(lambda: emu.frame_keys(8, 8, 4, out=fk))
                yard = statistics.median(ms)
                emit(what="frame_keys_8_8_4", envs=n, ms_median=yard, ms_min=min(ms), ms_max=max(ms),
                     bytes_read=n * 23040, gbytes_per_s=n * 23040 / yard / 1e6)
            for with_keys in (False, True):
                ms = timed(lambda: emu.tiles_eval(keys=keys if with_keys else None))
                med = statistics.median(ms)
                bound = 1.0 if mode == "id" else 2.0
                emit(what="tiles_eval", envs=n, mode=mode, objects=objects, keys=with_keys, ms_median=med, ms_min=min(ms),
                     ms_max=max(ms), bytes_written=n * emu.tile_planes * 720, yardstick_ms=yard, ratio=med / yard,
                     bound=bound, ok=med / yard <= bound)
            emu.close()
            del emu, keys
            torch.cuda.empty_cache()
    emit(what="done")


if __name__ == "__main__":
    main()
