"""Time pk_frame_keys on the GPU (profiles/cells/measure.jsonl).

pk_frame_keys at 4,096 and 65,536 envs for the parameter sets (16, 16, 8) and (8, 8, 4): keys only,
keys and the cell image, and keys with a salt.  The screens are random bytes written into the
handle's screen, so the kernel's arithmetic sees every value; its time does not depend on them.  HIP
events around each call, the median of --reps after --warmup, one process.  Two yardsticks in the
same process: (a) bounded: a device-to-device hipMemcpyAsync (Tensor.copy_) of the same range's
screen bytes — the kernel reads what the copy reads and writes almost nothing, so a call must take
no longer than the copy; (b) unbounded: the same cells in torch (shift, reshape, sum, multiply,
floor-divide), which stops before the keys.  There is no CPU fallback: without a GPU this fails.

    python tools/measure_cells.py --out profiles/cells/measure.jsonl
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
    import torch
    from pokegym_amd import _native
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
    out = open(a.out, "a") if a.out else None

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
        return statistics.median(ms)

    def torch_cells(screen, bw, bh, levels):
        n = screen.shape[0]
        v = (screen >> 6).view(n, 144 // bh, bh, 160 // bw, bw)
        s = v.sum(dim=(2, 4), dtype=torch.int32)
        return torch.div(s * levels, 3 * bw * bh + 1, rounding_mode="floor").to(torch.uint8).view(n, -1)

    emit(what="abi", version=_native.ABI_VERSION, reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_name(0),
         library=os.path.basename(_native.LIB_PATH))
    for n in a.envs:
        emu = BatchedEmulator(game_rom(), n)
        dev = emu.device
        gen = torch.Generator(device=dev)
        gen.manual_seed(1)
        emu.screen.copy_(torch.randint(0, 256, emu.screen.shape, generator=gen, device=dev, dtype=torch.uint8))
        other = torch.empty_like(emu.screen)
        keys = torch.zeros(n, dtype=torch.int64, device=dev)
        salt = torch.randint(0, 1 << 62, (n,), generator=gen, device=dev, dtype=torch.int64)
        nbytes = emu.screen.numel()
        copy_ms = timed(lambda: other.copy_(emu.screen))
        emit(what="copy_d2d", envs=n, bytes=nbytes, ms_median=copy_ms, read_tb_s=nbytes / copy_ms / 1e9)
        for bw, bh, levels in ((16, 16, 8), (8, 8, 4)):
            cells = torch.zeros((n, emu.frame_cells(bw, bh)), dtype=torch.uint8, device=dev)
            cases = {"keys": lambda: emu.frame_keys(bw, bh, levels, out=keys),
                     "keys_cells": lambda: emu.frame_keys(bw, bh, levels, out=keys, cells=cells),
                     "keys_salt": lambda: emu.frame_keys(bw, bh, levels, salt=salt, out=keys)}
            for name, fn in cases.items():
                ms = timed(fn)
                emit(what=name, envs=n, bw=bw, bh=bh, levels=levels, ms_median=ms, read_tb_s=nbytes / ms / 1e9,
                     copy_ms=copy_ms, ratio_to_copy=ms / copy_ms, within_bound=ms <= copy_ms)
            tt = timed(lambda: torch_cells(emu.screen, bw, bh, levels))
            assert torch.equal(torch_cells(emu.screen, bw, bh, levels), cells)
            emit(what="torch_cells", envs=n, bw=bw, bh=bh, levels=levels, ms_median=tt)
        emu.close()
    emit(what="done")


if __name__ == "__main__":
    main()
