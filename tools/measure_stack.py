"""Time pk_fstack_push on the GPU (profiles/stack/measure.jsonl).

The push at 4,096 and 65,536 envs for (scale, depth, layout) = (2, 4, chw), (2, 4, hwc), (4, 3, chw) and
(1, 2, chw): with no mask, and with a mask that fills 1 % of the envs.  The screens are random bytes
written into the handle's screen, so the kernel's arithmetic sees every value; its time does not
depend on them.  HIP events around each call, the median of --reps after --warmup, one process.  Two
yardsticks in the same process, neither taken from the code under test: (a) the torch formulation a
user would write — block mean, roll, where on the done mask — which the push must beat; (b) a
device-to-device hipMemcpyAsync (Tensor.copy_) of the same screens: the push must take at most the
copy's time x (bytes the push moves / bytes the copy moves) x 1.25 at 65,536 envs, the bytes being
reads plus writes from the model: 23,040 of screen, (D - 1) H W read and D H W written per env.
--variant labels the records of a build that is not the kept one (PK_LIB names the library).  There is
no CPU fallback: without a GPU this fails.

    python tools/measure_stack.py --out profiles/stack/measure.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
CONFIGS = ((2, 4, "chw"), (2, 4, "hwc"), (4, 3, "chw"), (1, 2, "chw"))
FACTOR = 1.25


def main():
    import torch
    from pokegym_amd import _native
    from pokegym_amd.emulator import BatchedEmulator
    from pokegym_amd.testrom.game import game_rom

    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--variant", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "a") if a.out else None

    def emit(**rec):
        if a.variant:
            rec["variant"] = a.variant
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

    def torch_push(stack, screen, done, s, layout):
        """What a user writes after every step: downscale, roll, fill the envs that were reset."""
        n = screen.shape[0]
        if s == 1:
            p = screen
        else:
            v = screen.view(n, 144 // s, s, 160 // s, s).sum(dim=(2, 4), dtype=torch.int32)
            p = torch.div(v + s * s // 2, s * s, rounding_mode="floor").to(torch.uint8)
        if layout == "chw":
            stack = torch.roll(stack, 1, dims=1)
            stack[:, 0] = p
            return torch.where(done[:, None, None, None], p[:, None], stack)
        stack = torch.roll(stack, 1, dims=3)
        stack[..., 0] = p
        return torch.where(done[:, None, None, None], p[..., None], stack)

    emit(what="abi", version=_native.ABI_VERSION, reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_name(0),
         library=os.path.basename(_native.LIB_PATH))
    for n in a.envs:
        gen = torch.Generator(device="cuda")
        gen.manual_seed(1)
        copy_ms = None
        for s, depth, layout in CONFIGS:
            emu = BatchedEmulator(game_rom(), n)
            dev = emu.device
            emu.screen.copy_(torch.randint(0, 256, emu.screen.shape, generator=gen, device=dev, dtype=torch.uint8))
            mask = (torch.rand(n, generator=gen, device=dev) < 0.01).to(torch.uint8)
            if copy_ms is None:
                other = torch.empty_like(emu.screen)
                copy_ms = timed(lambda: other.copy_(emu.screen))
                del other
                emit(what="copy_d2d", envs=n, bytes=2 * emu.screen.numel(), ms_median=copy_ms,
                     tb_s=2 * emu.screen.numel() / copy_ms / 1e9)
            emu.stack_create(s, depth, layout, "mean")
            plane = (144 // s) * (160 // s)
            moved = n * (144 * 160 + (2 * depth - 1) * plane)
            bound_ms = copy_ms * moved / (2 * n * 144 * 160) * FACTOR
            # the kernel against the torch formulation, bit for bit, before either is timed
            emu.stack_push(fill_only=True)
            emu.stack_push()
            ref = torch_push(torch_push(torch.zeros_like(emu.stack), emu.screen, mask.bool() | True, s, layout),
                             emu.screen, mask.bool() & False, s, layout)
            assert torch.equal(ref, emu.stack)
            emu.stack_push(mask)
            assert torch.equal(torch_push(ref, emu.screen, mask.bool(), s, layout), emu.stack)
            del ref
            push_ms = timed(lambda: emu.stack_push())
            mask_ms = timed(lambda: emu.stack_push(mask))
            hold = emu.stack.clone()
            done = mask.bool()
            torch_ms = timed(lambda: torch_push(hold, emu.screen, done, s, layout))
            del hold
            for name, ms in (("push", push_ms), ("push_mask_1pct", mask_ms)):
                emit(what=name, envs=n, scale=s, depth=depth, layout=layout, ms_median=ms, bytes=moved, tb_s=moved / ms / 1e9,
                     copy_ms=copy_ms, bound_ms=bound_ms, ratio_to_bound=ms / bound_ms, within_copy_bound=ms <= bound_ms,
                     torch_ms=torch_ms, torch_over_push=torch_ms / ms, faster_than_torch=ms < torch_ms)
            emit(what="torch_push", envs=n, scale=s, depth=depth, layout=layout, ms_median=torch_ms)
            emu.close()
            del emu
            torch.cuda.empty_cache()
    emit(what="done")


if __name__ == "__main__":
    main()
