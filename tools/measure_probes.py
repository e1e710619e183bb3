"""Time pk_probe_eval on the GPU (profiles/probes/measure.jsonl).

One evaluation (reward, done and features of every env) at 4,096 and 65,536 envs for two programs,
probes.pkbench_program() and probes.pokemon_red_program() (which holds the 319-byte bit count).  WRAM and
HRAM hold random bytes, rewritten between the calls that are compared, so the arithmetic sees every
value; the kernel's time does not depend on them.  HIP events around each call, the median of --reps
after --warmup, one process.  The yardstick comes from the same run and not from the code under test:
the torch formulation a user writes today — one get_ram per probe range (a strided array is read as
one span and sliced), byte arithmetic, state tensors — which the kernel must not be slower than at either size.  Before anything is timed the
kernel's rewards, terminals, features and the rewards of a second call are compared with that
formulation bit for bit.  There is no CPU fallback: without a GPU this fails.

    python tools/measure_probes.py --out profiles/probes/measure.jsonl
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

    pop = torch.tensor([bin(i).count("1") for i in range(256)], dtype=torch.int64, device="cuda")

    def torch_eval(emu, prog, state, rew, term, feat):
        """The header's evaluation of every env as a user writes it with get_ram and torch."""
        r = torch.zeros(emu.n, dtype=torch.float64, device=emu.device)
        done = torch.zeros(emu.n, dtype=torch.bool, device=emu.device)
        for j, p in enumerate(prog):
            v = None
            span = (p.count - 1) * p.stride + p.len
            one = p.addr + span <= 0xFE00 and (p.addr & 0x1FFF) + span <= 0x2000 or p.addr >= 0xFF80
            whole = emu.get_ram(p.addr, span).to(torch.int64) if one else None
            for k in range(p.count):
                if one:
                    b = whole[:, k * p.stride:k * p.stride + p.len]
                else:       # the elements lie in more than one region: one read each
                    b = emu.get_ram(p.addr + k * p.stride, p.len).to(torch.int64)
                if p.kind == "bits":
                    x = pop[b].sum(dim=1)
                else:
                    x = torch.zeros(emu.n, dtype=torch.int64, device=emu.device)
                    for i in range(p.len):
                        if p.kind == "le":
                            x = x | (b[:, i] << (8 * i))
                        elif p.kind == "be":
                            x = (x << 8) | b[:, i]
                        else:
                            x = (x * 10 + (b[:, i] >> 4)) * 10 + (b[:, i] & 15)
                v = x if v is None else (torch.maximum(v, x) if p.reduce == "max" else v + x)
            feat[:, j] = v.to(torch.int32)
            if p.done is not None:
                c, arg = p.done
                done |= {"eq": v == arg, "ne": v != arg, "ge": v >= arg, "le": v <= arg}[c]
            if p.op is None:
                continue
            s = state[:, j]
            if p.op == "delta":
                r = r + p.weight * (v - s).to(torch.float64)
                s.copy_(v)
            elif p.op == "newmax":
                r = r + torch.where(v > s, p.weight * (v - s).to(torch.float64), 0.0)
                torch.maximum(s, v, out=s)
            else:
                r = r + torch.where(v != s, torch.tensor(p.weight, dtype=torch.float64, device=emu.device), 0.0)
                s.copy_(v)
        rew += r
        term |= done.to(torch.uint8)

    emit(what="abi", version=_native.ABI_VERSION, reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_name(0),
         library=os.path.basename(_native.LIB_PATH))
    programs = (("pkbench", probes.pkbench_program()), ("pokemon_red", probes.pokemon_red_program()))
    for n in a.envs:
        gen = torch.Generator(device="cuda")
        gen.manual_seed(1)
        rams = [(torch.randint(0, 256, (n, 0x2000), generator=gen, device="cuda", dtype=torch.uint8),
                 torch.randint(0, 256, (n, 0x7F), generator=gen, device="cuda", dtype=torch.uint8)) for _ in range(2)]
        for name, prog in programs:
            m = len(prog)
            loads = sum(p.count * p.len for p in prog)
            emu = BatchedEmulator(game_rom(), n)
            dev = emu.device
            emu.probes_create(prog)
            rew, term = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
            feat = torch.zeros((n, m), dtype=torch.int32, device=dev)
            t_state = torch.zeros((n, m), dtype=torch.int64, device=dev)
            t_rew, t_term, t_feat = torch.zeros_like(rew), torch.zeros_like(term), torch.zeros_like(feat)
            for w, h in rams:       # two evaluations, so that the second one's differences are checked too
                emu.set_ram(0xC000, w)
                emu.set_ram(0xFF80, h)
                emu.probes_eval(rewards=rew, terminals=term, features=feat)
                torch_eval(emu, prog, t_state, t_rew, t_term, t_feat)
                assert torch.equal(rew.view(torch.int64), t_rew.view(torch.int64))
                assert torch.equal(term, t_term) and torch.equal(feat, t_feat)
            ms = timed(lambda: emu.probes_eval(rewards=rew, terminals=term, features=feat))
            rebase_ms = timed(lambda: emu.probes_eval(term, rebase_only=True))
            torch_ms = timed(lambda: torch_eval(emu, prog, t_state, t_rew, t_term, t_feat))
            emit(what="probe_eval", envs=n, program=name, probes=m, yardstick="get_ram per probe range",
                 bytes_read_per_env=loads, ms_median=ms, rebase_only_masked_ms=rebase_ms, torch_ms=torch_ms,
                 torch_over_kernel=torch_ms / ms, not_slower_than_torch=ms <= torch_ms)
            emu.close()
            del emu
            torch.cuda.empty_cache()
    emit(what="done")


if __name__ == "__main__":
    main()
