"""Time the visit-count table on the GPU (profiles/counts/measure.jsonl).

pk_counts_update at 4,096 and 65,536 envs on a table of 2^22 entries, in four regimes: every key new
and distinct, every key stored and distinct, every env on one key, and the frame keys of pkbench
after 64 random steps; pk_counts_add and pk_counts_pack of 2^20 records.  HIP events around each
call, the median of --reps after --warmup, one process.  The yardstick, in the same process, is the
torch formulation the table replaces: a sorted key tensor and a count tensor, torch.unique with the
inverse and the counts, searchsorted, a merge of the new keys, and rsqrt for the bonus (TorchCounts);
its results are compared with the table's.  The bound: no call is slower than its yardstick.
pk_frame_keys at the same sizes is recorded beside them for scale.  --variant names the build
measured (PK_LIB selects it).  There is no CPU fallback: without a GPU this fails.

    python tools/measure_counts.py --out profiles/counts/measure.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

LG = 22
RECORDS = 1 << 20


def main():
    import torch
    from pokegym_amd import _native
    from pokegym_amd.emulator import BatchedEmulator
    from pokegym_amd.testrom.game import game_rom

    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--variant", default="kept")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "a") if a.out else None
    calls = a.warmup + a.reps

    def emit(**rec):
        line = json.dumps(dict(rec, variant=a.variant))
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def timed(fn, before=None):
        """Median of fn(k) over the timed calls; before(k) runs untimed ahead of each."""
        ms = []
        for k in range(calls):
            if before:
                before(k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(k)
            e1.record()
            e1.synchronize()
            if k >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return statistics.median(ms)

    class TorchCounts:
        """The same table in torch: sorted keys (as int64) and their counts."""

        def __init__(self, dev):
            self.keys = torch.empty(0, dtype=torch.int64, device=dev)
            self.cnt = torch.empty(0, dtype=torch.int64, device=dev)

        def add(self, uniq, m):
            """uniq sorted and distinct, m their amounts."""
            if self.keys.numel():
                pos = torch.searchsorted(self.keys, uniq).clamp_(max=self.keys.numel() - 1)
                hit = self.keys[pos] == uniq
                self.cnt.index_add_(0, pos[hit], m[hit])
                uniq, m = uniq[~hit], m[~hit]
            if uniq.numel():        # the merge
                keys, cnt = torch.cat([self.keys, uniq]), torch.cat([self.cnt, m])
                self.keys, order = torch.sort(keys)
                self.cnt = cnt[order]

        def update(self, keys, beta=1.0):
            uniq, m = torch.unique(keys, return_counts=True)
            self.add(uniq, m)
            c = self.cnt[torch.searchsorted(self.keys, keys)]
            return c, beta * torch.rsqrt(c.to(torch.float64))

        def add_records(self, rec):
            uniq, inv = torch.unique(rec[:, 0], return_inverse=True)
            self.add(uniq, torch.zeros_like(uniq).index_add_(0, inv, rec[:, 1]))

        def pack(self):
            sel = self.cnt != 0
            return torch.stack([self.keys[sel], self.cnt[sel]], dim=1)

    def distinct(k, n, dev):
        """n distinct keys, different for every k."""
        return (torch.arange(k * n + 1, (k + 1) * n + 1, dtype=torch.int64, device=dev) * -7046029254386353131)

    emit(what="abi", version=_native.ABI_VERSION, reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_name(0),
         library=os.path.basename(_native.LIB_PATH), cap_log2=LG)
    for n in a.envs:
        emu = BatchedEmulator(game_rom(), n)
        dev = emu.device
        emu.counts_create(LG)
        c_out = torch.zeros(n, dtype=torch.int64, device=dev)
        b_out = torch.zeros(n, dtype=torch.float64, device=dev)
        keys_out = torch.zeros(n, dtype=torch.int64, device=dev)
        ref = TorchCounts(dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(2)
        emu.reset()
        for _ in range(64):
            emu.step(torch.randint(0, 8, (n,), generator=gen, device=dev, dtype=torch.uint8))
        frame = emu.frame_keys().clone()
        regimes = {"new_distinct": lambda k: distinct(k, n, dev), "known_distinct": lambda k: distinct(calls - 1, n, dev),
                   "one_key": lambda k: torch.full((n,), 12345, dtype=torch.int64, device=dev), "frame_keys": lambda k: frame}
        for name, make in regimes.items():
            sets = [make(k) for k in range(calls)]
            ms = timed(lambda k: emu.counts_update(sets[k], None, 0, n, 1.0, False, c_out, b_out))
            got = (c_out.clone(), b_out.clone())
            res = []
            tt = timed(lambda k: res.append(ref.update(sets[k])))
            assert torch.equal(got[0], res[-1][0]), name
            err = float((got[1] - res[-1][1]).abs().max())       # torch's rsqrt is not the correctly rounded quotient
            emit(what="update", regime=name, envs=n, distinct=int(torch.unique(sets[-1]).numel()), ms_median=ms,
                 torch_ms=tt, ratio_to_torch=ms / tt, within_bound=ms <= tt, max_bonus_diff=err)
        emit(what="update_peek", envs=n, ms_median=timed(lambda k: emu.counts_update(frame, None, 0, n, 1.0, True, c_out, b_out)))
        emit(what="frame_keys_call", envs=n, ms_median=timed(lambda k: emu.frame_keys(out=keys_out)))
        emit(what="table", envs=n, **emu.counts_read())
        emu.close()
    # pack and add of 2^20 records, on a small handle
    emu = BatchedEmulator(game_rom(), 64)
    dev = emu.device
    emu.counts_create(LG)
    rec = torch.stack([distinct(0, RECORDS, dev), torch.arange(1, RECORDS + 1, dtype=torch.int64, device=dev)], dim=1).contiguous()
    refs = [TorchCounts(dev) for _ in range(calls)]
    ms = timed(lambda k: emu.counts_add(rec), before=lambda k: emu.counts_clear())
    tt = timed(lambda k: refs[k].add_records(rec))
    emit(what="add", regime="new", records=RECORDS, ms_median=ms, torch_ms=tt, ratio_to_torch=ms / tt, within_bound=ms <= tt)
    ms = timed(lambda k: emu.counts_add(rec, foreign=True))
    tt = timed(lambda k: refs[0].add_records(rec))
    emit(what="add", regime="known_foreign", records=RECORDS, ms_median=ms, torch_ms=tt, ratio_to_torch=ms / tt,
         within_bound=ms <= tt)
    for name, delta in (("full", False), ("delta", True)):
        # every timed delta pack has 2^20 records to send: the counts move between the packs
        before = (lambda k: emu.counts_add(rec)) if delta else None
        ms = timed(lambda k: emu.counts_pack_raw(delta), before=before)
        tt = timed(lambda k: refs[0].pack())
        n_packed = int(emu.counts_pack_raw(False)[1])
        emit(what="pack", regime=name, records=n_packed, ms_median=ms, torch_ms=tt, ratio_to_torch=ms / tt,
             within_bound=ms <= tt)
    got = emu.counts_pack()
    want = refs[1].pack()
    assert torch.equal(got[:, 0], torch.sort(want[:, 0] ^ torch.iinfo(torch.int64).min)[0] ^ torch.iinfo(torch.int64).min)
    emu.close()
    emit(what="done")


if __name__ == "__main__":
    main()
