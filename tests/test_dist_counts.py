"""VecEnv.counts_sync over gloo (world size 2) on the CPU: each rank runs its own host-simulated
VecEnv with its own keys, the ranks exchange what their tables counted, and both end with the sum
of the two.  The collective is pokegym_amd.dist.counts_all_gather."""
import os
import sys
from collections import Counter

import numpy as np
import torch
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from test_dist import _free_port, _worker  # noqa: E402

ENVS = 64


def _sync_fn(rank, world, out_dir):
    sys.path.insert(0, os.path.join(HERE, "hostsim"))
    import counts_common as cc
    from emulator import HostsimEmulator
    from test_hostsim_archive import _NoStream
    from pokegym_amd.env import VecEnv
    from pokegym_amd.testrom.game import game_rom
    for name in ("Stream", "Event", "current_stream", "stream"):
        setattr(torch.cuda, name, _NoStream)
    emu = HostsimEmulator(game_rom(), ENVS, frame_skip=4, release_frame=2, max_episode_steps=100)
    env = VecEnv(ENVS, emulator=emu, log_interval=0, novelty_log2=cc.LG, novelty_key="ram")
    rng = np.random.default_rng(50 + rank)
    env.reset()
    own, tables = Counter(), []
    for rnd in range(2):
        for _ in range(2):
            # the benchmark ROM keeps its player elsewhere: the coordinates the keys read, per rank
            # (x and y in {rank, rank + 1}: overlapping, not equal, key sets)
            emu.set_ram(0xD361, torch.from_numpy(rng.integers(rank, rank + 2, (ENVS, 2)).astype(np.uint8)))
            env.step(torch.from_numpy(rng.integers(0, 8, ENVS).astype(np.uint8)))
            own.update(env.novelty_keys.numpy().view(np.uint64).tolist())
        env.counts_sync()
        tables.append((dict(own), cc.packed(emu).tolist()))
        env.counts_sync()                                        # nothing new: nothing changes
        assert cc.packed(emu).tolist() == tables[-1][1]
    with open(os.path.join(out_dir, f"counts{rank}.txt"), "w") as f:
        f.write(repr(tables))
    emu.close()


def test_counts_sync_gloo_world2(tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path), _sync_fn), nprocs=2, join=True)
    t0, t1 = (eval(open(tmp_path / f"counts{r}.txt").read()) for r in range(2))
    for rnd in range(2):
        own0, own1 = Counter(t0[rnd][0]), Counter(t1[rnd][0])
        assert set(own0) != set(own1) and set(own0) & set(own1)
        union = own0 + own1
        want = [[k, union[k]] for k in sorted(union)]
        assert t0[rnd][1] == want and t1[rnd][1] == want, rnd
        assert sum(union.values()) == 2 * 2 * ENVS * (rnd + 1)
