"""VecEnv.archive_sync over gloo (world size 2) on the CPU: each rank runs its own host-simulated
VecEnv with its own actions, the ranks exchange what their archives learned, and both end with the
same table key -> (score, length, visits).  The collective is pokegym_amd.dist.archive_all_gather."""
import os
import sys

import numpy as np
import torch
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from test_dist import _free_port, _worker  # noqa: E402

ENVS, CELLS = 8, 12


def _table(env):
    st = env.archive_state()
    u = st["used"]
    return {int(k): (float(s), int(ln), int(v)) for k, s, ln, v in
            zip(st["keys"][:u], st["scores"][:u], st["lengths"][:u], st["visits"][:u])}


def _sync_fn(rank, world, out_dir):
    sys.path.insert(0, os.path.join(HERE, "hostsim"))
    from emulator import HostsimEmulator
    from test_hostsim_archive import _NoStream
    from pokegym_amd.env import VecEnv
    from pokegym_amd.testrom.game import game_rom
    for name in ("Stream", "Event", "current_stream", "stream"):
        setattr(torch.cuda, name, _NoStream)
    emu = HostsimEmulator(game_rom(), ENVS, frame_skip=4, release_frame=2, reward=True, max_episode_steps=12)
    env = VecEnv(ENVS, emulator=emu, log_interval=0, bank_slots=1, bank_episodes=True, archive_cells=CELLS,
                 archive_exchange=True)
    rng = np.random.default_rng(40 + rank)
    env.reset()
    tables = []
    for rnd in range(2):
        for _ in range(2):
            # the benchmark ROM keeps its player elsewhere: the coordinates the keys read, per rank
            # (x and y in {rank, rank + 1}: overlapping, not equal, key sets)
            pos = rng.integers(rank, rank + 2, (ENVS, 2)).astype(np.uint8)
            pos[0] = 1                                           # a key both ranks reach
            emu.set_ram(0xD361, torch.from_numpy(pos))
            env.step(torch.from_numpy(rng.integers(0, 8, ENVS).astype(np.uint8)))
        env.archive_update(scores=torch.from_numpy(rng.integers(0, 4, ENVS).astype(np.float64)))
        own = _table(env)
        env.archive_sync()
        tables.append((own, _table(env)))
    env.archive_sync()                                           # nothing new: nothing changes
    assert _table(env) == tables[-1][1]
    with open(os.path.join(out_dir, f"sync{rank}.txt"), "w") as f:
        f.write(repr((tables, _table(env), env.emu.bank_rejects())))
    emu.close()


def test_archive_sync_gloo_world2(tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path), _sync_fn), nprocs=2, join=True)
    got = [eval(open(tmp_path / f"sync{r}.txt").read()) for r in range(2)]
    (t0, final0, rej0), (t1, final1, rej1) = got
    assert rej0 == rej1 == 0
    assert final0 == final1 and len(final0) > 0
    # every rank's own visits are in the common table exactly once
    own0, own1 = t0[0][0], t1[0][0]
    assert set(own0) != set(own1) and set(own0) & set(own1)
    assert t0[0][1] == t1[0][1]
    for k, (s, ln, v) in t0[0][1].items():
        assert v == own0.get(k, (0, 0, 0))[2] + own1.get(k, (0, 0, 0))[2], k
        assert (s, ln) == min((x[k][:2] for x in (own0, own1) if k in x), key=lambda r: (-r[0], r[1])), k
    assert sum(v for _, _, v in final0.values()) == 2 * 2 * ENVS
