"""Shared scenarios of the frame-cell tests (pk_frame_keys / pk_frame_cells, ABI v12):
test_hostsim_cells.py runs them on the host-simulation build, test_gpu_cells.py on the gfx950 build.
The oracle is the model of include/pokegym_amd.h, stated once here in numpy (model).  Screens are
written straight into emu.screen, the writable tensor over pk_screen_ptr."""
import os

import numpy as np

import episodes_common as ec

N = 192                 # three 64-env groups
ROWS, COLS = 144, 160
M64 = (1 << 64) - 1
NOKEY = np.uint64(M64)
GOLD = np.uint64(0x9E3779B97F4A7C15)
GREY = np.array([0xFF, 0x99, 0x55, 0x00], np.uint8)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ppu_states.npz")
BW = (8, 16, 32, 40, 80, 160)
BH = (8, 16, 24, 48, 72, 144)
RANDOM_SETS = [(8, 8, 4), (16, 16, 8), (32, 24, 8), (40, 48, 3), (80, 72, 16), (160, 144, 256), (8, 144, 2), (160, 8, 255)]
# (bw, bh, levels) -> distinct keys = distinct cell rows over the 264 reference frames (236 distinct
# frames), from this model on the CPU
FRAME_SETS = {(8, 8, 4): 231, (16, 16, 8): 229, (32, 24, 8): 216, (80, 72, 16): 181, (160, 144, 256): 118, (16, 16, 2): 187}


def mix(z):
    """splitmix64's finaliser over a uint64 array (sums and products mod 2^64)."""
    z = np.asarray(z, np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def model(screens, bw, bh, levels, salt=None):
    """(keys uint64 (k,), cells uint8 (k, C)) of uint8 (k, 144, 160) screens."""
    screens = np.asarray(screens, np.uint8)
    k = len(screens)
    nbx, nby = COLS // bw, ROWS // bh
    v = (screens >> 6).astype(np.uint64)
    s = v.reshape(k, nby, bh, nbx, bw).sum(axis=(2, 4)).reshape(k, nbx * nby)     # block i = by * nbx + bx
    q = s * np.uint64(levels) // np.uint64(3 * bw * bh + 1)
    assert q.max() < levels
    i = np.arange(1, nbx * nby + 1, dtype=np.uint64)
    total = mix(GOLD * i[None, :] + q).sum(axis=1, dtype=np.uint64)
    if salt is not None:
        salt = np.asarray(salt).view(np.uint64)
        total = total + mix(salt)
    keys = mix(total)
    keys[keys == NOKEY] = NOKEY - np.uint64(1)
    if salt is not None:
        keys[salt == NOKEY] = NOKEY
    return keys, q.astype(np.uint8)


def u64(t):
    """An int64 key tensor as a host uint64 array."""
    return t.cpu().numpy().view(np.uint64)


def random_screens(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, ROWS, COLS), dtype=np.uint8)


def put_screens(emu, screens, dev):
    emu.screen.copy_(dev(screens, np.uint8))


def fresh_cells(emu, bw, bh, dev, fill=0xEE):
    return dev(np.full((emu.n, emu.frame_cells(bw, bh)), fill), np.uint8)


def check_random(make, dev):
    """Uniform random bytes, every value: keys and cell rows equal the model for eight parameter
    sets, and the keys are the same without cells_dev."""
    emu = make(N)
    screens = random_screens(N, 1)
    assert len(np.unique(screens)) == 256
    put_screens(emu, screens, dev)
    for bw, bh, levels in RANDOM_SETS:
        want_k, want_c = model(screens, bw, bh, levels)
        assert emu.frame_cells(bw, bh) == want_c.shape[1]
        cells = fresh_cells(emu, bw, bh, dev)
        keys = emu.frame_keys(bw, bh, levels, cells=cells)
        assert np.array_equal(u64(keys), want_k), (bw, bh, levels)
        assert np.array_equal(cells.cpu().numpy(), want_c), (bw, bh, levels)
        assert np.array_equal(u64(emu.frame_keys(bw, bh, levels)), want_k), (bw, bh, levels)
    emu.close()


def check_reference_frames(make, dev):
    """The 264 reference frames in a 320-env handle (the other 56 envs hold frame 0): keys equal the
    model, and as many distinct keys as distinct cell rows — the counts the model gives on the CPU."""
    frames = GREY[np.load(FIXTURE)["frames"]]
    k = len(frames)
    assert frames.shape == (264, ROWS, COLS) and len(np.unique(frames.reshape(k, -1), axis=0)) == 236
    n = 320
    screens = np.concatenate([frames, np.repeat(frames[:1], n - k, axis=0)])
    emu = make(n)
    put_screens(emu, screens, dev)
    for (bw, bh, levels), distinct in FRAME_SETS.items():
        want_k, want_c = model(screens, bw, bh, levels)
        cells = fresh_cells(emu, bw, bh, dev)
        keys = u64(emu.frame_keys(bw, bh, levels, cells=cells))
        assert np.array_equal(keys, want_k), (bw, bh, levels)
        rows = len(np.unique(cells.cpu().numpy()[:k], axis=0))
        assert len(np.unique(keys[:k])) == rows == distinct, (bw, bh, levels, len(np.unique(keys[:k])), rows)
        assert (keys[k:] == keys[0]).all()
    emu.close()


def one_pixel_positions():
    pos = [(0, 0), (0, 159), (143, 0), (143, 159)]                       # the corners
    pos += [(0, x) for x in range(16)]                                   # every byte of piece 0 ...
    pos += [(143, 144 + x) for x in range(16)]                           # ... and of piece 1,439
    pos += [(y, x) for y in (7, 8, 143) for x in (0, 159)]
    pos += [(72, x) for x in (7, 8, 15, 16, 159)]
    return pos


def check_one_pixel(make, dev):
    """(8, 8, 256): 256 / 193 > 1, so every unit of a block's sum moves its level.  One pixel of a
    0x55 screen raised to 0xFF changes the key, whatever byte of a piece and whatever tile edge it
    sits on, and changes it alike for every pixel of one block."""
    pos = one_pixel_positions()
    screens = np.full((N, ROWS, COLS), 0x55, np.uint8)
    for e, (y, x) in enumerate(pos, start=1):
        screens[e, y, x] = 0xFF
    emu = make(N)
    put_screens(emu, screens, dev)
    want_k, want_c = model(screens, 8, 8, 256)
    cells = fresh_cells(emu, 8, 8, dev)
    keys = u64(emu.frame_keys(8, 8, 256, cells=cells))
    assert np.array_equal(keys, want_k) and np.array_equal(cells.cpu().numpy(), want_c)
    base = keys[0]
    assert (keys[len(pos) + 1:] == base).all()
    block = {}
    for e, (y, x) in enumerate(pos, start=1):
        assert keys[e] != base, (y, x)
        block.setdefault((y // 8, x // 8), []).append(e)
    shared = [es for es in block.values() if len(es) > 1]
    assert len(shared) >= 4                                              # the corners' blocks, pieces 0 and 1,439
    for es in shared:
        assert len({int(keys[e]) for e in es}) == 1, es
    assert len({int(keys[es[0]]) for es in block.values()}) == len(block)
    emu.close()


def check_ranges(make, dev, streams=None):
    """A call over [64, 104) writes those 40 keys and rows only.  streams = a function (first,
    second) that runs two calls on two streams: ranges [0, 64) and [64, 192) then equal one call."""
    emu = make(N)
    screens = random_screens(N, 2)
    put_screens(emu, screens, dev)
    for bw, bh, levels in ((16, 16, 8), (8, 8, 4)):
        want_k, want_c = model(screens, bw, bh, levels)
        keys = dev(np.full(N, -5), np.int64)
        cells = fresh_cells(emu, bw, bh, dev)
        emu.frame_keys(bw, bh, levels, out=keys, cells=cells, env0=64, count=40)
        k, c = keys.cpu().numpy(), cells.cpu().numpy()
        assert np.array_equal(k[64:104].view(np.uint64), want_k[64:104]) and (k[:64] == -5).all() and (k[104:] == -5).all()
        assert np.array_equal(c[64:104], want_c[64:104]) and (c[:64] == 0xEE).all() and (c[104:] == 0xEE).all()
        if streams is not None:
            keys.fill_(-5)
            cells.fill_(0xEE)
            streams(lambda: emu.frame_keys(bw, bh, levels, out=keys, cells=cells, env0=0, count=64),
                    lambda: emu.frame_keys(bw, bh, levels, out=keys, cells=cells, env0=64, count=128))
            assert np.array_equal(u64(keys), want_k) and np.array_equal(cells.cpu().numpy(), want_c)
    emu.close()


def check_salt(make, dev):
    emu = make(N)
    screens = random_screens(N, 3)
    screens[1] = screens[0]                                              # equal screens, different salts
    salt = np.random.default_rng(4).integers(0, 1 << 63, N, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    salt[3] = salt[2]                                                    # equal salts, different screens
    salt[[7, 64, 191]] = NOKEY
    salt[8] = 0
    put_screens(emu, screens, dev)
    plain, _ = model(screens, 16, 16, 8)
    want, _ = model(screens, 16, 16, 8, salt)
    got = u64(emu.frame_keys(16, 16, 8, salt=dev(salt.view(np.int64), np.int64)))
    assert np.array_equal(got, want)
    assert (got[[7, 64, 191]] == NOKEY).all() and (np.delete(got, [7, 64, 191]) != NOKEY).all()
    assert got[0] != got[1] and got[2] != got[3] and plain[0] == plain[1]
    assert got[8] == plain[8] and (np.delete(got, 8) != np.delete(plain, 8)).all()   # mix(0) = 0: the one salt that adds nothing
    inplace = dev(salt.view(np.int64), np.int64)
    assert emu.frame_keys(16, 16, 8, salt=inplace, out=inplace) is inplace
    assert np.array_equal(u64(inplace), want)
    emu.close()


def check_screen_source(make, dev):
    emu = make(N)
    screens = random_screens(N, 5)
    put_screens(emu, screens, dev)
    want, _ = model(screens, 16, 16, 8)
    own = u64(emu.frame_keys())
    copy = emu.screen.clone()
    emu.screen.zero_()
    assert np.array_equal(own, want) and np.array_equal(u64(emu.frame_keys(screen=copy)), want)
    emu.close()
    blind = make(N, render=False)
    keys = dev(np.full(N, -5), np.int64)
    L, h = blind._L, blind._h
    assert L.pk_frame_keys(h, 16, 16, 8, None, None, keys.data_ptr(), None, 0, N, None) < 0 and L.pk_last_error()
    assert (keys.cpu().numpy() == -5).all()
    assert np.array_equal(u64(blind.frame_keys(screen=copy, out=keys)), want)
    blind.close()


def check_guards(make, dev):
    emu = make(N)
    L, h = emu._L, emu._h
    put_screens(emu, random_screens(N, 6), dev)
    keys = dev(np.full(N, -5), np.int64)
    cells = dev(np.full((N, 360), 0xEE), np.uint8)
    kp, cp = keys.data_ptr(), cells.data_ptr()

    def refused(bw, bh, levels, k, env0, count, screen=None):
        assert L.pk_frame_keys(h, bw, bh, levels, screen, None, k, cp, env0, count, None) < 0, (bw, bh, levels, env0, count)
        assert L.pk_last_error()
        assert (keys.cpu().numpy() == -5).all() and (cells.cpu().numpy() == 0xEE).all()

    for bw in (0, 4, 12, 24, 64):
        refused(bw, 16, 8, kp, 0, N)
    for bh in (0, 4, 32, 36):
        refused(16, bh, 8, kp, 0, N)
    for levels in (0, 1, 257):
        refused(16, 16, levels, kp, 0, N)
    refused(16, 16, 8, None, 0, N)                                       # NULL keys
    refused(16, 16, 8, kp, 128, 65)                                      # a range past n
    refused(16, 16, 8, kp, 32, 8)                                        # check_range: the start is no multiple of 64
    refused(16, 16, 8, kp, 0, 0)
    refused(16, 16, 8, kp, 0, N, emu.screen.data_ptr() + 8)              # a misaligned screen
    assert L.pk_frame_keys(h, 16, 16, 8, None, None, kp, cp, 128, 64, None) == 0   # the last group is a legal range
    for bw in range(0, 200):
        for bh in range(0, 200):
            want = (COLS // bw) * (ROWS // bh) if bw in BW and bh in BH else 0
            assert L.pk_frame_cells(bw, bh) == want, (bw, bh)
    assert len(BW) * len(BH) == 36
    emu.close()


def emulator_scenario(make, dev):
    """128 envs of the benchmark ROM, six random-action steps: keys equal the model over emu.screen
    after the reset and after every step; env 5, checkpointed at step 3 and resumed into env 70 at
    step 6, has the key it had at step 3.  Returns every key read."""
    n, steps = 128, 6
    emu = make(n, reward=True, max_episode_steps=ec.MAX_STEPS)
    emu.bank_create(2)
    emu.bank_enable_episodes()
    acts = dev(np.random.default_rng(7).integers(0, 8, (steps, n)), np.uint8)
    seen = []

    def read():
        want, want_c = model(emu.screen.cpu().numpy(), 16, 16, 8)
        cells = fresh_cells(emu, 16, 16, dev)
        keys = u64(emu.frame_keys(cells=cells))
        assert np.array_equal(keys, want) and np.array_equal(cells.cpu().numpy(), want_c), len(seen)
        seen.append(keys)
        return keys

    emu.reset()
    read()
    for t in range(steps):
        emu.step(acts[t])
        keys = read()
        if t == 2:
            held = keys[5]
            emu.bank_checkpoint(dev(ec.slot_map({5: 1}, n)))
    emu.bank_resume(dev(ec.slot_map({70: 1}, n)))
    keys = read()
    assert keys[70] == held and emu.bank_rejects() == 0
    assert np.array_equal(np.delete(keys, 70), np.delete(seen[-2], 70))
    emu.close()
    return np.stack(seen)


def check_with_emulator(make, dev):
    a = emulator_scenario(make, dev)
    b = emulator_scenario(make, dev)
    assert np.array_equal(a, b)


def ram_keys(env):
    """pk_cell_keys at shift 0 from the RAM bytes, env order."""
    pos = env.emu.get_ram(0xD35E, 5).cpu().numpy().astype(np.uint64)
    badges = env.emu.get_ram(0xD356, 1).cpu().numpy().astype(np.uint64)[:, 0]
    keys = pos[:, 0] | pos[:, 4] << np.uint64(8) | pos[:, 3] << np.uint64(16) | badges << np.uint64(24)
    return keys[[env.phys(e) for e in range(env.num_envs)]]


def check_vecenv(make_env, dev):
    """make_env(**kw): VecEnv(48, batch_size=24, bank_episodes=True, archive_cells=8, **kw), padded
    slots.  The frame keys and the cell image come back in env order; archive_update() by default
    keys equals archive_update(keys=<model keys>) on a twin; the default VecEnv keeps the RAM keys."""
    def play(env):
        rng = np.random.default_rng(9)
        env.reset()
        for _ in range(2):
            env.emu.set_ram(0xD361, dev(rng.integers(0, 3, (env.emu.n, 2)), np.uint8))
            env.step(dev(rng.integers(0, 8, env.num_envs), np.uint8))
        # frames that differ from env to env, whatever the ROM drew (the same on a twin): four blocks
        # of 16 x 24 pixels, each of one shade
        shades = GREY[rng.integers(0, 4, (env.emu.n, 4))]
        env.emu.screen[:, 48:72, 16:80] = dev(np.repeat(shades, 16, axis=1)[:, None, :].repeat(24, axis=1), np.uint8)

    for name in ("frame", "frame+ram"):
        env, twin = make_env(archive_key=name, archive_frame=(16, 24, 5)), make_env(archive_key=name, archive_frame=(16, 24, 5))
        assert env.emu.n == 128 and env.archive_key == name and env.archive_frame == (16, 24, 5)
        for v in (env, twin):
            play(v)
        order = [env.phys(e) for e in range(env.num_envs)]
        screens = env.emu.screen.cpu().numpy()[order]
        want_k, want_c = model(screens, 16, 24, 5, ram_keys(env) if name == "frame+ram" else None)
        assert len(np.unique(want_k)) > 8                                # the 8-cell archive overflows
        assert np.array_equal(u64(env.cell_keys()), want_k), name
        assert np.array_equal(env.frame_cells().cpu().numpy(), want_c), name
        won = env.archive_update().cpu().numpy()
        won_twin = twin.archive_update(keys=dev(want_k.view(np.int64), np.int64)).cpu().numpy()
        a, b = env.archive_state(), twin.archive_state()
        assert a["used"] == 8 and a["overflow"] > 0 and np.array_equal(won, won_twin)
        for k in a:
            assert np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k], (name, k)
        assert a["keys"].tolist() == list(dict.fromkeys(want_k.tolist()))[:8]
        env.emu.close()
        twin.emu.close()
    plain = make_env()
    assert plain.archive_key == "ram"
    play(plain)
    assert np.array_equal(u64(plain.cell_keys()), ram_keys(plain))
    plain.emu.close()
