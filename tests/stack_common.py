"""Shared scenarios of the frame-stack tests (pk_fstack_*): test_hostsim_stack.py runs them on the
host-simulation build, test_gpu_stack.py on the gfx950 build.  The oracle is the model of
include/pokegym_amd.h, stated once here in numpy (plane, Model).  make(n, **kw) builds an emulator,
dev(values, dtype) a tensor on its device."""
import functools
import os

import numpy as np
import pytest

import episodes_common as ec

ROWS, COLS = 144, 160
GREY = np.array([0xFF, 0x99, 0x55, 0x00], np.uint8)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ppu_states.npz")
# (scale, depth, layout, mode)
CONFIGS = [(1, 1, "chw", "mean"), (2, 4, "chw", "mean"), (2, 4, "hwc", "mean"), (2, 4, "chw", "pick"),
           (4, 3, "chw", "mean"), (4, 8, "hwc", "pick"), (2, 8, "chw", "mean"), (1, 2, "hwc", "mean")]
FILL_ONLY = 1


def plane(screens, s, mode):
    """The header's plane of uint8 (k, 144, 160) screens: uint8 (k, 144 / s, 160 / s)."""
    screens = np.asarray(screens, np.uint8)
    k = len(screens)
    a = screens.reshape(k, ROWS // s, s, COLS // s, s)
    if mode == "pick":
        return np.ascontiguousarray(a[:, :, 0, :, 0])
    return ((a.astype(np.uint32).sum(axis=(2, 4)) + s * s // 2) // (s * s)).astype(np.uint8)


class Model:
    """The header's stack of n envs, kept as (n, D, H, W) whatever the layout."""

    def __init__(self, n, s, depth, layout, mode):
        self.n, self.s, self.depth, self.layout, self.mode = n, s, depth, layout, mode
        self.st = np.zeros((n, depth, ROWS // s, COLS // s), np.uint8)

    def load(self, stack):
        """Take a stack in the layout's shape as the state."""
        stack = np.asarray(stack, np.uint8)
        self.st = np.ascontiguousarray(stack.transpose(0, 3, 1, 2) if self.layout == "hwc" else stack).copy()

    def push(self, screens, mask=None, fill_only=False, env0=0, count=None):
        p = plane(screens, self.s, self.mode)
        r = np.arange(env0, self.n if count is None else env0 + count)
        m = None if mask is None else np.asarray(mask)[r] != 0
        if fill_only:
            fill, shift = (r if m is None else r[m]), r[:0]
        else:
            fill, shift = (r[:0] if m is None else r[m]), (r if m is None else r[~m])
        self.st[shift] = np.concatenate([p[shift][:, None], self.st[shift][:, :-1]], axis=1)
        self.st[fill] = p[fill][:, None]

    def view(self):
        return self.st.transpose(0, 2, 3, 1) if self.layout == "hwc" else self.st


def got(emu):
    return emu.stack.cpu().numpy()


def same(emu, model, what=None):
    assert np.array_equal(got(emu), model.view()), what


@functools.lru_cache(maxsize=None)
def random_screens(n, seed):
    """uint8 (n, 144, 160), every byte value; computed once and shared: nobody writes into it."""
    a = np.random.default_rng(seed).integers(0, 256, (n, ROWS, COLS), dtype=np.uint8)
    assert len(np.unique(a)) == 256
    return a


def create(emu, s, depth, layout, mode):
    emu.stack_create(s, depth, layout, mode)
    shape = (depth, ROWS // s, COLS // s) if layout == "chw" else (ROWS // s, COLS // s, depth)
    assert tuple(emu.stack.shape) == (emu.n,) + shape and emu.stack.dtype.itemsize == 1
    assert emu._L.pk_fstack_depth(emu._h) == depth and emu._L.pk_fstack_scale(emu._h) == s
    assert not got(emu).any()                                            # starts as all zeros
    return Model(emu.n, s, depth, layout, mode)


def check_model(make, dev):
    """Eight configurations on 64 envs: a fill from one random screen, then nine pushes of other random
    screens, three of them with a random fill mask; the whole stack equals the model after every call,
    and the HWC stack is the CHW stack transposed."""
    n = 64
    final = {}
    for s, depth, layout, mode in CONFIGS:
        emu = make(n)
        model = create(emu, s, depth, layout, mode)
        first = random_screens(n, 100)
        emu.stack_push(fill_only=True, screen=dev(first, np.uint8))
        model.push(first, fill_only=True)
        same(emu, model, (s, depth, layout, mode, "fill"))
        rng = np.random.default_rng(7)
        for t in range(9):
            screens = random_screens(n, 101 + t)
            mask = rng.integers(0, 2, n).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8) if t in (2, 5, 8) else None
            emu.stack_push(None if mask is None else dev(mask, np.uint8), screen=dev(screens, np.uint8))
            model.push(screens, mask)
            same(emu, model, (s, depth, layout, mode, t))
        final[(s, depth, layout, mode)] = got(emu).copy()
        emu.close()
    assert np.array_equal(final[(2, 4, "hwc", "mean")], final[(2, 4, "chw", "mean")].transpose(0, 2, 3, 1))
    # plane 0 is the newest and does not depend on the depth
    assert np.array_equal(final[(2, 8, "chw", "mean")][:, :4], final[(2, 4, "chw", "mean")])


def edge_positions(s):
    """(y, x) of the single pixels: the corners, the last column and row of a block, and the first and
    last source pixel of every piece of a row (a CHW piece is 32 source pixels wide at s = 2 and 4)."""
    pos = [(0, 0), (0, COLS - 1), (ROWS - 1, 0), (ROWS - 1, COLS - 1)]
    pos += [(0, s - 1), (s - 1, 0), (s - 1, s - 1), (s, s)]
    pos += [(70, x) for x in range(32, COLS, 32)] + [(71, x - 1) for x in range(32, COLS, 32)]
    pos += [(77, x) for x in (8, 16, 24)]                                # piece boundaries of the HWC pieces
    return pos


def check_edges(make, dev):
    """Both modes at s = 2 and 4, in both layouts: one non-zero pixel per env at the corners, block
    edges and piece boundaries, with the values that sit on the mean's rounding step, and the constant
    screens 0x00, 0x7F, 0x80, 0xFF."""
    n = 64
    for s in (2, 4):
        pos = edge_positions(s)
        values = (0xFF, s * s // 2, s * s // 2 - 1)                      # the mean rounds the last one down to 0
        screens = np.zeros((n, ROWS, COLS), np.uint8)
        cases = [(y, x, v) for v in values for (y, x) in pos]
        consts = (0x00, 0x7F, 0x80, 0xFF)
        assert len(cases) + len(consts) <= n
        for e, (y, x, v) in enumerate(cases):
            screens[e, y, x] = v
        for i, c in enumerate(consts):
            screens[len(cases) + i] = c
        for mode in ("mean", "pick"):
            for layout in ("chw", "hwc"):
                emu = make(n)
                model = create(emu, s, 2, layout, mode)
                emu.stack_push(screen=dev(screens, np.uint8))
                model.push(screens)
                same(emu, model, (s, mode, layout))
                newest = got(emu)[:, 0] if layout == "chw" else got(emu)[..., 0]
                older = got(emu)[:, 1] if layout == "chw" else got(emu)[..., 1]
                assert not older.any()
                for e, (y, x, v) in enumerate(cases):
                    want = np.zeros((ROWS // s, COLS // s), np.uint8)
                    if mode == "mean":
                        want[y // s, x // s] = (v + s * s // 2) // (s * s)
                    elif y % s == 0 and x % s == 0:
                        want[y // s, x // s] = v
                    assert np.array_equal(newest[e], want), (s, mode, layout, y, x, v)
                for i, c in enumerate(consts):
                    assert (newest[len(cases) + i] == c).all(), (s, mode, layout, c)
                emu.close()


def check_reference_frames(make, dev):
    """The 264 reference frames as caller screens of a 320-env handle (the other 56 envs hold frame 0):
    the planes equal the model, and PICK at s = 2 is screen[:, ::2, ::2]."""
    frames = GREY[np.load(FIXTURE)["frames"]]
    k, n = len(frames), 320
    assert frames.shape == (264, ROWS, COLS)
    screens = np.concatenate([frames, np.repeat(frames[:1], n - k, axis=0)])
    sd = dev(screens, np.uint8)
    for s, layout, mode in ((1, "chw", "mean"), (2, "chw", "mean"), (2, "hwc", "pick"), (4, "chw", "mean"), (4, "hwc", "pick")):
        emu = make(n)
        model = create(emu, s, 2, layout, mode)
        emu.stack_push(screen=sd)
        model.push(screens)
        same(emu, model, (s, layout, mode))
        if (s, mode) == (2, "pick"):
            assert np.array_equal(got(emu)[..., 0], screens[:, ::2, ::2])
            assert len(np.unique(got(emu)[:k, :, :, 0].reshape(k, -1), axis=0)) > 100
        emu.close()


def check_fill_push(make, dev):
    """A mask over envs {0, 5, 63}: flags = 0 fills those and pushes the rest; FILL_ONLY leaves every
    other env's bytes as a snapshot taken before has them; at depth 1 push and fill agree."""
    n = 64
    mask = np.zeros(n, np.uint8)
    mask[[0, 5, 63]] = (1, 0x80, 0xFF)
    a, b, c, d = (random_screens(n, 200 + i) for i in range(4))
    for layout in ("chw", "hwc"):
        emu = make(n)
        model = create(emu, 2, 4, layout, "mean")
        emu.stack_push(fill_only=True, screen=dev(a, np.uint8))
        emu.stack_push(screen=dev(b, np.uint8))
        emu.stack_push(dev(mask, np.uint8), screen=dev(c, np.uint8))
        model.push(a, fill_only=True)
        model.push(b)
        model.push(c, mask)
        same(emu, model, layout)
        pc, pb, pa = (plane(x, 2, "mean") for x in (c, b, a))
        chw = got(emu) if layout == "chw" else got(emu).transpose(0, 3, 1, 2)
        for e in range(n):
            want = [pc[e]] * 4 if mask[e] else [pc[e], pb[e], pa[e], pa[e]]
            assert np.array_equal(chw[e], np.stack(want)), (layout, e)
        before = got(emu).copy()
        emu.stack_push(dev(mask, np.uint8), fill_only=True, screen=dev(d, np.uint8))
        model.push(d, mask, fill_only=True)
        same(emu, model, layout)
        after = got(emu)
        keep = mask == 0
        assert np.array_equal(after[keep], before[keep]) and not np.array_equal(after[~keep], before[~keep])
        emu.stack_push(fill_only=True, screen=dev(a, np.uint8))          # FILL_ONLY, no mask: every env
        model.push(a, fill_only=True)
        same(emu, model, layout)
        emu.close()
    one, two = make(n), make(n)
    for emu in (one, two):
        create(emu, 2, 1, "chw", "mean")
        emu.stack_push(screen=dev(a, np.uint8))
    one.stack_push(screen=dev(b, np.uint8))
    two.stack_push(fill_only=True, screen=dev(b, np.uint8))
    assert np.array_equal(got(one), got(two)) and np.array_equal(got(one)[:, 0], plane(b, 2, "mean"))
    one.close()
    two.close()


def check_ranges(make, dev, streams=None):
    """192 envs, stacks filled with random canary bytes: ranges [0, 64) and [64, 192) together equal one
    call (streams = a function (first, second) that runs them on two streams), and a range [64, 100)
    writes those envs only."""
    n = 192
    screens = random_screens(n, 300)
    sd = dev(screens, np.uint8)
    mask = (np.arange(n) % 5 == 0).astype(np.uint8)
    md = dev(mask, np.uint8)
    for s, depth, layout in ((2, 4, "chw"), (2, 4, "hwc"), (4, 3, "chw")):
        emu = make(n)
        model = create(emu, s, depth, layout, "mean")
        canary = np.random.default_rng(301).integers(0, 256, got(emu).shape, dtype=np.uint8)
        emu.stack.copy_(dev(canary, np.uint8))
        model.load(canary)
        emu.stack_push(md, screen=sd, env0=64, count=36)
        model.push(screens, mask, env0=64, count=36)
        same(emu, model, (s, depth, layout))
        after = got(emu)
        assert np.array_equal(after[:64], canary[:64]) and np.array_equal(after[100:], canary[100:])
        assert not np.array_equal(after[64:100], canary[64:100])
        emu.stack.copy_(dev(canary, np.uint8))
        model.load(canary)
        run = streams if streams is not None else (lambda first, second: (first(), second()))
        run(lambda: emu.stack_push(md, screen=sd, env0=0, count=64),
            lambda: emu.stack_push(md, screen=sd, env0=64, count=128))
        model.push(screens, mask)
        same(emu, model, (s, depth, layout))
        emu.close()


def check_screen_source(make, dev):
    """A NULL screen is the handle's own screen after a step; a caller's screen works on a handle
    without PK_F_RENDER, a NULL screen fails there."""
    n = 64
    emu = make(n)
    model = create(emu, 2, 4, "chw", "mean")
    emu.reset()
    emu.step(dev(np.arange(n) % 8, np.uint8))
    own = emu.screen.cpu().numpy().copy()
    assert own.any()
    emu.stack_push()
    model.push(own)
    same(emu, model)
    copy = emu.screen.clone()
    emu.close()
    blind = make(n, render=False)
    model = create(blind, 2, 4, "chw", "mean")
    blind.stack_push(screen=copy)
    model.push(own)
    same(blind, model)
    L, h = blind._L, blind._h
    assert L.pk_fstack_push(h, None, None, 0, 0, n, None) < 0 and L.pk_last_error()
    same(blind, model)
    blind.close()


def check_guards(make, dev):
    """Every bad call is a negative code with a message, and the stack and the handle stay as they were."""
    n = 192
    emu = make(n)
    L, h = emu._L, emu._h
    screens = dev(random_screens(n, 400), np.uint8)
    sp = screens.data_ptr()

    def none():
        return L.pk_fstack_depth(h) == 0 and L.pk_fstack_scale(h) == 0 and not L.pk_fstack_ptr(h) and emu.stack is None

    assert none()
    assert L.pk_fstack_push(h, sp, None, 0, 0, n, None) < 0 and L.pk_last_error()       # no stack
    for scale, depth, layout, mode in ((3, 4, 0, 0), (8, 4, 0, 0), (0, 4, 0, 0), (2, 0, 0, 0), (2, 9, 0, 0), (2, 3, 1, 0),
                                       (2, 5, 1, 0), (2, 4, 2, 0), (2, 4, 0, 2)):
        assert L.pk_fstack_create(h, scale, depth, layout, mode) < 0 and L.pk_last_error(), (scale, depth, layout, mode)
        assert none()
    for kw in ({"scale": 3}, {"scale": 8}, {"depth": 0}, {"depth": 9}, {"depth": 3, "layout": "hwc"}, {"layout": "nhwc"},
               {"mode": "max"}):
        with pytest.raises(ValueError):
            emu.stack_create(**kw)
        assert none()
    model = create(emu, 2, 4, "chw", "mean")
    ptr = L.pk_fstack_ptr(h)
    assert ptr and ptr % 16 == 0
    emu.stack_push(fill_only=True, screen=screens)
    model.push(random_screens(n, 400), fill_only=True)

    def unchanged():
        same(emu, model)
        assert L.pk_fstack_depth(h) == 4 and L.pk_fstack_scale(h) == 2 and L.pk_fstack_ptr(h) == ptr

    for args in ((2, 4, 0, 0), (4, 3, 0, 0), (1, 1, 1, 1)):                             # create twice
        assert L.pk_fstack_create(h, *args) < 0 and L.pk_last_error()
        unchanged()
    other = dev(random_screens(n, 401), np.uint8)
    op = other.data_ptr()
    for mask, flags, env0, count, screen in ((None, 2, 0, n, op), (None, 0x80000000, 0, n, op), (None, 0, 32, 8, op),
                                             (None, 0, 128, 65, op), (None, 0, 192, 1, op), (None, 0, 0, 0, op),
                                             (None, 0, 0, n, op + 4), (None, FILL_ONLY, 0, n, op + 4)):
        assert L.pk_fstack_push(h, screen, mask, flags, env0, count, None) < 0, (flags, env0, count)
        assert L.pk_last_error()
        unchanged()
    assert L.pk_fstack_push(h, op, None, 0, 128, 64, None) == 0                          # the last group is a legal range
    model.push(random_screens(n, 401), env0=128, count=64)
    same(emu, model)
    emu.close()


def check_with_emulator(make, dev):
    """The benchmark ROM from power-on, 12 steps of fixed actions with a push after each: the stack
    equals the model fed with the screens cloned after each step.  On a reward handle with PICK at
    s = 2, plane 0 is channel 0 of the composite observation after a step and after a reset."""
    n, steps = 64, 12
    acts = np.random.default_rng(11).integers(0, 8, (steps, n)).astype(np.uint8)
    emu = make(n)
    model = create(emu, 2, 4, "hwc", "mean")
    emu.reset()
    emu.stack_push(fill_only=True)
    model.push(emu.screen.cpu().numpy(), fill_only=True)
    same(emu, model, "reset")
    seen = []
    for t in range(steps):
        emu.step(dev(acts[t], np.uint8))
        screens = emu.screen.clone().cpu().numpy()
        seen.append(screens)
        emu.stack_push()
        model.push(screens)
        same(emu, model, t)
    assert len(np.unique(np.stack(seen).reshape(steps, -1), axis=0)) > 1          # the frames do change
    emu.close()
    emu = make(n, reward=True, max_episode_steps=ec.MAX_STEPS)
    model = create(emu, 2, 4, "hwc", "pick")
    emu.reset()
    emu.stack_push(fill_only=True)
    assert np.array_equal(got(emu)[..., 0], emu.obs.cpu().numpy()[..., 0])
    for t in range(3):
        emu.step(dev(acts[t], np.uint8))
        emu.stack_push()
        assert np.array_equal(got(emu)[..., 0], emu.obs.cpu().numpy()[..., 0]), t
        assert np.array_equal(got(emu)[..., 0], emu.screen.cpu().numpy()[:, ::2, ::2]), t
    emu.reset()
    emu.stack_push(fill_only=True)
    o = emu.obs.cpu().numpy()[..., 0]
    assert all(np.array_equal(got(emu)[..., k], o) for k in range(4))
    emu.close()


def _order(env):
    return [env.phys(e) for e in range(env.num_envs)]


def _equal_planes(stack, layout):
    """Per env: are all planes of the stack the same?"""
    chw = stack if layout == "chw" else stack.transpose(0, 3, 1, 2)
    return (chw == chw[:, :1]).reshape(len(chw), -1).all(axis=1)


def check_vecenv_step(make_env, dev, layout):
    """make_env(**kw): VecEnv(48, batch_size=24, max_episode_steps=5, ...) on padded 64-env slots.
    step(): the observations have the space's shape and equal the model fed with emu.screen and the
    returned terminals after each step; a finished env returns D equal planes of its reset frame."""
    env = make_env(reward=False, frame_stack=4, stack_layout=layout)
    shape = (4, 72, 80) if layout == "chw" else (72, 80, 4)
    assert env.emu.n == 128 and tuple(env.single_observation_space.shape) == shape
    order = _order(env)
    model = Model(48, 2, 4, layout, "mean")
    obs, _ = env.reset()
    model.push(env.emu.screen.cpu().numpy()[order], fill_only=True)
    assert tuple(obs.shape) == (48,) + shape and np.array_equal(obs.cpu().numpy(), model.view())
    assert _equal_planes(obs.cpu().numpy(), layout).all()
    rng = np.random.default_rng(13)
    finished = mixed = 0
    for t in range(13):
        if t == 2:      # stagger the episodes: the odd envs start over, so later steps finish some envs and not others
            odd = np.zeros(env.emu.n, np.uint8)
            odd[[p for e, p in enumerate(order) if e % 2]] = 1
            env.emu.reset(dev(odd, np.uint8))
        obs, rew, term, trunc, _ = env.step(dev(rng.integers(0, 8, 48), np.uint8))
        done = term.cpu().numpy()
        screens = env.emu.screen.cpu().numpy()[order]
        model.push(screens, done)
        o = obs.cpu().numpy()
        assert o.shape == (48,) + shape and np.array_equal(o, model.view()), t
        if done.any():
            finished += 1
            mixed += not done.all()
            newest = o[done][:, 0] if layout == "chw" else o[done][..., 0]
            assert _equal_planes(o[done], layout).all() and np.array_equal(newest, plane(screens[done], 2, "mean"))
    assert finished >= 3 and mixed >= 2
    assert not _equal_planes(env._logical(env.emu.stack).cpu().numpy(), layout).all()
    obs, _ = env.reset()
    assert _equal_planes(obs.cpu().numpy(), layout).all()
    assert np.array_equal(obs.cpu().numpy()[:, 0] if layout == "chw" else obs.cpu().numpy()[..., 0],
                          plane(env.emu.screen.cpu().numpy()[order], 2, "mean"))
    env.emu.close()


def check_vecenv_pipeline(make_env, dev):
    """recv() / send(): each sub-batch's observation equals the model of its 24 envs."""
    env = make_env(reward=True, frame_stack=4, stack_scale=4, stack_mode="pick")
    order = np.array(_order(env))
    model = Model(48, 4, 4, "chw", "pick")
    env.async_reset()
    model.push(env.emu.screen.cpu().numpy()[order], fill_only=True)
    rng = np.random.default_rng(17)
    finished = 0
    for t in range(16):
        obs, rew, term, trunc, infos, ids, masks = env.recv()
        sl = env.current_envs()
        if t >= 2:      # the sub-batch's last send(): its step, its auto-reset and its push
            done = term.cpu().numpy()
            finished += int(done.sum())
            mask = np.zeros(48, np.uint8)
            mask[sl] = done
            model.push(env.emu.screen.cpu().numpy()[order], mask, env0=sl.start, count=24)
        o = obs.cpu().numpy()
        assert o.shape == (24, 4, 36, 40) and np.array_equal(o, model.view()[sl]), t
        env.send(dev(rng.integers(0, 8, 24), np.uint8))
    assert finished >= 24
    env.emu.close()


def check_vecenv_bank(make_env, dev):
    """resume_from_bank, fork, load_from_bank, archive_explore and load_state refill the envs whose
    machine they replaced, and only those."""
    env = make_env(reward=True, frame_stack=4, bank_slots=2, bank_episodes=True, fork_slots=2, archive_cells=4,
                   max_episode_steps=ec.MAX_STEPS)
    order = _order(env)
    rng = np.random.default_rng(19)

    def step(k=1):
        for _ in range(k):
            env.step(dev(rng.integers(0, 8, 48), np.uint8))

    def stack():
        return env._logical(env.emu.stack).cpu().numpy().copy()

    def refilled(before, envs):
        """The envs hold 4 planes of their current frame, every other env what it held before."""
        after = stack()
        keep = np.ones(48, bool)
        keep[list(envs)] = False
        assert np.array_equal(after[keep], before[keep])
        now = plane(env.emu.screen.cpu().numpy()[order], 2, "mean")
        for e in envs:
            assert all(np.array_equal(after[e, k], now[e]) for k in range(4)), e

    env.reset()
    step(2)
    env.checkpoint_to_bank([3], [0])
    env.save_to_bank([4], [1])                                           # a slot without an episode: a resume rejects it
    step(3)
    before = stack()
    assert not _equal_planes(before, "chw").all()
    env.resume_from_bank([7, 30, 9], [0, 0, 1])
    assert env.emu.bank_rejects() == 1
    refilled(before, [7, 30])
    step(2)
    before = stack()
    env.fork([11, 40], [2, 2])
    refilled(before, [11, 40])
    assert np.array_equal(stack()[11, 0], plane(env.emu.screen.cpu().numpy()[order], 2, "mean")[2])
    step(1)
    before = stack()
    env.load_from_bank([5, 47], [1, 1])
    refilled(before, [5, 47])
    step(1)
    env.archive_update()
    step(1)
    before = stack()
    mask = np.zeros(48, np.uint8)
    mask[[0, 25, 46]] = 1
    drawn = env.archive_explore(dev(mask, np.uint8)).cpu().numpy()
    assert (drawn[[0, 25, 46]] >= 0).all() and (np.delete(drawn, [0, 25, 46]) == -1).all()
    refilled(before, [0, 25, 46])
    step(1)
    before = stack()
    env.load_state(33, env.save_state(2))
    refilled(before, [33])
    env.emu.close()


def check_vecenv_off(make_env, dev):
    """frame_stack=0 returns today's observations: the composite observation, or the screen, of a twin
    that never heard of the keyword; the handle has no stack."""
    for reward, shape in ((True, (48, 72, 80, 4)), (False, (48, 144, 160))):
        env, twin = make_env(reward=reward, frame_stack=0), make_env(reward=reward)
        assert env.emu.stack is None and env.emu._L.pk_fstack_depth(env.emu._h) == 0
        assert tuple(env.single_observation_space.shape) == shape[1:]
        a, b = env.reset()[0], twin.reset()[0]
        assert tuple(a.shape) == shape and np.array_equal(a.cpu().numpy(), b.cpu().numpy())
        rng = np.random.default_rng(23)
        for _ in range(3):
            act = dev(rng.integers(0, 8, 48), np.uint8)
            a, b = env.step(act)[0], twin.step(act)[0]
            buf = env.emu.obs if reward else env.emu.screen
            assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()) and np.array_equal(a.cpu().numpy(), env._logical(buf).cpu().numpy())
        env.emu.close()
        twin.emu.close()


BAD_KEYWORDS = ({"frame_stack": 9}, {"frame_stack": -1}, {"frame_stack": 2.5}, {"frame_stack": 4, "stack_scale": 3},
                {"frame_stack": 4, "stack_scale": 8}, {"frame_stack": 3, "stack_layout": "hwc"},
                {"frame_stack": 4, "stack_layout": "nhwc"}, {"frame_stack": 4, "stack_mode": "max"})
