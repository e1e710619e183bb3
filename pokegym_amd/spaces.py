"""Observation/action spaces of the reference env (environment.py:164-167).

gymnasium is not a dependency of the hot path: when it is importable its Box/Discrete are used,
otherwise these minimal stand-ins carry the same attributes (shape, dtype, low, high, n)."""
from __future__ import annotations

import numpy as np

try:  # pragma: no cover - depends on the environment
    from gymnasium.spaces import Box, Discrete  # type: ignore
except Exception:  # noqa: BLE001
    class Box:  # type: ignore[no-redef]
        def __init__(self, low, high, shape, dtype):
            self.low, self.high, self.shape, self.dtype = low, high, tuple(shape), np.dtype(dtype)

        def contains(self, x) -> bool:
            x = np.asarray(x)
            return x.shape == self.shape and x.dtype == self.dtype

        def __repr__(self):
            return f"Box({self.low}, {self.high}, {self.shape}, {self.dtype})"

    class Discrete:  # type: ignore[no-redef]
        def __init__(self, n: int):
            self.n = int(n)
            self.shape = ()
            self.dtype = np.dtype(np.int64)

        def contains(self, x) -> bool:
            return 0 <= int(x) < self.n

        def __repr__(self):
            return f"Discrete({self.n})"


def observation_space():
    return Box(low=0, high=255, shape=(72, 80, 4), dtype=np.uint8)


def action_space():
    return Discrete(8)


def screen_space():
    """The full-resolution grey screen (screen.screen_ndarray()[:, :, 0], environment.py:268) that
    the screen-obs configuration returns instead of the (72, 80, 4) composite."""
    return Box(low=0, high=255, shape=(144, 160), dtype=np.uint8)


def stack_shape(scale: int = 2, depth: int = 4, layout: str = "chw"):
    """Shape of one env's frame stack (pk_fstack_create); ValueError for a geometry it does not take."""
    if scale not in (1, 2, 4):
        raise ValueError("stack scale must be 1, 2 or 4")
    if layout not in ("chw", "hwc"):
        raise ValueError("stack layout must be 'chw' or 'hwc'")
    if isinstance(depth, bool) or not isinstance(depth, (int, np.integer)) or not 1 <= depth <= 8:
        raise ValueError("stack depth must be 1..8")
    if layout == "hwc" and depth not in (1, 2, 4, 8):
        raise ValueError("stack depth must be 1, 2, 4 or 8 with layout 'hwc'")
    h, w = 144 // scale, 160 // scale
    return (int(depth), h, w) if layout == "chw" else (h, w, int(depth))


def stack_space(scale: int = 2, depth: int = 4, layout: str = "chw"):
    """The frame stack VecEnv(frame_stack=depth) returns: depth downscaled frames, newest first —
    (depth, 144 / scale, 160 / scale) for "chw", (144 / scale, 160 / scale, depth) for "hwc"."""
    return Box(low=0, high=255, shape=stack_shape(scale, depth, layout), dtype=np.uint8)


def probe_space(m: int):
    """The feature vector of a RAM probe program of m probes (VecEnv.probe_values): m values below 2**30."""
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 1 <= m <= 64:
        raise ValueError("a probe program has 1..64 probes")
    return Box(low=0, high=(1 << 30) - 1, shape=(int(m),), dtype=np.int32)


def tile_space(planes: int):
    """The tile view (VecEnv.tile_obs): int16 (planes, 18, 20), planes 1 or 2; -1 is "nothing", ids run to
    383 and hashes to 2**15 - 1."""
    if isinstance(planes, bool) or planes not in (1, 2):
        raise ValueError("a tile view has 1 or 2 planes")
    return Box(low=-1, high=(1 << 15) - 1, shape=(int(planes), 18, 20), dtype=np.int16)
