"""Tile view (pk_tiles_*): the model of include/pokegym_amd.h in numpy, written from the header's
statement and not from the kernel.

The tile view of an env is the frame the PPU would draw if the registers held at the end of the step
had held for the whole frame, sampled once per 8 x 8 screen cell: uint16 (P, 18, 20), plane 0 the
background / window, plane 1 the objects, 0xFFFF "nothing".  model() states the planes, key_model()
the optional key, from_states() feeds model() with v9 savestates (BatchedEmulator.snapshot).
"""
from __future__ import annotations

import numpy as np

ROWS, COLS = 18, 20
NONE = 0xFFFF
GOLD = np.uint64(0x9E3779B97F4A7C15)
# v9 savestate offsets: VRAM, OAM, and LCDC / SCY, SCX, WY, WX among the LCD registers
_O_VRAM, _O_OAM, _O_LCDC, _O_SCY = 23, 8215, 8375, 8382


def mix(z):
    """splitmix64's finaliser on uint64 arrays (modulo 2**64)."""
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def tile_hash(vram, ids, bits):
    """The hash of the 16 data bytes of tile ids[e, ...] of vram[e] (uint8 (n, 8192)), cut to bits."""
    n = vram.shape[0]
    ids = np.asarray(ids, np.int64)
    flat = ids.reshape(n, -1)
    at = flat[:, :, None] * 16 + np.arange(16)[None, None, :]
    data = np.take_along_axis(vram[:, None, :], at.reshape(n, 1, -1), axis=2).reshape(n, flat.shape[1], 16)
    w = np.ascontiguousarray(data).view("<u4").astype(np.uint64)          # (n, k, 4)
    lo = w[..., 0] | (w[..., 1] << np.uint64(32))
    hi = w[..., 2] | (w[..., 3] << np.uint64(32))
    with np.errstate(over="ignore"):
        h = mix(lo ^ mix(hi + GOLD))
    return (h & np.uint64((1 << bits) - 1)).astype(np.int64).reshape(ids.shape)


def model(vram, oam, lcdc, scy, scx, wy, wx, mode="id", bits=12, obj=True):
    """uint16 (n, P, 18, 20), P = 2 with obj: the tile view of n envs.  vram uint8 (n, 8192), oam uint8
    (n, 160), the five registers one value per env; a single env's arrays (8192,), (160,) and scalars
    give (P, 18, 20).  mode "id" or "hash" (bits 8..15)."""
    if mode not in ("id", "hash"):
        raise ValueError('mode must be "id" or "hash"')
    if mode == "hash" and not 8 <= int(bits) <= 15:
        raise ValueError("bits must be 8..15")
    single = np.ndim(vram) == 1
    vram = np.asarray(vram, np.uint8).reshape(-1, 8192)
    n = vram.shape[0]
    oam = np.asarray(oam, np.uint8).reshape(n, 40, 4).astype(np.int64)
    lcdc, scy, scx, wy, wx = (np.asarray(v, np.int64).reshape(n)[:, None, None] for v in (lcdc, scy, scx, wy, wx))
    out = np.full((n, 2 if obj else 1, ROWS, COLS), NONE, np.int64)
    y = (8 * np.arange(ROWS))[None, :, None]
    x = (8 * np.arange(COLS))[None, None, :]
    on = (lcdc & 0x80) != 0

    # plane 0
    window = ((lcdc & 0x20) != 0) & (y >= wy) & (wx <= 166) & (x + 7 >= wx)
    row = np.where(window, (y - wy) >> 3, ((y + scy) & 255) >> 3)
    col = np.where(window, (x + 7 - wx) >> 3, ((x + scx) & 255) >> 3)
    high = np.where(window, (lcdc & 0x40) != 0, (lcdc & 0x08) != 0)
    at = np.where(high, 0x1C00, 0x1800) + row * 32 + col
    t = np.take_along_axis(vram, at.reshape(n, -1), axis=1).reshape(n, ROWS, COLS).astype(np.int64)
    ids = np.where(((lcdc & 0x10) != 0) | (t >= 128), t, 256 + t)
    shown = np.broadcast_to(on & ((lcdc & 0x01) != 0), ids.shape)
    if mode == "hash":
        ids = tile_hash(vram, ids, int(bits))
    out[:, 0] = np.where(shown, ids, NONE)

    # plane 1: walk the objects from the lowest priority to the highest, so that the last writer wins
    if obj:
        for e in range(n):
            l = int(lcdc[e, 0, 0])
            if not (l & 0x80 and l & 0x02):
                continue
            tall = bool(l & 0x04)
            order = sorted(range(40), key=lambda i: (oam[e, i, 1], i), reverse=True)
            for i in order:
                oy, ox, t_, attr = int(oam[e, i, 0]) - 16, int(oam[e, i, 1]) - 8, int(oam[e, i, 2]), int(oam[e, i, 3])
                r, c = (oy + 4) >> 3, (ox + 4) >> 3
                if tall:
                    halves = [t_ & 0xFE, t_ | 1]
                    if attr & 0x40:
                        halves.reverse()
                    puts = [(r, halves[0]), (r + 1, halves[1])]
                else:
                    puts = [(r, t_)]
                for rr, v in puts:
                    if 0 <= rr < ROWS and 0 <= c < COLS:
                        out[e, 1, rr, c] = v
        if mode == "hash":
            p1 = out[:, 1]
            has = p1 != NONE
            p1[...] = np.where(has, tile_hash(vram, np.where(has, p1, 0), int(bits)), NONE)
    out = out.astype(np.uint16)
    return out[0] if single else out


def key_model(view, salt=None):
    """uint64 (n,): the keys of views uint16 (n, P, 18, 20) (or one view (P, 18, 20): a scalar array);
    salt uint64 (n,) or None."""
    view = np.asarray(view, np.uint16)
    single = view.ndim == 3
    v = view.reshape(1 if single else view.shape[0], -1).astype(np.uint64)
    i = np.arange(1, v.shape[1] + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = np.bitwise_xor.reduce(mix(v + i[None, :] * GOLD), axis=1)
    none = np.uint64(0xFFFFFFFFFFFFFFFF)
    s = np.zeros(v.shape[0], np.uint64) if salt is None else np.asarray(salt).astype(np.uint64).reshape(-1)
    key = mix(s ^ x)
    key = np.where(key == none, none - np.uint64(1), key)
    if salt is not None:
        key = np.where(s == none, none, key)
    return key[0] if single else key


def split_state(state):
    """(vram, oam, lcdc, scy, scx, wy, wx) of v9 savestates: bytes, or a uint8 array (..., >= 8386)."""
    s = np.frombuffer(state, np.uint8) if isinstance(state, (bytes, bytearray)) else np.asarray(state, np.uint8)
    reg = s[..., _O_SCY:_O_SCY + 4].astype(np.int64)
    return (s[..., _O_VRAM:_O_VRAM + 8192], s[..., _O_OAM:_O_OAM + 160], s[..., _O_LCDC].astype(np.int64),
            reg[..., 0], reg[..., 1], reg[..., 2], reg[..., 3])


def from_states(states, mode="id", bits=12, obj=True):
    """model() of v9 savestates: a uint8 array (n, >= 8386), e.g. BatchedEmulator.snapshot_range()."""
    return model(*split_state(states), mode=mode, bits=bits, obj=obj)
