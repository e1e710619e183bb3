"""PPU states that reach the rasteriser's edges — TEST INFRASTRUCTURE ONLY.

A generator of named v9 state prefixes (9125 bytes, as tests/golden/ppu_states.npz holds them; the
renderer reads nothing after the per-line parameters), shared by tests/test_ppu_spec.py (oracle and
host-simulated K2 vs tests/ppu_spec.py) and tests/test_k2_frames.py (the gfx950 K2).  The 264 PyBoy
frames hold LCDC E3, BGP E4, WX 7, WY 0/144, coarse scroll, 8x8 objects that never tie, clip or
exceed eight a line; the directed cases below hold the rest, one documented rule at
a time, and 160 seeded random states mix them.

Every directed case sets each line's tile-data byte to LCDC.4 unless the case is about that byte.
"""
from __future__ import annotations

import numpy as np

from tests.ppu_spec import O_OAM, O_REGS, O_SCAN, O_VRAM, PREFIX, ROWS

V9 = 142610
N_RANDOM = 160
SOLID = 0xF0        # tiles F0..F3: solid colour 0..3 (at 8F00 under either addressing mode)


def base_vram() -> np.ndarray:
    """Tile data: seeded noise (every tile row differs, all four colours everywhere) except the solid
    tiles F0..F3; map 9800 and map 9C00 hold different ids, both on both sides of 128."""
    rng = np.random.default_rng(0x9800)
    v = np.zeros(8192, np.uint8)
    v[:0x1800] = rng.integers(0, 256, 0x1800, dtype=np.uint8)
    for c in range(4):
        t = (SOLID + c) * 16
        v[t:t + 16:2] = 0xFF if c & 1 else 0
        v[t + 1:t + 16:2] = 0xFF if c & 2 else 0
    r, c = np.divmod(np.arange(1024), 32)
    v[0x1800:0x1C00] = (r * 7 + c * 37 + 3) & 0xFF
    v[0x1C00:0x2000] = (r * 45 + c * 11 + 130) & 0xFF
    return v


def solid_columns_vram() -> np.ndarray:
    """Both maps: column c shows the solid tile of colour c & 3 (behind-BG cases)."""
    v = base_vram()
    c = np.arange(1024) % 32
    v[0x1800:0x1C00] = SOLID + (c & 3)
    v[0x1C00:0x2000] = SOLID + ((c + 2) & 3)
    return v


def _lines(v):
    a = np.asarray(v)
    return np.full(ROWS, int(a), np.uint8) if a.ndim == 0 else (a.astype(np.int64) & 0xFF).astype(np.uint8)


def make(lcdc, *, vram=None, oam=(), bgp=0xE4, obp0=0xD2, obp1=0x39, scx=0, scy=0, wx=7, wy=0, td=None) -> np.ndarray:
    """One state prefix.  oam: (Y, X, tile, attribute) in OAM order, or a 160-byte array; scx, scy,
    wx, wy, td: one value or one per line (td defaults to LCDC.4)."""
    p = np.zeros(PREFIX, np.uint8)
    p[0] = 9
    p[O_VRAM:O_VRAM + 8192] = base_vram() if vram is None else vram
    o = np.zeros(160, np.uint8)
    if isinstance(oam, np.ndarray):
        o[:] = oam.reshape(160)
    else:
        assert len(oam) <= 40
        for i, e in enumerate(oam):
            o[4 * i:4 * i + 4] = e
    p[O_OAM:O_OAM + 160] = o
    par = np.stack([_lines(scx), _lines(scy), _lines(wx), _lines(wy),
                    _lines((lcdc >> 4) & 1 if td is None else td)], axis=1)
    p[O_REGS:O_REGS + 11] = [lcdc, bgp, obp0, obp1, 0x80, 0, 0, par[0, 1], par[0, 0], par[0, 3], par[0, 2]]
    p[O_SCAN:O_SCAN + ROWS * 5] = par.reshape(-1)
    return p


def full_state(prefix: np.ndarray) -> bytes:
    s = np.zeros(V9, np.uint8)
    s[:PREFIX] = prefix
    return s.tobytes()


BG_OBJ = 0x93          # LCD on, tile data 8000, BG map 9800, 8x8 objects, BG on, window off
BG_OBJ16 = 0x97
Y = np.arange(ROWS)


def _crowd(n, size16=False):
    """n objects on the same lines: the first ten overlap with X falling as the OAM index rises, the
    11th and later have the smallest X of all (they must not appear); a second row further down
    where the late objects come first in OAM order among other lines' objects."""
    oam = [(60 + (i & 1), 104 - 6 * i, 2 * i + 1, (0x10 if i % 3 == 0 else 0) | (0x20 if i % 4 == 1 else 0)) for i in range(10)]
    oam += [(60, 12 + 9 * (i - 10), 2 * i + 1, 0) for i in range(10, n)]
    oam += [(100, 30 + 9 * k, 41 + 2 * k, 0x40 if size16 else 0) for k in range(5)]
    return oam


def directed() -> list[tuple[str, np.ndarray]]:
    c: list[tuple[str, np.ndarray]] = []

    def add(name, lcdc, **kw):
        c.append((name, make(lcdc, **kw)))

    # ---- objects
    flips = (0x00, 0x40, 0x20, 0x60)
    add("obj16_odd_tiles_flips", BG_OBJ16,
        oam=[(30 + 20 * (k // 4), 20 + 18 * (k % 4) + 70 * (k // 8), 2 * k + 1, flips[k % 4] | (0x10 if k & 4 else 0)) for k in range(16)])
    add("obj8_flips", BG_OBJ,
        oam=[(30 + 12 * (k // 4), 20 + 18 * (k % 4), 2 * k + 1, flips[k % 4]) for k in range(8)])
    add("obj16_top_edge", BG_OBJ16,
        oam=[(yy, 10 + 11 * k, 2 * k + 3, flips[k % 4]) for k, yy in enumerate((1, 2, 5, 8, 9, 12, 15, 16))])
    add("obj16_bottom_edge", BG_OBJ16,
        oam=[(yy, 10 + 11 * k, 2 * k + 3, flips[k % 4]) for k, yy in enumerate((144, 145, 148, 151, 152, 155, 159))])
    add("obj8_top_edge", BG_OBJ,
        oam=[(yy, 10 + 11 * k, k + 3, flips[k % 4]) for k, yy in enumerate((8, 9, 10, 12, 15, 16))])
    add("obj8_bottom_edge", BG_OBJ,
        oam=[(yy, 10 + 11 * k, k + 3, flips[k % 4]) for k, yy in enumerate((152, 153, 156, 159, 160))])
    for nm, l in (("obj8_y0_y160", BG_OBJ), ("obj16_y0_y160", BG_OBJ16)):
        add(nm, l, oam=[(0, 20, 5, 0), (160, 40, 7, 0), (161, 60, 9, 0), (200, 80, 11, 0), (255, 100, 13, 0), (80, 120, 15, 0)])
    add("obj_limit_12", BG_OBJ, oam=_crowd(12))
    add("obj_limit_14", BG_OBJ, oam=_crowd(14))
    add("obj16_limit_12", BG_OBJ16, oam=_crowd(12, True))
    add("obj16_limit_14", BG_OBJ16, oam=_crowd(14, True))
    add("obj_offscreen_slots", BG_OBJ,
        oam=[(70, xx, 2 * k + 1, 0) for k, xx in enumerate((0, 168, 50, 0, 200, 255, 60, 169, 0, 70))]
        + [(70, 90 + 10 * k, 31 + k, 0) for k in range(3)])
    add("obj_equal_x", BG_OBJ,
        oam=[(0, 0, 0, 0)] * 3 + [(50, 60, 5, 0)] + [(0, 0, 0, 0)] * 3 + [(52, 60, 9, 0x10), (90, 100, 11, 0x10), (90, 100, 13, 0)])
    add("obj_overlap_x_orders", BG_OBJ,
        oam=[(50, 40, 5, 0), (51, 44, 7, 0x10), (90, 84, 9, 0), (91, 80, 11, 0x10), (120, 30, 13, 0), (120, 37, 15, 0x10), (120, 33, 17, 0)])
    add("obj_left_clip", BG_OBJ, oam=[(20 + 10 * xx, xx, 2 * xx + 1, 0x20 if xx & 1 else 0) for xx in range(1, 8)])
    add("obj_right_clip", BG_OBJ, oam=[(20 + 10 * (xx - 160), xx, 2 * xx + 1 & 0xFF, 0x20 if xx & 1 else 0) for xx in range(161, 168)])
    add("obj_exact_edges", BG_OBJ, oam=[(40, 8, 3, 0), (60, 160, 5, 0), (80, 8, 7, 0x20), (100, 160, 9, 0x20)])
    behind = [(24 + 20 * (k // 5), 16 + 28 * (k % 5) + (k // 5), 2 * k + 1, 0x80 | (0x10 if k & 1 else 0)) for k in range(25)]
    for bgp in (0xE4, 0xE0, 0x00, 0x1B):
        add(f"behind_bg_bgp_{bgp:02x}", BG_OBJ, vram=solid_columns_vram(), oam=behind, bgp=bgp)
    add("behind_bg_noise_e0", BG_OBJ, oam=behind, bgp=0xE0)
    # a behind-BG object above (smaller X) and below (larger X) a normal one, over each solid colour
    mix = []
    for k in range(4):
        mix += [(30, 20 + 8 * k + 32 * k, 2 * k + 1, 0x80), (32, 23 + 8 * k + 32 * k, 2 * k + 9, 0x10)]
        mix += [(80, 23 + 8 * k + 32 * k, 2 * k + 17, 0x80), (82, 20 + 8 * k + 32 * k, 2 * k + 25, 0x10)]
    add("behind_over_normal", BG_OBJ, vram=solid_columns_vram(), oam=mix)
    add("behind_over_normal_e0", BG_OBJ, vram=solid_columns_vram(), oam=mix, bgp=0xE0)
    pal = [(30 + 14 * (k // 6), 16 + 22 * (k % 6), 2 * k + 1, 0x10 if k & 1 else 0) for k in range(24)]
    add("obj_palettes_differ", BG_OBJ, oam=pal, obp0=0x1B, obp1=0x8D)
    add("obj_colour0_black", BG_OBJ, oam=pal, obp0=0x27, obp1=0x4B)
    add("obj_attr_low_bits", BG_OBJ, oam=[(e[0], e[1], e[2], e[3] | (1 + k % 15)) for k, e in enumerate(pal)], obp0=0x1B, obp1=0x8D)

    # ---- LCDC
    win = dict(wx=87, wy=40)
    add("lcdc4_on", 0xF3, **win)
    add("lcdc4_off", 0xE3, **win)
    for b3 in (0, 1):
        for b6 in (0, 1):
            add(f"maps_bg{b3}_win{b6}", 0xB1 | b3 << 3 | b6 << 6, **win)
    add("bg_off_win_on", 0xF2, oam=pal, bgp=0x1B, **win)
    add("bg_off_win_off", 0xD2, oam=pal, bgp=0x1B, **win)
    add("obj_off_sprites_in_oam", 0xF1, oam=pal, **win)
    add("win_off_wy_wx_on_screen", 0xD3, oam=pal, **win)

    # ---- scroll
    for s in range(1, 8):
        add(f"scx_{s}", BG_OBJ, scx=s)
    add("scx_cross_255", BG_OBJ, scx=200)
    add("scy_cross_255", BG_OBJ, scy=200)
    add("scx_scy_cross_255", 0x9B, scx=251, scy=133)
    add("scx_per_line", BG_OBJ, scx=Y * 7 + 3)
    add("scy_per_line", BG_OBJ, scy=Y * 5 + 1)
    add("scx_scy_per_line", 0x8B, scx=Y * 3 + 250, scy=200 - Y * 2)

    # ---- window
    for w in (0, 1, 2, 3, 4, 5, 6, 7, 8, 15):
        add(f"wx_{w}", 0xF3, wx=w, wy=20, scx=3)
    for w, s in ((10, 3), (45, 5), (100, 7), (12, 1), (161, 6), (9, 2)):
        add(f"wx_{w}_cuts_bg_run_scx_{s}", 0xE3, wx=w, wy=5, scx=s, scy=2)
    add("wx_166", 0xF3, wx=166, wy=10)
    add("wx_167", 0xF3, wx=167, wy=10)
    add("wx_255", 0xF3, wx=255, wy=10)
    for w in (0, 1, 143, 144, 255):
        add(f"wy_{w}", 0xF3, wx=30, wy=w)
    add("wx_band_off_screen", 0xF3, wy=10, wx=np.where((Y >= 40) & (Y < 80), 200, np.where((Y >= 100) & (Y < 110), 167, 47)))
    add("wx_per_line", 0xE3, wy=3, wx=(Y * 13) % 176, scx=5)
    add("wy_per_line_crossing", 0xF3, wx=27,
        wy=np.where(Y < 30, 50, np.where(Y < 70, 20, np.where(Y < 110, 100, np.where(Y & 1, Y + 1, Y - 1)))))
    add("win_full_screen_bg_off", 0xF2, wx=7, wy=0, oam=pal)
    add("tile_select_alternates_lcdc4_off", 0xE3, td=Y & 1, **win)
    add("tile_select_alternates_lcdc4_on", 0xF3, td=(Y >> 1) & 1, **win)
    names = [n for n, _ in c]
    assert len(set(names)) == len(names)
    return c


def _random_oam(rng) -> np.ndarray:
    """Objects clustered on a few lines so that lines hold 0 to about 14; X over 0..175 with ties."""
    o = np.zeros((40, 4), np.uint8)
    centres = rng.integers(0, 176, rng.integers(1, 5))
    xpool = rng.integers(0, 176, 6)
    for i in range(40):
        k = rng.integers(0, 10)
        o[i, 0] = rng.integers(0, 256) if k == 0 else (centres[rng.integers(len(centres))] + rng.integers(-9, 10)) & 0xFF
        o[i, 1] = xpool[rng.integers(6)] if rng.integers(3) == 0 else rng.integers(0, 176)
        o[i, 2] = rng.integers(0, 256)
        o[i, 3] = rng.integers(0, 256)
    return o.reshape(160)


def _random_lines(rng, mode, lo, hi):
    if mode == 0:
        return np.full(ROWS, rng.integers(lo, hi))
    if mode == 1:                                   # piecewise: a few bands
        cuts = np.sort(rng.integers(0, ROWS, rng.integers(1, 5)))
        vals = rng.integers(lo, hi, len(cuts) + 1)
        return vals[np.searchsorted(cuts, Y, side="right")]
    return rng.integers(lo, hi, ROWS)              # every line


def random_cases(n: int = N_RANDOM) -> list[tuple[str, np.ndarray]]:
    out = []
    for k in range(n):
        rng = np.random.default_rng(0xD316 + k)
        lcdc = 0x80 | int(rng.integers(0, 128))
        vram = rng.integers(0, 256, 8192, dtype=np.uint8)
        varying = k & 1
        m = (lambda: int(rng.integers(1, 3))) if varying else (lambda: 0)
        # window on screen most of the time: WX mostly below 167, WY mostly small
        wx = _random_lines(rng, m(), 0, 256 if rng.integers(4) == 0 else 170)
        wy = _random_lines(rng, m(), 0, 256 if rng.integers(4) == 0 else 100)
        td = _random_lines(rng, m(), 0, 2) if varying else (lcdc >> 4) & 1
        out.append((f"random_{k:03d}", make(lcdc, vram=vram, oam=_random_oam(rng), bgp=int(rng.integers(256)),
                                             obp0=int(rng.integers(256)), obp1=int(rng.integers(256)),
                                             scx=_random_lines(rng, m(), 0, 256), scy=_random_lines(rng, m(), 0, 256),
                                             wx=wx, wy=wy, td=td)))
    return out


_cache = None


def all_cases() -> list[tuple[str, np.ndarray]]:
    global _cache
    if _cache is None:
        _cache = directed() + random_cases()
    return _cache


_expected = None


def expected() -> np.ndarray:
    """tests/ppu_spec.py's screen of every case, (n, 144, 160) shade ids, computed once a process."""
    global _expected
    if _expected is None:
        from tests.ppu_spec import render_prefix
        _expected = np.stack([render_prefix(p) for _, p in all_cases()])
        _expected.setflags(write=False)
    return _expected


def env_count(n_cases: int) -> int:
    """Envs of the handle that holds every case: never a multiple of 64 (a partial last group)."""
    return n_cases + 1 if n_cases % 64 == 0 else n_cases


def placements(n_cases: int):
    """The two loads: case i in env i, then case i in env n - 1 - i — neighbouring lanes always hold
    different cases, and every case meets two lanes and two interleave rows."""
    n = env_count(n_cases)
    return [list(range(n_cases)), [n - 1 - i for i in range(n_cases)]]
