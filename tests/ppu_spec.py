"""The DMG scanline as the published PPU documentation states it (Pan Docs: "Tile Data", "Tile
Maps", "OAM", "LCD Control", "Scrolling", "Palettes") — TEST INFRASTRUCTURE ONLY.

An independent statement of every pixel of a frame, written from the documentation and not from
oracle/gbcore.c render_scanline or pk_render.h render_line, in the manner of tests/sm83_spec.py.
tests/test_ppu_spec.py compares the oracle and the host-simulated K2 with it, tests/test_k2_frames.py
the gfx950 K2, on the 264 PyBoy frames and on the states of tests/ppu_cases.py.

The model is one latch per line (no mid-scanline effects), DMG only.  Inputs: VRAM (8192 bytes), OAM
(160 bytes), LCDC, BGP, OBP0, OBP1 and 144 x 5 per-line parameters (SCX, SCY, WX, WY, tile-data
select = the line's LCDC.4).  Output: 144 x 160 shade ids 0..3.

Per pixel (x, y):

  layer     The window supplies the pixel when LCDC.5 is set, WY <= y, WX <= 166 and x >= WX - 7;
            its column is x - (WX - 7) and its row is the window line counter: the number of EARLIER
            lines of this frame on which the window was shown (LCDC.5, WY <= line, WX <= 166).
            Otherwise, when LCDC.0 is set, the background supplies it: column (x + SCX) mod 256, row
            (y + SCY) mod 256.  Otherwise no layer does and the pixel is shade 0 (white).
  tile      The 32 x 32 map at 9800 or 9C00 (LCDC.6 for the window, LCDC.3 for the background) gives
            the tile id at (row / 8, column / 8); the tile's 16 bytes sit at 8000 + 16 id when the
            line's tile-data select is 1, else at 9000 + 16 * signed(id); row r of a tile is bytes
            2r (low bit plane) and 2r + 1 (high bit plane), bit 7 the leftmost pixel.
  objects   With LCDC.1 set, the line's objects are the first ten in OAM order with
            Y - 16 <= y < Y - 16 + h (h = 16 when LCDC.2 is set, else 8) — X plays no part in the
            choice, so an object at X = 0 or X >= 168 takes a slot and shows nothing.  An object
            covers x in [X - 8, X - 1]; its tile row is y - (Y - 16), mirrored over all h rows by
            attribute bit 6, its tile column mirrored by bit 5; in 8x16 mode bit 0 of the tile index
            is ignored (rows 8..15 come from the tile index | 1).  Colour 0 is transparent whatever
            the palette maps it to; other colours go through OBP1 (bit 4 set) or OBP0.  Where
            objects overlap, the smaller X has priority, equal X the smaller OAM index.  Attribute
            bits 0..3 mean nothing on DMG.

Four behaviours are PyBoy 1.x's and not the hardware's.  Each is taken from the restatement,
unverified against PyBoy: the tree holds no PyBoy evidence for them (the 264 frames cannot show
them).  DESIGN.md §3 carries the same list.

  1. A behind-BG object pixel (attribute bit 7) is drawn where the pixel's current SHADE equals
     BGP's shade for colour 0 — taken from the restatement, unverified against PyBoy.  (Hardware
     tests the BG/window colour index, so a BGP that maps two colours to one shade differs.)
  2. That test runs against whatever a lower-priority object has already put there, and a behind-BG
     object pixel that fails it does not hide lower-priority objects — taken from the restatement,
     unverified against PyBoy.  (On hardware the highest-priority opaque object pixel alone
     competes with the BG.)  Stated per pixel: with the line's objects that are opaque at x ordered
     c1 (highest priority) .. ck, U(k+1) = the layer's shade and U(i) = shade(ci) if ci is not
     behind-BG or U(i+1) equals BGP's shade for colour 0, else U(i+1); the pixel is U(1).
  3. With LCDC.0 clear the window is still shown when LCDC.5 is set — taken from the restatement,
     unverified against PyBoy.  (On DMG hardware LCDC.0 clear blanks BG and window alike.)  Found
     while reconciling the spec with the oracle; none of the 264 frames has LCDC.0 clear.
  4. The window's WY condition is WY <= y with the line's own latched WY — taken from the
     restatement, unverified against PyBoy.  (Hardware latches WY == LY once per frame.)  Found
     while reconciling; none of the 264 frames changes WY within a frame.

`Rules` holds one switch per documented rule so that tests/test_ppu_spec.py can break one rule at a
time and demand that a directed case notices; the defaults are the rules above.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

ROWS, COLS = 144, 160
PREFIX = 9125                       # v9 state prefix: header, CPU, VRAM, OAM, LCD registers, line params
O_VRAM, O_OAM, O_REGS, O_SCAN = 23, 8215, 8375, 8405


@dataclass(frozen=True)
class Rules:
    obj16_index_mask: int = 0xFE            # 8x16: bit 0 of the tile index ignored
    yflip_over_height: bool = True          # y-flip mirrors over all h rows (False: over 8 rows)
    xflip: bool = True
    obj_limit: int = 10
    select_in_oam_order: bool = True        # False: the ten smallest X are taken
    tie_by_oam_index: bool = True           # False: equal X, the larger OAM index wins
    left_edge: int = 0                      # first screen column an object may draw
    offscreen_x_takes_slot: bool = True     # False: X = 0 objects are not counted
    behind_test_on_shade: bool = True       # False: on the layer's colour index
    obj_colour0_transparent: bool = True
    signed_tile_ids: bool = True            # tile-data select 0: 9000 + signed id
    window_row_is_counter: bool = True      # False: y - WY
    counter_needs_wx_on_screen: bool = True  # False: advances while WX >= 167
    wx_below_7_shifts: bool = True          # False: WX - 7 clamped at 0
    map_wraps: bool = True                  # tile-map row and column taken mod 32
    bg_off_is_shade0: bool = True           # False: BGP's shade for colour 0
    window_without_bg: bool = True          # False: LCDC.0 clear hides the window too


DOCUMENTED = Rules()


def _tile_colour(vram, addr, row, col):
    """colour index 0..3 of pixel (row, col) of the 16-byte tile at VRAM offset addr (arrays)."""
    a = (addr + 2 * row) & 0x1FFF
    lo = vram[a].astype(np.int32)
    hi = vram[(a + 1) & 0x1FFF].astype(np.int32)
    bit = 7 - col
    return ((lo >> bit) & 1) | (((hi >> bit) & 1) << 1)


def _shade(palette, colour):
    return (palette >> (2 * colour)) & 3


def render(vram, oam, lcdc, bgp, obp0, obp1, params, rules: Rules = DOCUMENTED) -> np.ndarray:
    vram = np.asarray(vram, np.uint8).reshape(8192)
    oam = np.asarray(oam, np.uint8).reshape(40, 4).astype(np.int32)
    params = np.asarray(params, np.uint8).reshape(ROWS, 5).astype(np.int32)
    lcdc, bgp, obp0, obp1 = int(lcdc), int(bgp), int(obp0), int(obp1)
    y = np.arange(ROWS, dtype=np.int32)[:, None]
    x = np.arange(COLS, dtype=np.int32)[None, :]
    scx, scy, wx, wy, tsel = (params[:, k][:, None] for k in range(5))
    bg_on, obj_on, obj16 = bool(lcdc & 0x01), bool(lcdc & 0x02), bool(lcdc & 0x04)
    win_on = bool(lcdc & 0x20) and (rules.window_without_bg or bg_on)

    # ---- layer: window, background or none
    win_line = win_on & (wy <= y)                                   # (144, 1)
    shown = win_line & (wx <= 166)
    counted = shown if rules.counter_needs_wx_on_screen else win_line
    counter = np.cumsum(counted, axis=0) - counted                   # earlier lines that showed it
    wleft = wx - 7 if rules.wx_below_7_shifts else np.maximum(wx - 7, 0)
    from_win = shown & (x >= wleft)                                  # (144, 160)
    wrow = counter if rules.window_row_is_counter else y - wy
    row = np.where(from_win, wrow, (y + scy) & 0xFF if rules.map_wraps else y + scy)
    col = np.where(from_win, x - wleft, (x + scx) & 0xFF if rules.map_wraps else x + scx)
    high_map = np.where(from_win, bool(lcdc & 0x40), bool(lcdc & 0x08))
    if rules.map_wraps:
        cell = ((row >> 3) & 31) * 32 + ((col >> 3) & 31)
    else:
        cell = (row >> 3) * 32 + (col >> 3)
    tid = vram[(np.where(high_map, 0x1C00, 0x1800) + cell) & 0x1FFF].astype(np.int32)
    signed = np.where(tid >= 128, tid - 256, tid) if rules.signed_tile_ids else tid
    taddr = np.where(tsel & 1, tid * 16, 0x1000 + signed * 16)
    layer_colour = _tile_colour(vram, taddr, row & 7, col & 7)
    has_layer = from_win | bg_on
    blank = 0 if rules.bg_off_is_shade0 else bgp & 3
    layer_colour = np.where(has_layer, layer_colour, 0)
    under = np.where(has_layer, _shade(bgp, layer_colour), blank)   # U(k+1)
    if not obj_on:
        return under.astype(np.uint8)

    # ---- the line's objects: (144, 40) membership, then rank by priority
    h = 16 if obj16 else 8
    oy, ox, oti, oat = oam[:, 0][None, :], oam[:, 1][None, :], oam[:, 2], oam[:, 3]
    on_line = (oy - 16 <= y) & (y < oy - 16 + h)                     # (144, 40)
    idx = np.arange(40, dtype=np.int32)[None, :]
    if not rules.offscreen_x_takes_slot:
        on_line = on_line & (ox != 0)
    if rules.select_in_oam_order:
        chosen = on_line & (np.cumsum(on_line, axis=1) <= rules.obj_limit)
    else:
        key = np.where(on_line, ox * 64 + idx, 1 << 20)
        chosen = on_line & (np.argsort(np.argsort(key, axis=1, kind="stable"), axis=1) < rules.obj_limit)
    prio = ox * 64 + (idx if rules.tie_by_oam_index else 39 - idx)  # smaller = higher priority
    order = np.argsort(np.where(chosen, prio, 1 << 20), axis=1, kind="stable")   # (144, 40) best first
    nsel = chosen.sum(axis=1)

    # ---- U(i) from the lowest priority up; `under` ends as U(1)
    zero_shade = bgp & 3
    for rank in range(int(nsel.max()) - 1, -1, -1):
        n = order[:, rank]                                           # (144,) OAM index per line
        live = (rank < nsel)[:, None]
        sy, sx = oam[n, 0][:, None] - 16, oam[n, 1][:, None] - 8
        at = oat[n][:, None]
        ti = oti[n][:, None]
        r = y - sy
        if rules.yflip_over_height:
            r = np.where(at & 0x40, h - 1 - r, r)
        else:
            r = np.where(at & 0x40, r ^ 7, r)
        c = x - sx
        covers = live & (c >= 0) & (c < 8) & (x >= rules.left_edge)
        c = np.clip(c, 0, 7)
        if rules.xflip:
            c = np.where(at & 0x20, 7 - c, c)
        if obj16:
            ti = ti & rules.obj16_index_mask
        r = np.clip(r, 0, h - 1)
        colour = _tile_colour(vram, ti * 16, r, c)
        opaque = covers & ((colour != 0) if rules.obj_colour0_transparent else True)
        shade = _shade(np.where(at & 0x10, obp1, obp0), colour)
        behind = (at & 0x80) != 0
        if rules.behind_test_on_shade:
            loses = behind & (under != zero_shade)
        else:
            loses = behind & (layer_colour != 0)
        under = np.where(opaque & ~loses, shade, under)
    return under.astype(np.uint8)


def split_prefix(prefix):
    """(vram, oam, lcdc, bgp, obp0, obp1, params) of a v9 state (prefix)."""
    p = np.frombuffer(bytes(prefix[:PREFIX]), np.uint8) if not isinstance(prefix, np.ndarray) else prefix
    regs = p[O_REGS:O_REGS + 4]
    return (p[O_VRAM:O_VRAM + 8192], p[O_OAM:O_OAM + 160], int(regs[0]), int(regs[1]), int(regs[2]), int(regs[3]),
            p[O_SCAN:O_SCAN + ROWS * 5].reshape(ROWS, 5))


def render_prefix(prefix, rules: Rules = DOCUMENTED) -> np.ndarray:
    return render(*split_prefix(prefix), rules=rules)
