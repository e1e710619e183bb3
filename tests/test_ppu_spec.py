"""The scanline rasteriser against the documented PPU (tests/ppu_spec.py), on the CPU.

The oracle's render_scanline (oracle/gbcore.c) and the HIP render_line (pk_render.h, here through
the host-simulation build of the unmodified kernel source) were written by one hand and were pinned
only on 264 PyBoy frames that keep LCDC, BGP and WX constant and never tie, clip or crowd objects.
Here the spec is pinned to those frames (the only PyBoy evidence), then the oracle and K2 are
compared with the spec on tests/ppu_cases.py's directed and random states, and every single-rule
change of the spec must be seen by a named directed case (as tests/test_sm83_kat.py does for its
checksums), so a missing directed case shows up as a failure here.
tests/test_k2_frames.py runs the same cases on the gfx950 build."""
import os

import numpy as np
import pytest

from oracle import oracle
from tests import ppu_cases, ppu_spec
from tests.ppu_spec import Rules

GOLD = os.path.join(os.path.dirname(__file__), "golden", "ppu_states.npz")
GREY = np.array([0xFF, 0x99, 0x55, 0x00], np.uint8)


def _diff(names, got, want):
    return [(str(names[i]), int((got[i] != want[i]).sum())) for i in range(len(names)) if not np.array_equal(got[i], want[i])]


def _dummy_rom() -> bytes:
    rom = bytearray(0x8000)
    rom[0x147] = 0x13
    return bytes(rom)


def test_spec_and_oracle_equal_the_264_pyboy_frames():
    z = np.load(GOLD)
    prefix, frames, names = z["prefix"], z["frames"], z["names"]
    assert len(prefix) == 264
    spec = [ppu_spec.render_prefix(p) for p in prefix]
    orc = [oracle.render_from_state(p.tobytes()) for p in prefix]
    assert not _diff(names, spec, frames)
    assert not _diff(names, orc, spec)


def test_case_names_and_shapes():
    cases = ppu_cases.all_cases()
    names = [n for n, _ in cases]
    assert len(set(names)) == len(names)
    assert sum(n.startswith("random_") for n in names) == ppu_cases.N_RANDOM == 160
    assert all(p.shape == (ppu_spec.PREFIX,) and p.dtype == np.uint8 and p[0] == 9 for _, p in cases)
    assert ppu_cases.env_count(len(cases)) % 64 != 0
    assert len(ppu_cases.full_state(cases[0][1])) == ppu_cases.V9


def test_directed_cases_keep_tile_select_equal_to_lcdc4_unless_about_it():
    for name, p in ppu_cases.directed():
        _, _, lcdc, _, _, _, par = ppu_spec.split_prefix(p)
        same = bool((par[:, 4] == ((lcdc >> 4) & 1)).all())
        assert same != name.startswith("tile_select_"), name


def test_random_cases_reach_crowded_lines_ties_and_varying_lines():
    """What the issue asks of the random states, measured: lines with 0 and with more than ten
    objects, equal-X overlaps, both object sizes, every LCDC bit 0..6 in both states, and half the
    states with per-line parameters that change."""
    crowd, ties, varying, bits = 0, 0, 0, np.zeros((7, 2), int)
    for name, p in ppu_cases.random_cases():
        _, oam, lcdc, _, _, _, par = ppu_spec.split_prefix(p)
        o = oam.reshape(40, 4).astype(int)
        h = 16 if lcdc & 4 else 8
        y = np.arange(144)[:, None]
        on = (o[:, 0][None, :] - 16 <= y) & (y < o[:, 0][None, :] - 16 + h)
        per_line = on.sum(axis=1)
        crowd += int(per_line.max() > 10 and per_line.min() == 0)
        ties += int(any(len(set(o[on[l], 1])) < on[l].sum() for l in range(144)))
        varying += int((par != par[0]).any())
        for b in range(7):
            bits[b, (lcdc >> b) & 1] += 1
    assert crowd >= 40 and ties >= 80, (crowd, ties)
    assert 70 <= varying <= 80, varying
    assert bits.min() >= 40, bits


def test_oracle_equals_spec_on_every_case():
    cases = ppu_cases.all_cases()
    want = ppu_cases.expected()
    got = [oracle.render_from_state(p.tobytes()) for _, p in cases]
    bad = _diff([n for n, _ in cases], got, want)
    assert not bad, bad[:10]


def test_both_loaders_honour_the_per_line_tile_select():
    """gb_render_from_state used LCDC.4 for every line while pk_load_env built each line's LCDC from
    the latched byte; the alternating cases differ from their constant twins, and the oracle (here)
    and K2 (the every-case tests) equal the spec on them."""
    cases = dict(ppu_cases.directed())
    for name in ("tile_select_alternates_lcdc4_off", "tile_select_alternates_lcdc4_on"):
        p = cases[name]
        const = p.copy()
        lcdc = int(p[ppu_spec.O_REGS])
        const[ppu_spec.O_SCAN + 4:ppu_spec.O_SCAN + 720:5] = (lcdc >> 4) & 1
        want = ppu_spec.render_prefix(p)
        assert not np.array_equal(want, ppu_spec.render_prefix(const))
        assert np.array_equal(oracle.render_from_state(p.tobytes()), want)


def test_hostsim_k2_equals_spec_on_every_case_in_both_lane_orders():
    from tests.hostsim.sim import SimEmulator
    cases = ppu_cases.all_cases()
    names = [n for n, _ in cases]
    want = GREY[ppu_cases.expected()]
    n = ppu_cases.env_count(len(cases))
    assert n % 64 != 0
    emu = SimEmulator(_dummy_rom(), n, render=True)
    try:
        for place in ppu_cases.placements(len(cases)):
            for i, (_, p) in enumerate(cases):
                emu.load_env(place[i], ppu_cases.full_state(p))
            emu.render_latched()
            scr = emu.screen()
            bad = _diff(names, scr[place], want)
            assert not bad, bad[:10]
    finally:
        emu.close()


# One documented rule broken at a time (a field of ppu_spec.Rules, never a second renderer), and the
# directed cases that must notice.  A change no directed case saw would mean a case is missing.
RULE_CHANGES = [
    ("no 8x16 index mask", dict(obj16_index_mask=0xFF), ["obj16_odd_tiles_flips", "obj16_top_edge", "obj16_limit_14"]),
    ("y-flip over 8 rows in 8x16 mode", dict(yflip_over_height=False), ["obj16_odd_tiles_flips", "obj16_bottom_edge"]),
    ("no x-flip", dict(xflip=False), ["obj8_flips", "obj16_odd_tiles_flips", "obj_left_clip", "obj_right_clip"]),
    ("object limit 11", dict(obj_limit=11), ["obj_limit_12", "obj_limit_14", "obj16_limit_12", "obj16_limit_14", "obj_offscreen_slots"]),
    ("selection by X, not OAM order", dict(select_in_oam_order=False), ["obj_limit_12", "obj_limit_14", "obj16_limit_14", "obj_offscreen_slots"]),
    ("reversed tie order", dict(tie_by_oam_index=False), ["obj_equal_x"]),
    ("left clip off by one", dict(left_edge=1), ["obj_left_clip", "obj_exact_edges"]),
    ("X = 0 objects not counted", dict(offscreen_x_takes_slot=False), ["obj_offscreen_slots"]),
    ("behind-BG test on the colour index", dict(behind_test_on_shade=False),
     ["behind_bg_bgp_e0", "behind_bg_bgp_00", "behind_bg_noise_e0", "behind_over_normal"]),
    ("object colour 0 opaque", dict(obj_colour0_transparent=False), ["obj_colour0_black", "obj_palettes_differ", "obj8_flips"]),
    ("unsigned tile ids with LCDC.4 = 0", dict(signed_tile_ids=False), ["lcdc4_off", "tile_select_alternates_lcdc4_on"]),
    ("window row from y - WY", dict(window_row_is_counter=False), ["wx_band_off_screen", "wy_per_line_crossing", "wx_per_line"]),
    ("counter advanced while WX >= 167", dict(counter_needs_wx_on_screen=False), ["wx_band_off_screen", "wx_per_line"]),
    ("WX - 7 clamped at 0", dict(wx_below_7_shifts=False), ["wx_0", "wx_1", "wx_2", "wx_3", "wx_4", "wx_5", "wx_6"]),
    ("map index not wrapped", dict(map_wraps=False), ["scx_cross_255", "scy_cross_255", "scx_scy_cross_255", "scx_per_line", "scy_per_line"]),
    ("BG off draws BGP's colour-0 shade", dict(bg_off_is_shade0=False), ["bg_off_win_off", "bg_off_win_on"]),
    ("window hidden when LCDC.0 = 0", dict(window_without_bg=False), ["bg_off_win_on", "win_full_screen_bg_off"]),
]


def test_rule_changes_cover_the_required_list():
    assert len(RULE_CHANGES) >= 14
    assert len({tuple(sorted(ch)) for _, ch, _ in RULE_CHANGES}) == len(RULE_CHANGES)
    fields = set(Rules.__dataclass_fields__)
    for _, ch, _ in RULE_CHANGES:
        assert len(ch) == 1 and set(ch) <= fields            # one rule at a time


@pytest.mark.parametrize("label,change,seen_by", RULE_CHANGES, ids=[r[0].replace(" ", "_") for r in RULE_CHANGES])
def test_single_rule_change_is_seen_by_named_directed_cases(label, change, seen_by):
    directed = ppu_cases.directed()
    names = [n for n, _ in directed]
    want = ppu_cases.expected()[:len(directed)]
    rules = Rules(**change)
    assert rules != ppu_spec.DOCUMENTED
    changed = {n for i, (n, p) in enumerate(directed) if not np.array_equal(ppu_spec.render_prefix(p, rules), want[i])}
    assert set(seen_by) <= set(names)
    assert set(seen_by) <= changed, (label, sorted(set(seen_by) - changed))
