"""Machine states K1 and the oracle are stepped from side by side — TEST INFRASTRUCTURE ONLY.

Every case is (name, n_banks, state, action, expect): a v9 state for the stage ROM
(pokegym_amd/testrom/stage.py) of n_banks banks, the action of every step, and optionally which
loop-skip records the host simulation's trace must (True) or must not (False) hold for the env in
its first frame, e.g. {"copy": True} — decided from the conditions documented above pk_copy_loop,
pk_poll_loop and pk_dec_loop in pk_step.hip.

The LCD block of every state (clock, clock_target, STAT mode, next_stat_mode, LY) is an oracle's,
stopped mid-frame with gb_run_instrs while the stage ROM spins in `boot` (phases()); nothing of it
is written by hand.  All cycle counts of the machine are even and the mode-3 length is 170, so the
distances to the next event that exist are the even ones: "8 and 9 cycles before the event" of the
copy loop's bound are the phases 8 and 10, "60 and 61" are 60 and 62, the dec loop's "15, 16, 17"
are 14, 16, 18.  Everything else is patched onto that state with patch() at the v9 offsets.

Directed cases first, family by family, then seeded random ones from the same generators.
"""
from __future__ import annotations

import functools
import random

import numpy as np

from pokegym_amd.testrom import stage as ST

V9 = 142610
O_CPU, O_VRAM, O_OAM, O_LCD, O_CLOCK, O_TARGET, O_NEXT = 5, 23, 8215, 8375, 8388, 8396, 8404
O_WRAM, O_FEA0, O_IO, O_HRAM, O_FF4C, O_TIMER, O_MBC, O_SRAM = 101285, 109477, 109573, 109649, 109776, 109828, 109836, 109842

# patch() fields -> (offset, bytes)
_F8 = {"a": O_CPU, "f": O_CPU + 1, "b": O_CPU + 2, "c": O_CPU + 3, "d": O_CPU + 4, "e": O_CPU + 5,
       "ime": O_CPU + 12, "halted": O_CPU + 13, "ie": O_CPU + 15, "queued": O_CPU + 16, "if_": O_CPU + 17,
       "lyc": O_LCD + 6, "div": O_TIMER, "tima": O_TIMER + 1, "tma": O_TIMER + 6, "tac": O_TIMER + 7,
       "rombank": O_MBC, "rambank": O_MBC + 1, "ramen": O_MBC + 2}
_F16 = {"hl": O_CPU + 6, "sp": O_CPU + 8, "pc": O_CPU + 10, "divc": O_TIMER + 2, "timac": O_TIMER + 4}
FIELDS = tuple(_F8) + tuple(_F16) + ("stat_en", "ram")


def ram_offset(addr: int, rambank: int = 0) -> int:
    """The v9 offset of a RAM byte (plain bytes only: no IO register with a meaning of its own)."""
    if 0x8000 <= addr < 0xA000:
        return O_VRAM + addr - 0x8000
    if 0xA000 <= addr < 0xC000:
        return O_SRAM + (rambank & 3) * 0x2000 + addr - 0xA000
    if 0xC000 <= addr < 0xFE00:
        return O_WRAM + (addr & 0x1FFF)
    if 0xFE00 <= addr < 0xFEA0:
        return O_OAM + addr - 0xFE00
    if 0xFEA0 <= addr < 0xFF00:
        return O_FEA0 + addr - 0xFEA0
    if addr in (0xFF01, 0xFF02, 0xFF03, 0xFF08, 0xFF09, 0xFF0A) or 0xFF4C <= addr < 0xFF80:
        return O_IO + addr - 0xFF00 if addr < 0xFF4C else O_FF4C + addr - 0xFF4C
    if 0xFF80 <= addr < 0xFFFF:
        return O_HRAM + addr - 0xFF80
    raise ValueError(f"{addr:04X} is not a plain RAM byte")


def patch(state: bytes, **fields) -> bytes:
    """state with the given fields set: a f b c d e hl sp pc ime halted queued ie if_ (CPU), div tima
    divc timac tma tac (timer), rombank rambank ramen (MBC3), stat_en (STAT bits 3-6), lyc, and
    ram = {address: bytes} (SRAM addresses go to the bank given by the patched or present rambank)."""
    s = bytearray(state)
    ram = fields.pop("ram", None)
    for k, v in fields.items():
        if k in _F8:
            s[_F8[k]] = v & 0xFF
        elif k in _F16:
            s[_F16[k]] = v & 0xFF
            s[_F16[k] + 1] = (v >> 8) & 0xFF
        elif k == "stat_en":
            s[O_LCD + 4] = (s[O_LCD + 4] & 0x87) | (v & 0x78)
        else:
            raise KeyError(k)
    for addr, data in (ram or {}).items():
        for i, byte in enumerate(bytes(data)):
            s[ram_offset((addr + i) & 0xFFFF, s[O_MBC + 1])] = byte
    return bytes(s)


def fields_of(state: bytes) -> dict:
    """The fields patch() can set, read back (ram excluded)."""
    out = {k: state[o] for k, o in _F8.items()}
    out.update({k: state[o] | (state[o + 1] << 8) for k, o in _F16.items()})
    out["stat_en"] = state[O_LCD + 4] & 0x78
    return out


def lcd_of(state: bytes) -> dict:
    clock = int.from_bytes(state[O_CLOCK:O_CLOCK + 8], "little")
    target = int.from_bytes(state[O_TARGET:O_TARGET + 8], "little")
    return {"lcdc": state[O_LCD], "mode": state[O_LCD + 4] & 3, "ly": state[O_LCD + 5], "left": target - clock,
            "next": state[O_NEXT]}


# ---- oracle-stopped LCD phases ----
LINES = (0, 1, 70, 142, 143, 144, 152, 153)


@functools.lru_cache(maxsize=None)
def phases(n_banks: int = 2) -> dict:
    """{(mode, ly, cycles left to the next event): state} while the stage ROM spins in `boot`, from
    three start alignments (entry at 0100, 0101 and boot: 20, 16 and 12 cycles + 12 per pass)."""
    from oracle import oracle as O
    rom = ST.stage_rom(n_banks)
    out = {}
    for pc in (0x100, 0x101, rom.sym["boot"]):
        gb = O.GB(rom.rom)
        gb.power_on()
        gb.load_state(patch(gb.save_state(), pc=pc))
        for _ in range(2 * 70224 // 12):
            gb.run_instrs(1)
            ly, left = gb.read(0xFF44), None
            if ly in LINES:
                s = gb.save_state()
                p = lcd_of(s)
                left = p["left"]
                if left <= 34 or 58 <= left <= 62 or left in (100, 200):
                    out.setdefault((p["mode"], ly, left), s)
    return out


def phase(n_banks, mode, ly, left):
    """The oracle-stopped state in `mode` on line `ly` with the cycles to the next event nearest to
    `left` (ties: the larger)."""
    ph = phases(n_banks)
    cand = [k for k in ph if k[0] == mode and k[1] == ly]
    assert cand, (mode, ly)
    k = min(cand, key=lambda k: (abs(k[2] - left), -k[2]))
    return ph[k], k[2]


@functools.lru_cache(maxsize=None)
def lcd_off_state(n_banks: int = 2) -> bytes:
    """An oracle that switched its LCD off with the probe routine (LCDC bit 7 toggled on pass 0)."""
    from oracle import oracle as O
    rom = ST.stage_rom(n_banks)
    base, _ = phase(n_banks, 0, 70, 100)
    gb = O.GB(rom.rom, patch(base, pc=rom.sym["probe"], b=0, d=2, sp=0xDF00))
    for _ in range(400):
        gb.run_instrs(1)
        if not gb.read(0xFF40) & 0x80:
            break
    assert not gb.read(0xFF40) & 0x80
    gb.run_instrs(5)
    return gb.save_state()


def poll_passes_24(left: int, frames: int = 24) -> int:
    """The LY-poll passes K1 skips in one step of `frames` frames (the last one rendered) for a CPU
    that does nothing but poll for a value LY never takes, from `left` cycles before line 145, by the
    rule above pk_poll_loop and lcd_unfold in pk_step.hip, restated: an attempt at clock c (a pass's
    start) skips the passes whose LY read, at c + 32p, comes before the next LY change as K1 knows it
    and which end before the next LCD event, then one pass runs instruction by instruction.  Events,
    in cycles from line 144's start: the loaded state is unfolded, one event per VBlank line; line 0's
    event folds an unrendered frame up to its VBlank event, which folds VBlank up to line 0; LY then
    changes every 456 cycles before the event.  The rendered frame has its three events per line."""
    F = 70224
    ev = [(456 * j, False) for j in range(1, 10)]
    for f in range(frames):                      # line 0 of frame f + 1, then its VBlank event
        t0 = F * f + 4560
        if f + 1 == frames:
            ev += [(t0 + 456 * y + o, False) for y in range(144) for o in (0, 80, 250)]
        else:
            ev.append((t0, True))
        ev.append((F * (f + 1), True))
    c, skipped, i, folded = 456 - left, 0, 0, False
    while True:
        while ev[i][0] <= c:                     # events up to c are processed: the next one is lim
            folded = ev[i][1]
            i += 1
        lim = ev[i][0]
        chg = lim - 456 * ((lim - c - 1) // 456) if folded else lim
        k = min(256, (chg - c - 1) // 32 + 1, (lim - c - 1) // 32)
        skipped += k
        c += 32 * k
        if c + 32 >= F * frames:                 # the step ends inside this pass
            return skipped
        c += 32


def _jp(addr):
    return bytes([0xC3, addr & 0xFF, addr >> 8])


class _Cases(list):
    def add(self, name, n_banks, state, expect=None, action=8):
        assert len(state) == V9
        if any(c[0] == name for c in self):    # a cross may name the same combination twice
            return
        self.append((name, n_banks, state, action, expect))


def _mid(n=2):
    return phase(n, 3, 70, 100)[0]


# ---- families ----
def front_end(C, rng=None, n=0):
    rom = ST.stage_rom(2)
    land = rom.sym["landing"]
    ies = [0, 1, 2, 4, 8, 16, 0x1F, 0xFF]
    ifs = [0, 1, 2, 4, 8, 16, 0x1F, 0xE0, 0xFF]
    base = _mid()
    hcode = {0xFF80: bytes([0x04, 0x0C, 0x14]) + _jp(land)}   # inc b / inc c / inc d / jp landing
    if rng is None:
        # the cross, IE and IF paired so that every value of each meets all eight (ime, halted, queued)
        k = 0
        for ime in (0, 1):
            for halted in (0, 1):
                for queued in (0, 1):
                    for ie in ies:
                        for i_f in (ifs[k % 9], ifs[(k + 4) % 9], ie & 0x1F):
                            k += 1
                            C.add(f"fe-ime{ime}-h{halted}-q{queued}-ie{ie:02X}-if{i_f:02X}", 2,
                                  patch(base, pc=rom.sym["s_halt"] if halted else rom.sym["s_ei_di"] + 2, sp=0xDF80,
                                        ime=ime, halted=halted, queued=queued, ie=ie, if_=i_f))
        # where the dispatch push lands
        pushes = {"e000": 0xE001, "fe00": 0xFE01, "hram-code": 0xFF83, "ff0f": 0xFF11, "ie": 0x0001,
                  "bank": 0x2002, "vram": 0x9802, "sram": 0xA002, "wram": 0xC0F0}
        for where, sp in pushes.items():
            for ime, halted, queued, ie, i_f in ((1, 0, 0, 0x1F, 0x04), (1, 1, 0, 0x01, 0x01), (1, 0, 0, 0xFF, 0x10),
                                                 (0, 1, 0, 0x02, 0x02), (1, 1, 1, 0x04, 0x04), (1, 0, 1, 0x08, 0x1F)):
                if where in ("ie", "bank") and not (ime and bin(ie & i_f & 0x1F).count("1") == 1):
                    continue
                for nb, ramen in ((2, 1), (8, 0)):
                    r8 = ST.stage_rom(nb)
                    b0, _ = phase(nb, 0 if where == "vram" else 2, 70, 30)
                    pc = 0xFF80 if where == "hram-code" else (r8.sym["s_halt"] if halted else r8.sym["s_ei_di"] + 2)
                    C.add(f"fe-push-{where}-{nb}b-ime{ime}-h{halted}-q{queued}-ie{ie:02X}-if{i_f:02X}", nb,
                          patch(b0, pc=pc, sp=sp, ime=ime, halted=halted, queued=queued, ie=ie, if_=i_f, ramen=ramen,
                                rombank=r8.hi, rambank=2, ram=hcode))
        for site in ("s_halt", "s_ei_halt", "s_ei_di", "s_di_halt"):
            for ie, i_f in ((0, 0), (1, 1), (4, 4), (0x1F, 0), (0x10, 0x10)):
                for ime in (0, 1):
                    C.add(f"site-{site}-ime{ime}-ie{ie:02X}-if{i_f:02X}", 2,
                          patch(base, pc=rom.sym[site], sp=0xDF80, ime=ime, ie=ie, if_=i_f))
        for ie, i_f in ((0, 0), (1, 1), (2, 2)):
            C.add(f"site-s_ei_ret-ie{ie:02X}-if{i_f:02X}", 2,
                  patch(base, pc=rom.sym["s_ei_ret"], sp=0xDF80, ie=ie, if_=i_f, ram={0xDF80: bytes([land & 0xFF, land >> 8])}))
        for nb in (2, 8, 64):
            r = ST.stage_rom(nb)
            for ie, i_f in ((0, 0), (1, 0), (4, 4)):
                C.add(f"site-halt-bank-end-{nb}b-ie{ie:02X}-if{i_f:02X}", nb,
                      patch(_mid(nb), pc=0x7FFF, rombank=r.hi, sp=0xDF80, ie=ie, if_=i_f, ime=1,
                            ram={0x8000: bytes([0x0C]) + _jp(land)}))
        return
    for i in range(n):
        b0, _ = phase(2, rng.choice((0, 2, 3)), rng.choice(LINES[:5]), rng.choice((0, 8, 30, 100)))
        halted = rng.randrange(2)
        C.add(f"fe-rand{i}", 2, patch(b0, pc=rom.sym["s_halt"] if halted else rom.sym["s_ei_di"] + 2,
                                      sp=rng.choice((0xDF80, 0xE001, 0xFE01, 0xFF11, 0x9802, 0xC0F0)),
                                      ime=rng.randrange(2), halted=halted, queued=rng.randrange(2),
                                      ie=rng.choice(ies), if_=rng.choice(ifs), tac=rng.choice((0, 5, 6)),
                                      tima=rng.choice((0, 0xFE, 0xFF))))


def halt_skip(C, rng=None, n=0):
    rom = ST.stage_rom(2)
    div = (1024, 16, 64, 256)
    if rng is None:
        for mode, ly, left in ((2, 1, 30), (3, 70, 100), (0, 70, 200), (0, 142, 30), (1, 144, 200)):
            b0, left = phase(2, mode, ly, left)
            for tac in (4, 5, 6, 7):
                for tima in (0x00, 0xFE, 0xFF):
                    d = div[tac & 3]
                    for what, timac in (("before", (0x100 - tima) * d - (left - 4)), ("at", (0x100 - tima) * d - left),
                                        ("after", (0x100 - tima) * d - (left + 4)), ("stale", d + 8)):
                        timac = timac % d if what != "stale" and tima != 0xFF else timac
                        if not 0 <= timac < 0x10000:
                            continue
                        for ie in ((0x04, 0x00)[len(C) & 1],):
                            C.add(f"halt-m{mode}-ly{ly}-tac{tac}-tima{tima:02X}-{what}-ie{ie:02X}", 2,
                                  patch(b0, pc=rom.sym["s_halt"], halted=1, sp=0xDF80, ime=1, ie=ie, tac=tac, tima=tima,
                                        timac=timac, tma=0xF0))
            for en in (0, 0x08, 0x10, 0x20, 0x40):
                for ie in (0, 2, 0x1F):
                    C.add(f"halt-m{mode}-ly{ly}-stat{en:02X}-ie{ie:02X}", 2,
                          patch(b0, pc=rom.sym["s_halt"], halted=1, sp=0xDF80, ime=1, ie=ie, stat_en=en, lyc=(ly + 1) % 154))
        for ie in (0, 1, 4):
            for tac in (0, 5):
                C.add(f"halt-lcdoff-ie{ie:02X}-tac{tac}", 2,
                      patch(lcd_off_state(), pc=rom.sym["s_halt"], halted=1, sp=0xDF80, ime=1, ie=ie, tac=tac, tima=0xFE))
        return
    for i in range(n):
        b0, _ = phase(2, rng.choice((0, 2, 3)), rng.choice(LINES[:5]), rng.choice((0, 8, 30, 100)))
        tac = rng.choice((0, 4, 5, 6, 7))
        C.add(f"halt-rand{i}", 2, patch(b0, pc=rom.sym["s_halt"], halted=1, sp=0xDF80, ime=rng.randrange(2),
                                        ie=rng.choice((0, 1, 2, 4, 0x1F)), tac=tac, tima=rng.choice((0, 0xFE, 0xFF)),
                                        timac=rng.randrange(0, 2 * div[tac & 3], 2), stat_en=rng.choice((0, 0, 0x08, 0x40)),
                                        lyc=rng.choice((0, 71, 143, 144))))


def lcd_observer(C, rng=None, n=0):
    rom = ST.stage_rom(2)
    if rng is None:
        k = 0
        for mode in (2, 3, 0, 1):
            for ly in (0, 1, 142, 143, 144, 152, 153):
                if (mode == 1) != (ly >= 144):
                    continue
                for want in (0, 4, 8):
                    b0, left = phase(2, mode, ly, want)
                    for en in (0, 0x08, 0x10, 0x20, 0x40, 0x78):
                        lyc = (ly, (ly + 1) % 154, 255)[k % 3]
                        reg = (0, 1, 2, 0, 1, 3, 4, 5, 6, 7)[k % 10]
                        k += 1
                        C.add(f"probe-m{mode}-ly{ly}-left{left}-stat{en:02X}-lyc{lyc}-r{reg}", 2,
                              patch(b0, pc=rom.sym["probe"], sp=0xDF80, b=(3, 9, 17)[k % 3], c=(0x40, 0x48, ly, 0x05, 0xFF)[k % 5],
                                    d=reg, stat_en=en, lyc=lyc, ime=k & 1, ie=(0, 3, 0x1F)[k % 3]))
        return
    for i in range(n):
        b0, _ = phase(2, rng.choice((0, 2, 3)), rng.choice(LINES[:5]), rng.choice((0, 4, 8, 30)))
        C.add(f"probe-rand{i}", 2, patch(b0, pc=rom.sym["probe"], sp=0xDF80, b=rng.randrange(24), c=rng.randrange(256),
                                         d=rng.randrange(8), stat_en=rng.choice((0, 0, 0x08, 0x40, 0x78)),
                                         lyc=rng.choice((0, 1, 143, 144, 255)), ime=rng.randrange(2), ie=rng.choice((0, 3, 0x1F)),
                                         tac=rng.choice((0, 0, 5))))


def loops(C, rng=None, n=0):
    rom = ST.stage_rom(2)
    S = rom.sym
    fill = bytes((i * 7 + 3) & 0xFF for i in range(256))
    data = {0xC200: fill, 0xD000: fill, 0x9000: fill, 0xA000: fill}
    if rng is None:
        off = lcd_off_state()
        far = phase(2, 1, 144, 200)[0]     # VBlank line: the next event is a line away
        # copy: counts
        for bc in (0, 1, 2, 0x41, 0x100, 0xFFFF):
            for twin in ("copy_a", "copy_b"):
                C.add(f"copy-{twin}-bc{bc:04X}", 2, patch(off, pc=S[twin], b=bc >> 8, c=bc & 0xFF, hl=0xC200, d=0xD0, e=0x00,
                                                         sp=0xDF80, ram=data), {"copy": bc not in (1,)})
        # region and bank ends, overlap
        for name, hl, de, skip in (("hl-end0", 0xDFFF, 0xC300, None), ("hl-end1", 0xDFFE, 0xC300, True),
                                   ("hl-end65", 0xDFBF, 0xC300, True), ("de-end0", 0xC200, 0xDFFF, None),
                                   ("de-end1", 0xC200, 0xDFFE, True), ("de-end65", 0xC200, 0xDFBF, True),
                                   ("vram-end1", 0xC200, 0x9FFE, True), ("rom-end1", 0x3FFE, 0xC300, True),
                                   ("rom-end65", 0x3FBF, 0xC300, True), ("rom1-end1", 0x7FFE, 0xC300, True),
                                   ("ovl+1", 0xC200, 0xC201, True), ("ovl-1", 0xC201, 0xC200, True), ("same", 0xC200, 0xC200, False),
                                   ("de-echo", 0xC200, 0xE100, False), ("de-oam", 0xC200, 0xFE00, False),
                                   ("de-hram", 0xC200, 0xFF80, False), ("de-io", 0xC200, 0xFF30, False),
                                   ("de-sram", 0xC200, 0xA100, False), ("de-rom", 0xC200, 0x2000, False),
                                   ("hl-sram-off", 0xA000, 0xC300, False), ("hl-io", 0xFF00, 0xC300, False),
                                   ("hl-vram", 0x9000, 0xC300, True), ("hl-echo", 0xE200, 0xC300, False)):
            for nb in (2, 8):
                r = ST.stage_rom(nb)
                C.add(f"copy-{name}-{nb}b", nb, patch(lcd_off_state(nb), pc=r.sym["copy_a"], b=0, c=0x41, hl=hl, d=de >> 8,
                                                     e=de & 0xFF, sp=0xDF80, ram=data, ramen=0, rombank=1 if nb == 2 else 6),
                      None if skip is None or (nb == 8 and name.startswith("rom1")) else {"copy": skip})
        # timing: cycles left to the event
        for want in (8, 10, 60, 62, 100):
            b0, left = phase(2, 1, 144, want)
            C.add(f"copy-left{left}", 2, patch(b0, pc=S["copy_a"], b=0, c=0x41, hl=0xC200, d=0xD0, e=0, sp=0xDF80, ram=data),
                  # a pass (52 cycles) and the next ld a,[hli] (8) must end below the event: skips at once
                  # only from more than 60 cycles away (nearer: stands aside, and skips after the event)
                  {"copy_first": left > 60, **({"copy": True} if left > 60 else {})})
        C.add("copy-timer-on", 2, patch(off, pc=S["copy_a"], b=0, c=0x41, hl=0xC200, d=0xD0, e=0, sp=0xDF80, tac=5, ram=data), {"copy": False})
        C.add("copy-pending-ime0", 2, patch(off, pc=S["copy_a"], b=0, c=0x41, hl=0xC200, d=0xD0, e=0, sp=0xDF80, ie=4, if_=4, ram=data), {"copy": False})
        C.add("copy-queued", 2, patch(off, pc=S["copy_a"], b=0, c=0x41, hl=0xC200, d=0xD0, e=0, sp=0xDF80, queued=1, ram=data),
              {"copy_first": False})
        for ly in (1, 70):
            C.add(f"copy-vram-lines-pending-ly{ly}", 2, patch(phase(2, 0, ly, 200)[0], pc=S["copy_a"], b=1, c=0, hl=0xC200, d=0x98, e=0,
                                                              sp=0xDF80, ram=data),
                  {"copy_first": True})    # a freshly loaded env has no line latched yet
        # placements: switchable bank, bank ends
        C.add("copy-sw-bank", 2, patch(off, pc=S["sw_copy_a"], b=0, c=0x41, hl=0xC200, d=0xD0, e=0, sp=0xDF80, ram=data), {"copy": True})
        C.add("copy-end-exact-bank0", 2, patch(off, pc=0x3FF8, b=0, c=0x41, hl=0xC200, d=0xD0, e=0, sp=0xDF80, ram=data), {"copy": True})
        for nb in (8, 64):
            o8 = lcd_off_state(nb)
            v = {0x8000: _jp(S["landing"]), **data}
            C.add(f"copy-end-past-{nb}b", nb, patch(o8, pc=0x7FF9, rombank=1, b=0, c=0x41, hl=0xC200, d=0xD0, e=0, sp=0xDF80,
                                                    ram={**data, 0x8000: bytes([0xF8]) + _jp(S["landing"])}), {"copy": False})
            C.add(f"copy-end-exact-twin-{nb}b", nb, patch(o8, pc=0x7FF8, rombank=4, b=0, c=0x41, hl=0xC200, d=0xD0, e=0, sp=0xDF80, ram=v),
                  {"copy": True, "small": {"copy": False}})
            C.add(f"copy-end-exact-unstaged-{nb}b", nb, patch(o8, pc=0x7FF8, rombank=6, b=0, c=0x41, hl=0xC200, d=0xD0, e=0, sp=0xDF80, ram=v), {"copy": False})
            C.add(f"copy-sw-unstaged-{nb}b", nb, patch(o8, pc=S["sw_copy_a"], rombank=nb - 1, b=0, c=0x41, hl=0xC200, d=0xD0, e=0, sp=0xDF80, ram=data), {"copy": False})
            C.add(f"poll-end-exact-{nb}b", nb, patch(phase(nb, 0, 70, 200)[0], pc=0x7FFA, rombank=2, sp=0xDF80, ram=v),
                  {"poll": True, "small": {"poll": False}})
            C.add(f"poll-end-past-{nb}b", nb, patch(phase(nb, 0, 70, 200)[0], pc=0x7FFB, rombank=3, sp=0xDF80,
                                                   ram={0x8000: bytes([0xFA]) + _jp(S["landing"])}), {"poll": False})
            C.add(f"poll-sw-unstaged-{nb}b", nb, patch(phase(nb, 0, 70, 200)[0], pc=S["sw_poll_144"], rombank=nb - 1, sp=0xDF80), {"poll": False})
            C.add(f"dec-end-exact-{nb}b", nb, patch(phase(nb, 2, 70, 100)[0], pc=0x7FFD, rombank=5, a=0x28, sp=0xDF80, ram=v),
                  {"dec_first": True})     # the dec loop's code may be anywhere, an unstaged bank included
        C.add("poll-end-exact-bank0-64b", 64, patch(phase(64, 0, 70, 200)[0], pc=0x3FFA, sp=0xDF80), {"poll": True})
        # poll: N against LY, foldable (no STAT source) and not, VBlank, LCD off, near an LY change
        for ly in (0, 1, 70, 142, 143, 144, 152, 153):
            for nn in sorted({x for x in (ly, ly + 1, 144, 153, 0, 200) if x in ST.POLL_NS}):
                for en in (0, 0x40):
                    for want in (30, 200) if en == 0 else (200,):
                        b0, left = phase(2, 1 if ly >= 144 else 2, ly, want)
                        C.add(f"poll-n{nn}-ly{ly}-stat{en:02X}-left{left}", 2, patch(b0, pc=S[f"poll_{nn}"], sp=0xDF80, stat_en=en, lyc=255),
                              # a pass (32 cycles) must end before the event; N == LY leaves the loop
                              {"poll": False, "poll_first": False} if nn == ly else {"poll_first": left > 32})
        for nn in (0, 144, 200):
            C.add(f"poll-n{nn}-lcdoff", 2, patch(off, pc=S[f"poll_{nn}"], sp=0xDF80), {"poll": nn != 0})
        # the exact number of passes skipped over 24 frames, most of them folded (poll_passes_24)
        for want in (200, 100, 30):
            b0, left = phase(2, 1, 144, want)
            C.add(f"poll-count-left{left}", 2, patch(b0, pc=S["poll_200"], sp=0xDF80, stat_en=0, ie=0, lyc=255),
                  {"poll_24": poll_passes_24(left)})
        C.add("poll-sw-bank", 2, patch(far, pc=S["sw_poll_200"], sp=0xDF80), {"poll": True})
        C.add("poll-timer-on", 2, patch(far, pc=S["poll_200"], sp=0xDF80, tac=4), {"poll": False})
        # dec: A x carry, from ROM, HRAM mirror and WRAM, near an event
        dec_ram = {0xFF84: ST.DEC + _jp(S["landing"]), 0xFFA8: ST.DEC + _jp(S["landing"]), 0xC400: ST.DEC + _jp(S["landing"])}
        for a in (0, 1, 2, 0x10, 0x11, 0xFF):
            for f in (0x00, 0x10, 0xF0):
                for where, pc in (("rom", S["dec_rom"]), ("hram", 0xFF84), ("hram-hi", 0xFFA8), ("wram", 0xC400), ("sw", S["sw_dec"])):
                    C.add(f"dec-a{a:02X}-f{f:02X}-{where}", 2, patch(far, pc=pc, a=a, f=f, sp=0xDF80, ram=dec_ram),
                          {"dec": a != 1, "dec_first": a != 1})     # A = 1: the first dec ends the loop
        for want in (14, 16, 18, 30):
            b0, left = phase(2, 2, 70, want)
            for pc in (S["dec_rom"], 0xFF84):
                C.add(f"dec-left{left}-pc{pc:04X}", 2, patch(b0, pc=pc, a=0x28, sp=0xDF80, ram=dec_ram),
                      # a pass (16 cycles) must end before the event
                      {"dec_first": left > 16, **({"dec": True} if left > 16 else {})})
        C.add("dec-timer-on", 2, patch(far, pc=S["dec_rom"], a=0x28, sp=0xDF80, tac=5), {"dec": False})
        C.add("dec-pending", 2, patch(far, pc=0xFF84, a=0x28, sp=0xDF80, ie=8, if_=8, ram=dec_ram), {"dec": False})
        return
    for i in range(n):
        b0 = rng.choice((lcd_off_state(), phase(2, 2, rng.choice(LINES[:5]), rng.choice((8, 30, 60, 200)))[0]))
        kind = rng.choice(("copy_a", "copy_b", "dec_rom", "poll_144", "poll_0", "sw_copy_a", "sw_dec"))
        C.add(f"loop-rand{i}-{kind}", 2, patch(b0, pc=S[kind], a=rng.randrange(256), f=rng.choice((0, 0x10, 0xF0)),
                                               b=rng.choice((0, 0, 1)), c=rng.randrange(256), hl=rng.choice((0xC200, 0x9000, 0x3F00, 0xDFC0, 0x4100)),
                                               d=rng.choice((0xD0, 0xC2, 0x98, 0xDF, 0xFE)), e=rng.choice((0, 0x01, 0xC0)), sp=0xDF80,
                                               tac=rng.choice((0, 0, 0, 5)), ie=rng.choice((0, 0, 4)), if_=rng.choice((0, 4)), ram=data))


# one 2-byte and one 3-byte instruction across each seam (ld b,n from seam-1, ld de,nn from seam-2), then a
# marker and the way out
def seams(C, rng=None, n=0):
    rom = ST.stage_rom(2)
    land = rom.sym["landing"]
    base = _mid()
    mark = bytes([0x3E, 0xA5, 0xEA, 0xE8, 0xC0]) + _jp(land)     # ld a,$A5 / ld [$C0E8],a / jp landing
    if rng is None:
        for nb, bank in ((8, 1), (8, 7)):      # the bank behind the seam: staged, not staged
            for pc in (0x3FFD, 0x3FFE, 0x3FFF):
                C.add(f"seam-3FFF-{nb}b-bank{bank}-pc{pc:04X}", nb, patch(_mid(nb), pc=pc, rombank=bank, sp=0xDF80))
        for pc in (0x7FFD, 0x7FFE, 0x7FFF):
            C.add(f"seam-7FFF-pc{pc:04X}", 64, patch(_mid(64), pc=pc, rombank=ST.SEAM_BANK, sp=0xDF80, ram={0x8000: bytes([0x4F]) + mark}))
        for seam in (0xA000, 0xC000, 0xE000, 0xFE00, 0xFEA0, 0xFF80, 0xFFA0):
            for ramen in ((1, 0) if seam in (0xA000, 0xC000) else (1,)):
                # 3-byte: ld de,nn at seam-2 (operand bytes at seam-1, seam); 2-byte: ld c,n at seam-1 (the landing loop
                # uses A, B, HL and F: what a case computes must end in C, D, E, SP or memory)
                prog = {seam - 2: bytes([0x11, 0x0E, 0x5A]) + mark}
                for pc in (seam - 2, seam - 1):
                    C.add(f"seam-{seam:04X}-pc{pc:04X}-sram{ramen}", 2, patch(base, pc=pc, sp=0xDF80, ramen=ramen, ram=prog))
                # the first instruction overwrites a byte of the second (RAM code after a write: no
                # fusing, no reuse of fetched bytes): ld [hl],a / inc c -> dec c, and ld [hl],a / ld c,n
                for k, second in enumerate((bytes([0x0C]), bytes([0x0E, 0x11]))):
                    p2 = {seam - 1: bytes([0x77]) + second + mark}
                    C.add(f"seam-{seam:04X}-smc{k}-sram{ramen}", 2,
                          patch(base, pc=seam - 1, hl=seam + k, a=0x0D if k == 0 else 0x22, sp=0xDF80, ramen=ramen, ram=p2))
        # the same mid-block, in WRAM, in the HRAM mirror and in HRAM past it: the store rewrites the
        # fusable successor's opcode (inc c -> dec c), turns it into a non-fusable one (-> ld [hl],a is
        # not: -> push bc), or rewrites a fused jr's operand (jr nz,+1 over an inc c -> jr nz,+0)
        for where, at in (("wram", 0xC400), ("mirror", 0xFF84), ("hram", 0xFFA8), ("vram", 0x9000), ("oam", 0xFE10)):
            tail = bytes([0x14]) + mark                                      # inc d, then the way out
            C.add(f"smc-mid-{where}-opcode", 2, patch(base, pc=at, hl=at + 1, a=0x0D, c=0x40, d=0x50, sp=0xDF80,
                                                      ram={at: bytes([0x77, 0x0C]) + tail}))
            C.add(f"smc-mid-{where}-push", 2, patch(base, pc=at, hl=at + 1, a=0xC5, b=0x12, c=0x40, d=0x50, sp=0xDF80,
                                                    ram={at: bytes([0x77, 0x0C]) + tail}))
            C.add(f"smc-mid-{where}-jr-operand", 2, patch(base, pc=at, hl=at + 2, a=0x00, f=0x00, c=0x40, d=0x50, sp=0xDF80,
                                                          ram={at: bytes([0x77, 0x20, 0x01, 0x0C]) + tail}))
            C.add(f"smc-mid-{where}-ld-operand", 2, patch(base, pc=at, hl=at + 2, a=0x99, c=0x40, d=0x50, sp=0xDF80,
                                                          ram={at: bytes([0x77, 0x0E, 0x11]) + tail}))
        # FEFF|FF00: the operand is JOYP; the way on is SB/SC (plain bytes): jr to HRAM
        C.add("seam-FF00", 2, patch(base, pc=0xFEFF, sp=0xDF80, ram={0xFEFF: bytes([0x0E]), 0xFF01: bytes([0x18, 0x7D]), 0xFF80: mark}))
        C.add("seam-FF00-3", 2, patch(base, pc=0xFEFE, sp=0xDF80, ram={0xFEFE: bytes([0x11, 0x0E]), 0xFF01: bytes([0x18, 0x7D]), 0xFF80: mark}))
        # FFFE|FFFF|0000: PC wraps through IE
        for ie in (0x00, 0x04, 0x3E):
            C.add(f"seam-wrap2-ie{ie:02X}", 2, patch(base, pc=0xFFFE, sp=0xDF80, ie=ie, ram={0xFFFE: bytes([0x0E])}))
            C.add(f"seam-wrap3-ie{ie:02X}", 2, patch(base, pc=0xFFFE, sp=0xDF80, ie=ie, ram={0xFFFE: bytes([0x11])}))
            C.add(f"seam-wrap1-ie{ie:02X}", 2, patch(base, pc=0xFFFE, sp=0xDF80, ie=ie, ram={0xFFFE: bytes([0x0C])}))
        return
    legal = [op for op in range(256) if op not in (0xD3, 0xDB, 0xDD, 0xE3, 0xE4, 0xEB, 0xEC, 0xED, 0xF4, 0xFC, 0xFD,
                                                    0x10, 0x76, 0xCB) and op & 0xC7 != 0xC7 and op & 0xE7 != 0x20
             and op not in (0x18, 0xC3, 0xC9, 0xD9, 0xE9, 0xCD) and not (op >> 6 == 3 and op & 7 in (0, 2, 4) and op < 0xE0)]
    length = lambda op: 3 if op in (0x01, 0x11, 0x21, 0x31, 0x08, 0xEA, 0xFA) else 2 if (op & 0xC7 == 0x06 or op & 0xC7 == 0xC6 or op in (0xE0, 0xF0, 0xE8, 0xF8)) else 1  # noqa: E731
    for i in range(n):
        at = rng.choice((0xC400, 0xFF84, 0xFFA0, 0xD7F0))
        code = bytearray()
        for _ in range(24):
            op = rng.choice(legal)
            code.append(op)
            for _ in range(length(op) - 1):
                code.append(rng.choice((0x80, 0xC1, 0xD0, 0xFF, 0x00, 0x41)))
        if i % 4 == 0:                      # every fourth: one illegal opcode (crash-flag parity)
            code[rng.randrange(4, 12)] = rng.choice((0xD3, 0xE4, 0xFD))
        code += _jp(land)
        C.add(f"code-rand{i}-{at:04X}", 2, patch(base, pc=at, sp=0xDF80, hl=0xC0F0, b=0xC1, c=0x81, d=0xD0, e=0x10, a=rng.randrange(256),
                                                 f=rng.choice((0, 0x10, 0x80, 0xF0)), ram={at: bytes(code)}))


def mbc3(C, rng=None, n=0):
    if rng is None:
        sram = {0xA000: b"\x11", 0xBFFF: b"\x22"}
        for nb in (2, 8, 64):
            r = ST.stage_rom(nb)
            base = _mid(nb)
            for v in (0, 1, 0x7F, 0x80, nb, nb - 1, 5, 6):
                for d in (0x20, 0x3F):
                    C.add(f"mbc-{nb}b-bank{v:02X}-d{d:02X}", nb, patch(base, pc=r.sym["mbc"], d=d, e=v, sp=0xDF80, ramen=1, ram=sram))
            for v in (0x0A, 0x1A, 0xFA, 0x0B, 0x00):
                for d, en in ((0x00, 0), (0x1F, 1)):
                    C.add(f"mbc-{nb}b-ramen{v:02X}-d{d:02X}-was{en}", nb, patch(base, pc=r.sym["mbc"], d=d, e=v, sp=0xDF80, ramen=en, ram=sram))
            for v in (0, 1, 2, 3, 4, 8, 0x0C, 0xFF):
                C.add(f"mbc-{nb}b-rambank{v:02X}", nb, patch(base, pc=r.sym["mbc"], d=0x40, e=v, sp=0xDF80, ramen=1,
                                                            ram={0xA000: bytes([0x30 + (v & 3)])}, rambank=v & 3))
            for d in (0x60, 0x7F):
                C.add(f"mbc-{nb}b-latch-d{d:02X}", nb, patch(base, pc=r.sym["mbc"], d=d, e=1, sp=0xDF80, ramen=1, ram=sram))
            fill = bytes((i * 5 + 1) & 0xFF for i in range(0xA0))
            for page in (0x00, 0x3F, 0x40, 0x7F, 0x80, 0xA0, 0xC0, 0xE0, 0xFD, 0xFE, 0xFF):
                for bank, ramen in (((1, 1), (r.hi, 0)) if page in (0x40, 0x7F, 0xA0) else ((1, 1),)):
                    for ph in ((3, 70, 100), (0, 70, 200))[:1 if nb == 64 else 2]:
                        C.add(f"dma-{nb}b-page{page:02X}-bank{bank}-sram{ramen}-m{ph[0]}", nb,
                              patch(phase(nb, *ph)[0], pc=r.sym["dma"], a=page, sp=0xDF80, rombank=bank, ramen=ramen,
                                    ram={0x8000: fill, 0xA000: fill, 0xC000: fill, 0xFD00: fill, 0xFF80: fill[:0x7F]}))
        return
    for i in range(n):
        nb = rng.choice((2, 8, 64))
        r = ST.stage_rom(nb)
        C.add(f"mbc-rand{i}", nb, patch(_mid(nb), pc=r.sym[rng.choice(("mbc", "dma"))], a=rng.randrange(256), d=rng.randrange(0x80),
                                        e=rng.randrange(256), sp=0xDF80, ramen=rng.randrange(2), rombank=rng.randrange(1, nb)))


FAMILIES = (("front-end", front_end, 6), ("halt", halt_skip, 6), ("lcd", lcd_observer, 6), ("loops", loops, 6),
            ("code", seams, 12), ("mbc3", mbc3, 4))
SEED = 0x57A6E


@functools.lru_cache(maxsize=None)
def all_cases() -> tuple:
    """Directed cases of every family, then the seeded random ones."""
    C = _Cases()
    for _, gen, _ in FAMILIES:
        gen(C)
    rng = random.Random(SEED)
    for _, gen, n in FAMILIES:
        gen(C, rng, n)
    names = [c[0] for c in C]
    assert len(set(names)) == len(names), [x for x in names if names.count(x) > 1][:5]
    return tuple(C)


def family_counts() -> dict:
    out = {}
    for name, gen, n in FAMILIES:
        C = _Cases()
        gen(C)
        out[name] = (len(C), n)
    return out


def states_of(cases) -> np.ndarray:
    return np.stack([np.frombuffer(c[2], np.uint8) for c in cases])
