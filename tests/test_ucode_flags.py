"""Properties of the microcode tables (pk_ucode.h) that K1's flag and right-shift units rest on,
checked on the host over every primary entry (256 base, 256 CB-prefixed, 3 pseudo-ops) and every
secondary-op entry: compiled with g++ from the unmodified header, no GPU.

Primary entries (pk_step.hip pk_exec, "flags" and "right-shift unit"):
  * K's flag masks CM (computed), FC (set), FK (kept) and U's FY (loaded from Y) are pairwise disjoint
    and lie in the flag nibble; K's bits 0-3 are clear (the kernel ANDs the computed flags with K
    itself, and bits 0 and 9 of the shifted carries are garbage); FY is alone in its byte of U;
  * FY is 0xF0 exactly for POP AF and DAA, whose Y operand is the two bytes read (m0 | m1 << 8);
  * CW is one bit or none, and no spare-bit field of CI (the H/C shift in bits 0-4, the right unit's
    multiplier) meets it; the H/C shift is 8 for ADD HL,rr and 0 elsewhere;
  * a right-shift-unit entry holds a multiplier / shift pair the kernel's one formula turns into the
    documented result, for every X and shifted-in bit (the formula is restated below), and takes a
    one-byte X;
  * the address unit's ADIR field is 0 or +1 in every entry (pushes are stored low address first).
Secondary entries (the fused-op block): the four in-place masks MASK (b.w), FCONST (b.y), FLIP (b.z),
FK (a.x) lie in bits 20-23 with bits 16-19 of b.w and b.y clear; MASK, FCONST and FK are disjoint; an
entry that writes no flag, and only such an entry, takes F from w1 (S1 byte 2 = 0x02); every entry's
JR test value is nonzero against F & its a.x byte unless it is a JR."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "pokegym_amd", "csrc")

PROG = r"""
#include <stdio.h>
#include <stdint.h>
#include <vector>
#include "pk_ucode.h"
static unsigned bad = 0;
#define CHECK(i, c) do { if (!(c)) { bad++; printf("fail_%d_line_%d 1\n", (int)(i), __LINE__); } } while (0)
static bool disjoint(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    return !(a & b) && !(a & c) && !(a & d) && !(b & c) && !(b & d) && !(c & d);
}
int main() {
    std::vector<uint32_t> t(PK_UC_WORDS);
    pk_build_ucode(t.data());
    unsigned nright = 0, nswap = 0, nfy = 0, nhsh = 0;
    for (int i = 0; i < (int)PK_UC_ENTRIES; i++) {
        const uint32_t* e = t.data() + (size_t)i * PK_UE_WORDS;
        const uint32_t U = e[PK_UE_U], K = e[PK_UE_K], CW = e[PK_UE_CW], CI = e[PK_UE_CI], D = e[PK_UE_D];
        const uint32_t cm = K & 0xFFu, fc = (K >> 8) & 0xFFu, fk = (K >> 16) & 0xFFu, fy = (U >> PK_US_FY) & 0xFFu;
        CHECK(i, disjoint(cm, fc, fk, fy));
        CHECK(i, !((cm | fc | fk | fy) & 0x0Fu));
        CHECK(i, !(cm & 0x40u));                       // N is never computed
        const bool pop = i == 0xF1 || i == 0x27;
        CHECK(i, fy == (pop ? 0xF0u : 0u));
        if (pop) { CHECK(i, e[PK_UE_YE] == PK_E_M16 && e[PK_UE_YR] == PK_PZERO && (e[PK_UE_YC] & 0xFFu) == 0u); nfy++; }
        CHECK(i, (CW & (CW - 1u)) == 0u);              // one bit or none
        CHECK(i, CW == 0u || CW == 1u || CW == (1u << 7) || CW == (1u << 16) || CW == (1u << 20));
        const bool right = (U >> PK_US_RIGHT) & 1u;
        const uint32_t spare = CI & ~((1u << 16) | (1u << 20));
        CHECK(i, !(spare & CW));
        const bool addhl = i == 0x09 || i == 0x19 || i == 0x29 || i == 0x39;
        CHECK(i, (CI & 31u) == (addhl ? PK_CI_HSH : 0u));
        nhsh += addhl;
        const int adir = ((int)(D << (32 - PK_DB_ADIR - 2))) >> 30;
        CHECK(i, adir == 0 || adir == 1);
        const uint32_t rsh = U & 31u;
        if (!right) { CHECK(i, rsh == 0u && (CI & 0xFFFFFFu & ~((1u << 16) | (1u << 20) | 31u)) == 0u); continue; }
        nright++;
        const bool swap = i == 256 + 0x30 + (i & 7) && i >= 256;
        nswap += swap;
        CHECK(i, (CI & 0xFFFFFFu) == (swap ? PK_CI_SMUL : PK_CI_RMUL) && rsh == (swap ? 9u : 6u));
        CHECK(i, !swap || CW == 0u);
        // a one-byte X: one byte selector in one pool, the other pool zero
        const uint32_t xr = e[PK_UE_XR], xe = e[PK_UE_XE];
        CHECK(i, (xr == PK_PZERO && xe == PK_E_M0) || (xe == PK_PZERO && (xr & 0xFFFFFF00u) == 0x0C0C0C00u && (xr & 0xFFu) < 8u));
        // the kernel's formula against the documented result, every X and shifted-in bit
        for (uint32_t X = 0; X < 256; X++)
            for (uint32_t in = 0; in < 2; in++) {
                if (swap && in) continue;
                const uint32_t rs = ((X & 0xFFFFFFu) * (CI & 0xFFFFFFu) + (in << PK_RS_IN)) >> (U & 31u);
                const uint32_t want = swap ? (((X >> 4) | (X << 4)) & 0xFFu) : ((X >> 1) | (in << 7) | ((X & 1u) << 8));
                CHECK(i, (rs & (swap ? 0xFFu : 0x1FFu)) == want);
            }
    }
    printf("nright %u\nnswap %u\nnfy %u\nnhsh %u\n", nright, nswap, nfy, nhsh);
    unsigned nflag = 0, njr = 0;
    for (int op = 0; op < 256; op++) {
        const uint32_t* e = t.data() + PK_UC_U2 + (size_t)op * PK_U2_WORDS;
        const int id = 1000 + op;
        const uint32_t fk = (e[0] >> PK_U2_FPOS) & 0xF0u, fcst = (e[5] >> PK_U2_FPOS) & 0xFFu, flip = (e[6] >> PK_U2_FPOS) & 0xFFu,
                       mask = (e[7] >> PK_U2_FPOS) & 0xFFu;
        const bool jr = op == 0x18 || op == 0x20 || op == 0x28 || op == 0x30 || op == 0x38;
        const bool writes = (mask | fcst) != 0u || (!jr && fk != 0u);
        CHECK(id, !(fcst & 0x0Fu) && !(mask & 0x0Fu));
        CHECK(id, !(flip & ~0x30u) && !(flip & ~mask));
        const uint32_t s1f = (e[3] >> 16) & 0xFFu;
        if ((e[1] & 3u) == 0u) { CHECK(id, !writes); continue; }
        if (jr) {
            njr++;
            CHECK(id, mask == 0u && fcst == 0u && s1f == 0x02u);
            continue;
        }
        CHECK(id, ((e[1] >> PK_U2B_CV) & 0xFFu) == 1u);    // never taken: F's low nibble is 0
        if (!writes) { CHECK(id, s1f == 0x02u); continue; }
        nflag++;
        CHECK(id, s1f == 0x06u);
        CHECK(id, !(mask & fcst) && !(mask & fk) && !(fcst & fk));
        // what the op writes and keeps is the documented split: INC/DEC r keep C, ALU keeps none,
        // CPL keeps Z and C, SCF keeps Z
        const uint32_t keep = (op & 0xC6) == 0x04 ? 0x10u : op == 0x2F ? 0x90u : op == 0x37 ? 0x80u : 0u;
        CHECK(id, fk == keep);
    }
    printf("nflag %u\nnjr %u\nbad %u\n", nflag, njr, bad);
    return 0;
}
"""


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    d = tmp_path_factory.mktemp("ucode_flags")
    src, exe = d / "t.cpp", d / "t"
    src.write_text(PROG)
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", CSRC, "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    return dict(zip(out[0::2], map(int, out[1::2])))


def test_every_entry_holds_the_flag_and_shift_unit_properties(report):
    fails = sorted(k for k in report if k.startswith("fail_"))
    assert report["bad"] == 0 and not fails, fails[:10]


def test_the_cases_were_looked_at(report):
    """The checks above ran on the entries they are about: 4 right shifts/rotates x 8 operands + SWAP x 8
    + RRCA and RRA, POP AF and DAA, four ADD HL,rr, five JR, and the flag-writing secondary ops
    (14 INC/DEC r, 56 ALU A,r, 8 ALU A,n, CPL, SCF)."""
    assert report["nright"] == 4 * 8 + 8 + 2 and report["nswap"] == 8
    assert report["nfy"] == 2 and report["nhsh"] == 4 and report["njr"] == 5
    assert report["nflag"] == 14 + 56 + 8 + 2
