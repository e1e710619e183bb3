// pk_render.h — device helpers shared by K1 (pk_step.hip: deferred-line flush before a VRAM/OAM
// write) and K2 (pk_kernels.hip: rasterise the latched lines of the rendered frame).
//
// DMG scanline rasteriser = PyBoy 1.x renderer.scanline + scanline_sprites as the oracle restates
// it (oracle/gbcore.c render_scanline), grey palette FF/99/55/00 of screen.screen_ndarray()
// (pokegym/environment.py:268).  Pinned on the reference's 264 savestate frames.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pk_layout.h"

typedef uint32_t u32;
typedef uint8_t u8;

__device__ __forceinline__ u32 bfe8(u32 v, u32 sh) { return (v >> sh) & 0xFFu; }
__device__ __forceinline__ u32 setb8(u32 v, u32 sh, u32 b) { return (v & ~(0xFFu << sh)) | ((b & 0xFFu) << sh); }

// per-lane view of a lane-interleaved RAM image (pk_layout.h): byte(phys) = g[phys << sh | lane]
struct Mem {
    u8* g;      // the env's sub-block base
    u32 lane;   // lane within the sub-block
    u32 sh;     // interleave shift
};
__device__ __forceinline__ u32 ld_phys(const Mem& m, u32 phys) { return m.g[(phys << m.sh) + m.lane]; }
__device__ __forceinline__ void st_phys(const Mem& m, u32 phys, u32 v) { m.g[(phys << m.sh) + m.lane] = (u8)v; }
// the view of env (interleave shift sh)
__device__ __forceinline__ Mem mem_view(u8* mem, u32 env, u32 sh) {
    Mem m;
    m.g = mem + pk_img_off(env, 0u, sh) - (env & (PK_LANES - 1u) & ((1u << sh) - 1u));
    m.lane = env & (PK_LANES - 1u) & ((1u << sh) - 1u);
    m.sh = sh;
    return m;
}

// grey shade of palette index 0..3 (0xFF 0x99 0x55 0x00)
__device__ __forceinline__ u32 grey(u32 shade) { return (0x005599FFu >> (8u * shade)) & 0xFFu; }

__device__ __forceinline__ u32 bg_tile_addr(u32 lcdc, u32 t) {
    if (lcdc & 0x10u) return t * 16u;
    return (u32)(0x1000 + (int)(int8_t)(u8)t * 16);
}

// one scanline of one lane. lat0 = LCDC | SCX<<8 | SCY<<16 | WX<<24 ; lat1 = WY | BGP<<8 |
// OBP0<<16 | OBP1<<24 ; lw = window line counter after this line's increment. out: 160 grey bytes.
__device__ inline void render_line(const Mem& m, u32 y, u32 lat0, u32 lat1, int lw, u8* out) {
    u32 lcdc = lat0 & 0xFFu;
    int bx = (int)bfe8(lat0, 8), by = (int)bfe8(lat0, 16), wx = (int)bfe8(lat0, 24) - 7;
    int wy = (int)(lat1 & 0xFFu);
    u32 bgp = bfe8(lat1, 8), obp0 = bfe8(lat1, 16), obp1 = bfe8(lat1, 24);
    u32 bgmap = (lcdc & 0x08u) ? 0x1C00u : 0x1800u;
    u32 wmap = (lcdc & 0x40u) ? 0x1C00u : 0x1800u;
    bool win = (lcdc & 0x20u) && wy <= (int)y;
    u8 line[PK_COLS];
    // background / window, one 8-pixel tile row at a time
    int x = 0;
    while (x < (int)PK_COLS) {
        u32 lo, hi, sub;
        int run;
        if (win && wx <= x) {
            int wxx = x - wx;
            u32 t = ld_phys(m, PK_P_VRAM + wmap + (u32)(((lw / 8) * 32) % 0x400) + (u32)((wxx / 8) % 32));
            u32 ta = bg_tile_addr(lcdc, t) + (u32)(lw % 8) * 2u;
            lo = ld_phys(m, PK_P_VRAM + ta);
            hi = ld_phys(m, PK_P_VRAM + ta + 1u);
            sub = (u32)(wxx % 8);
            run = 8 - (int)sub;
        } else if (lcdc & 0x01u) {
            int xx = x + bx;
            u32 t = ld_phys(m, PK_P_VRAM + bgmap + (u32)((((y + (u32)by) / 8u) * 32u) % 0x400u) + (u32)((xx / 8) % 32));
            u32 ta = bg_tile_addr(lcdc, t) + ((y + (u32)by) % 8u) * 2u;
            lo = ld_phys(m, PK_P_VRAM + ta);
            hi = ld_phys(m, PK_P_VRAM + ta + 1u);
            sub = (u32)(xx % 8);
            run = 8 - (int)sub;
            if (win && wx > x && wx < x + run) run = wx - x;  // stop the run where the window starts
        } else {
            line[x] = 0;  // background disabled -> white (shade 0)
            x++;
            continue;
        }
        for (int k = 0; k < run && x < (int)PK_COLS; k++, x++) {
            u32 s = 7u - (sub + (u32)k);
            u32 ci = ((lo >> s) & 1u) | (((hi >> s) & 1u) << 1);
            line[x] = (u8)((bgp >> (2u * ci)) & 3u);
        }
    }
    if (lcdc & 0x02u) {
        int h = (lcdc & 0x04u) ? 16 : 8;
        int sel[10];
        int ns = 0;
        for (int n = 0; n < 40 && ns < 10; n++) {
            int sy = (int)ld_phys(m, PK_P_OAM + (u32)n * 4u) - 16;
            if (sy <= (int)y && (int)y < sy + h) sel[ns++] = n;
        }
        for (int i = 1; i < ns; i++) {
            int k = sel[i], j = i - 1;
            u32 kx = ld_phys(m, PK_P_OAM + (u32)k * 4u + 1u);
            while (j >= 0 && ld_phys(m, PK_P_OAM + (u32)sel[j] * 4u + 1u) > kx) { sel[j + 1] = sel[j]; j--; }
            sel[j + 1] = k;
        }
        u32 bg0 = bgp & 3u;
        for (int i = ns - 1; i >= 0; i--) {
            u32 base = PK_P_OAM + (u32)sel[i] * 4u;
            int sy = (int)ld_phys(m, base) - 16, sx = (int)ld_phys(m, base + 1u) - 8;
            u32 ti = ld_phys(m, base + 2u), at = ld_phys(m, base + 3u);
            if (h == 16) ti &= 0xFEu;
            int dy = (int)y - sy;
            int yy = (at & 0x40u) ? (h - dy - 1) : dy;
            u32 pal = (at & 0x10u) ? obp1 : obp0;
            u32 ta = ti * 16u + (u32)yy * 2u;
            u32 lo = ld_phys(m, PK_P_VRAM + ta), hi = ld_phys(m, PK_P_VRAM + ta + 1u);
            for (int dx = 0; dx < 8; dx++) {
                int px = sx + dx;
                u32 xx = (at & 0x20u) ? (u32)(7 - dx) : (u32)dx;
                u32 s = 7u - xx;
                u32 c = ((lo >> s) & 1u) | (((hi >> s) & 1u) << 1);
                if (px >= 0 && px < (int)PK_COLS && c != 0u) {
                    u32 shade = (pal >> (2u * c)) & 3u;
                    if (at & 0x80u) {
                        if (line[px] == bg0) line[px] = (u8)shade;
                    } else {
                        line[px] = (u8)shade;
                    }
                }
            }
        }
    }
    // grey write, 16 bytes at a time
    for (int q = 0; q < (int)PK_COLS; q += 16) {
        uint4 v;
        u32 w[4];
        for (int j = 0; j < 4; j++) {
            u32 a = 0;
            for (int b = 0; b < 4; b++) a |= grey(line[q + j * 4 + b]) << (8 * b);
            w[j] = a;
        }
        v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
        *reinterpret_cast<uint4*>(out + q) = v;
    }
}

// ---------------------------------------------------------------------------------------------
// K2's rasteriser: the same line as render_line, held in registers.  A line is two bit planes of
// 160 bits (five words each): pixel p is bit p & 31 of word p >> 5, plane 0 the low and plane 1 the
// high bit of its 2-bit value.  Tiles are decoded eight pixels at a time with whole-word operations,
// every array below is indexed by compile-time constants only (the loops are fully unrolled), so
// the line never leaves the VGPRs.
#ifdef __HIPCC__
__device__ __forceinline__ u32 pk_alignbit(u32 hi, u32 lo, u32 sh) { return __builtin_amdgcn_alignbit(hi, lo, sh); }
__device__ __forceinline__ u32 pk_brev32(u32 v) { return __builtin_bitreverse32(v); }
#else
// ({hi, lo} >> (sh & 31))[31:0]
static inline u32 pk_alignbit(u32 hi, u32 lo, u32 sh) { return (u32)((((uint64_t)hi << 32) | lo) >> (sh & 31u)); }
static inline u32 pk_brev32(u32 v) {
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0F0F0F0Fu) | ((v & 0x0F0F0F0Fu) << 4);
    return (v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24);
}
#endif
// bits of a where the mask is set, of b elsewhere (v_bfi_b32)
__device__ __forceinline__ u32 bsel(u32 mask, u32 a, u32 b) { return (a & mask) | (b & ~mask); }
// all ones when bit k of v is set
__device__ __forceinline__ u32 bit_fill(u32 v, u32 k) { return 0u - ((v >> k) & 1u); }

// A lane's view of its image through a base that is the same for the whole wave (the group's) and a
// 32-bit offset, so the loads take the scalar-base form: byte(phys) = gb[lo + (phys << sh)]
struct MemW {
    const u8* gb;   // the group's base (wave-uniform in K2)
    u32 lo;         // the lane's offset inside the group
    u32 sh;         // interleave shift
};
__device__ __forceinline__ u32 ldw(const MemW& m, u32 phys) { return m.gb[m.lo + (phys << m.sh)]; }
// the view of lane l of group gid
__device__ __forceinline__ MemW memw_view(const u8* mem, u32 gid, u32 l, u32 sh) {
    MemW m;
    m.gb = mem + (uint64_t)gid * pk_group_stride(sh);
    m.lo = (l >> sh) * (u32)pk_sub_stride(sh) + (l & ((1u << sh) - 1u));
    m.sh = sh;
    return m;
}

// Row `fine` of 21 neighbouring tiles of one map row (phys address maprow), from tile column c0 on
// and wrapping at 32: the colour-index planes of their 168 pixels.  The 21st tile is read only
// when the caller's fine scroll needs it.  Every address stays inside VRAM whatever the inputs.
__device__ __forceinline__ void tile_planes(const MemW& m, u32 maprow, u32 c0, u32 lcdc, u32 fine, bool last,
                                            u32 (&pl)[6], u32 (&ph)[6]) {
    // signed ids (LCDC.4 = 0): 0x1000 + (int8)t * 16 = ((t ^ 0x80) << 4) + 0x800
    const u32 flip = (lcdc & 0x10u) ? 0u : 0x80u;
    const u32 base = PK_P_VRAM + ((lcdc & 0x10u) ? 0u : 0x800u) + fine * 2u;
    u32 t[21], lo[24], hi[24];
#pragma unroll
    for (u32 k = 0; k < 21u; k++) t[k] = (k < 20u || last) ? ldw(m, maprow + ((c0 + k) & 31u)) : 0u;
#pragma unroll
    for (u32 k = 0; k < 24u; k++) {
        lo[k] = hi[k] = 0u;
        if (k < 20u || (k == 20u && last)) {
            const u32 ta = base + ((t[k] ^ flip) << 4);
            lo[k] = ldw(m, ta);
            hi[k] = ldw(m, ta + 1u);
        }
    }
    // four tiles a word: a tile's leftmost pixel is bit 7 of its bytes, so reverse the bits of the
    // word and put the bytes back in order
#pragma unroll
    for (u32 i = 0; i < 6u; i++) {
        const u32 a = lo[4 * i] | (lo[4 * i + 1] << 8) | (lo[4 * i + 2] << 16) | (lo[4 * i + 3] << 24);
        const u32 b = hi[4 * i] | (hi[4 * i + 1] << 8) | (hi[4 * i + 2] << 16) | (hi[4 * i + 3] << 24);
        pl[i] = __builtin_amdgcn_perm(0u, pk_brev32(a), 0x00010203u);
        ph[i] = __builtin_amdgcn_perm(0u, pk_brev32(b), 0x00010203u);
    }
}

// the most objects a line shows
#define PK_OBJ_LINE 10

// one scanline of one lane, arguments as render_line's; out is 16-byte aligned
__device__ __forceinline__ void render_line_regs(const MemW& m, u32 y, u32 lat0, u32 lat1, int lw, u8* out) {
    const u32 lcdc = lat0 & 0xFFu;
    const u32 bx = bfe8(lat0, 8), by = bfe8(lat0, 16);
    const int wx = (int)bfe8(lat0, 24) - 7, wy = (int)(lat1 & 0xFFu);
    const u32 bgp = bfe8(lat1, 8), obp0 = bfe8(lat1, 16), obp1 = bfe8(lat1, 24);
    // (a window that starts right of the screen shows nothing)
    const bool win = (lcdc & 0x20u) && wy <= (int)y && wx < (int)PK_COLS;
    const bool bgon = (lcdc & 0x01u) != 0u;
    u32 c0[5], c1[5];   // colour indices of the BG / window pixels
#pragma unroll
    for (u32 i = 0; i < 5u; i++) c0[i] = c1[i] = 0u;
    // background: the fine scroll is a funnel shift of the tile stream
    if (bgon && !(win && wx <= 0)) {
        const u32 yy = y + by, fs = bx & 7u;
        u32 pl[6], ph[6];
        tile_planes(m, PK_P_VRAM + ((lcdc & 0x08u) ? 0x1C00u : 0x1800u) + ((yy >> 3) & 31u) * 32u, bx >> 3, lcdc, yy & 7u,
                    fs != 0u, pl, ph);
#pragma unroll
        for (u32 i = 0; i < 5u; i++) {
            c0[i] = pk_alignbit(pl[i + 1], pl[i], fs);
            c1[i] = pk_alignbit(ph[i + 1], ph[i], fs);
        }
    }
    // window: the same stream, its pixel 0 at screen column wx (from -7 on), merged by a mask of
    // the columns from wx on
    u32 wm[5];
#pragma unroll
    for (u32 i = 0; i < 5u; i++) wm[i] = 0u;
    if (win) {
        const u32 lwu = (u32)lw & 0xFFu, nwx = (u32)(-wx), fs = nwx & 7u;   // column x shows window pixel x + nwx
        u32 pl[6], ph[6];
        tile_planes(m, PK_P_VRAM + ((lcdc & 0x40u) ? 0x1C00u : 0x1800u) + ((lwu >> 3) & 31u) * 32u, (u32)((int)nwx >> 3), lcdc,
                    lwu & 7u, fs != 0u, pl, ph);
#pragma unroll
        for (u32 i = 0; i < 5u; i++) {
            int n = wx - (int)(32u * i);   // columns of this word left of the window
            n = n < 0 ? 0 : (n > 32 ? 32 : n);
            wm[i] = (0xFFFFFFFFu << ((u32)n >> 1)) << ((u32)n - ((u32)n >> 1));
            c0[i] = bsel(wm[i], pk_alignbit(pl[i + 1], pl[i], fs), c0[i]);
            c1[i] = bsel(wm[i], pk_alignbit(ph[i + 1], ph[i], fs), c1[i]);
        }
    }
    // BGP on the planes: shade bit b of colour c is bit 2c + b of the palette.  With the BG
    // disabled only the window's pixels keep their shade, the rest is shade 0.
    u32 s0[5], s1[5];
    {
        const u32 p00 = bit_fill(bgp, 0), p01 = bit_fill(bgp, 1), p10 = bit_fill(bgp, 2), p11 = bit_fill(bgp, 3);
        const u32 p20 = bit_fill(bgp, 4), p21 = bit_fill(bgp, 5), p30 = bit_fill(bgp, 6), p31 = bit_fill(bgp, 7);
        const u32 keep = bgon ? 0xFFFFFFFFu : 0u;
#pragma unroll
        for (u32 i = 0; i < 5u; i++) {
            s0[i] = bsel(c1[i], bsel(c0[i], p30, p20), bsel(c0[i], p10, p00)) & (wm[i] | keep);
            s1[i] = bsel(c1[i], bsel(c0[i], p31, p21), bsel(c0[i], p11, p01)) & (wm[i] | keep);
        }
    }
    if (lcdc & 0x02u) {
        // one pass over the OAM: the first ten objects on this line in OAM order, kept sorted by
        // (X, OAM index) descending in registers: key = X << 16 | index << 8 | Y (never 0: Y = 0
        // is on no line), 0 = empty
        const u32 h = (lcdc & 0x04u) ? 16u : 8u;
        u32 K[PK_OBJ_LINE];
#pragma unroll
        for (u32 i = 0; i < PK_OBJ_LINE; i++) K[i] = 0u;
        u32 ns = 0;
#pragma unroll
        for (u32 n0 = 0; n0 < 40u; n0 += 10u) {
            u32 oy[10], ox[10];
#pragma unroll
            for (u32 k = 0; k < 10u; k++) {
                oy[k] = ldw(m, PK_P_OAM + (n0 + k) * 4u);
                ox[k] = ldw(m, PK_P_OAM + (n0 + k) * 4u + 1u);
            }
#pragma unroll
            for (u32 k = 0; k < 10u; k++) {
                if (y + 16u - oy[k] < h && ns < PK_OBJ_LINE) {
                    ns++;
                    u32 key = (ox[k] << 16) | ((n0 + k) << 8) | oy[k];
#pragma unroll
                    for (u32 i = 0; i < PK_OBJ_LINE; i++) {
                        const u32 a = K[i];
                        K[i] = a > key ? a : key;
                        key = a > key ? key : a;
                    }
                }
            }
        }
        // draw from the lowest priority (largest X, then largest index) to the highest
        const u32 b0 = bit_fill(bgp, 0), b1 = bit_fill(bgp, 1);   // the shade of BG colour 0
        while (K[0] != 0u) {
            const u32 key = K[0];
#pragma unroll
            for (u32 i = 0; i + 1u < PK_OBJ_LINE; i++) K[i] = K[i + 1];
            K[PK_OBJ_LINE - 1] = 0u;
            const u32 base = PK_P_OAM + ((key >> 8) & 0xFFu) * 4u;
            u32 ti = ldw(m, base + 2u);
            const u32 at = ldw(m, base + 3u);
            if (h == 16u) ti &= 0xFEu;
            const u32 dy = y + 16u - (key & 0xFFu);
            const u32 yy = (at & 0x40u) ? (h - 1u - dy) : dy;
            const u32 ta = PK_P_VRAM + ti * 16u + yy * 2u;
            const u32 w = ldw(m, ta) | (ldw(m, ta + 1u) << 8);
            // pixel k of the object is bit k: the bytes bit-reversed, or as they are under an X flip
            const u32 r = pk_brev32(w);
            const u32 ol = (at & 0x20u) ? (w & 0xFFu) : (r >> 24), oh = (at & 0x20u) ? (w >> 8) : ((r >> 16) & 0xFFu);
            const u32 pal = (at & 0x10u) ? obp1 : obp0;
            // colour 0 is transparent; the palette on the planes as above
            const u32 om = ol | oh;
            const u32 v0 = bsel(oh, bsel(ol, bit_fill(pal, 6), bit_fill(pal, 4)), ol & bit_fill(pal, 2)) & om;
            const u32 v1 = bsel(oh, bsel(ol, bit_fill(pal, 7), bit_fill(pal, 5)), ol & bit_fill(pal, 3)) & om;
            // the object's eight pixels start at column X - 8: a 32-column word left of the screen
            // takes what is clipped there, the words past the last one what is clipped on the right
            const u32 pos = (key >> 16) + 24u, j0 = pos >> 5, sft = pos & 31u;
            const u32 mlo = om << sft, mhi = (om >> 1) >> (31u - sft);
            const u32 v0lo = v0 << sft, v0hi = (v0 >> 1) >> (31u - sft);
            const u32 v1lo = v1 << sft, v1hi = (v1 >> 1) >> (31u - sft);
            const u32 front = (at & 0x80u) ? 0u : 0xFFFFFFFFu;
#pragma unroll
            for (u32 i = 0; i < 5u; i++) {
                const bool isl = j0 == i + 1u, ish = j0 == i;
                u32 mk = isl ? mlo : (ish ? mhi : 0u);
                // attribute bit 7: only over pixels that show the shade of BG colour 0 now
                mk &= front | ~((s0[i] ^ b0) | (s1[i] ^ b1));
                s0[i] = bsel(mk, isl ? v0lo : v0hi, s0[i]);
                s1[i] = bsel(mk, isl ? v1lo : v1hi, s1[i]);
            }
        }
    }
    // grey bytes, four pixels a word: the pixels' plane bits spread to one a byte select the byte of
    // the palette word FF 99 55 00
#pragma unroll
    for (u32 q = 0; q < PK_COLS / 16u; q++) {
        u32 wv[4];
#pragma unroll
        for (u32 j = 0; j < 4u; j++) {
            const u32 sft = (q & 1u) * 16u + j * 4u;
            const u32 l4 = (s0[q >> 1] >> sft) & 15u, h4 = (s1[q >> 1] >> sft) & 15u;
            const u32 sel = ((l4 * 0x00204081u) & 0x01010101u) | (((h4 * 0x00204081u) & 0x01010101u) << 1);
            wv[j] = __builtin_amdgcn_perm(0u, 0x005599FFu, sel);
        }
        uint4 v;
        v.x = wv[0]; v.y = wv[1]; v.z = wv[2]; v.w = wv[3];
        *reinterpret_cast<uint4*>(out + q * 16u) = v;
    }
}

// host-simulation hooks (design statistics): a flush_lines call (0) and a line it rasterises (1)
#ifndef PK_FLUSH_STAT
#define PK_FLUSH_STAT(rendered) ((void)0)
#endif

// The pending-lines word K1 keeps per lane (St.npend): 0 = no latched line waits for rasterisation,
// else (highest pending line + 1) | lowest pending line << 16 — lines are latched at mode-0 events
// (and in bulk by the HALT skip-ahead), so flush_lines reads only that range's latch flags
__device__ __forceinline__ u32 pend_add(u32 p, u32 lo, u32 hi) {
    const u32 h1 = hi + 1u;
    return p == 0u ? (h1 | (lo << 16)) : ((((p & 0xFFFFu) > h1) ? (p & 0xFFFFu) : h1) | (((p >> 16) < lo ? (p >> 16) : lo) << 16));
}

// rasterise every latched-but-pending line of this lane now (before VRAM/OAM change); pend = the
// lane's pending-lines word (pend_add).  Rare path: kept out of line with by-value arguments so
// the step loop's state stays in VGPRs.
__device__ __noinline__ static void flush_lines(u32* lat, u32 lat_stride, u8* screen, u8* gbase, u32 il, u32 sh, u32 lane,
                                                u32 env, u32 gid, u32 pend) {
    Mem m;
    m.g = gbase;
    m.lane = il;
    m.sh = sh;
    u32* lat0 = lat;
    u32* lat1 = lat + lat_stride;
    u32* lat2 = lat + 2u * lat_stride;
#ifndef PK_FLUSH_FULL
    const u32 ylo = pend >> 16, yend = pend & 0xFFFFu;   // lines [ylo, yend)
#else
    const u32 ylo = 0u, yend = pend ? PK_ROWS : 0u;       // (A/B diagnostic: every line's flag)
#endif
    // the latch flags of the range are read 16 lines at a time (independent loads: one memory
    // round trip per batch instead of one per line)
    for (u32 y0 = ylo; y0 < yend; y0 += 16u) {
        u32 f[16];
#pragma unroll
        for (u32 k = 0; k < 16u; k++) {
            const u32 y = y0 + k < PK_ROWS ? y0 + k : PK_ROWS - 1u;   // (reads past the range: never used)
            f[k] = lat2[(gid * PK_ROWS + y) * PK_LANES + lane];
        }
        for (u32 k = 0; k < 16u && y0 + k < yend; k++) {
            const u32 y = y0 + k, idx = (gid * PK_ROWS + y) * PK_LANES + lane, l2 = f[k];
            if (l2 & 0x100u) {
                render_line(m, y, lat0[idx], lat1[idx], (int)(l2 & 0xFFu) - 1, screen + (size_t)env * PK_SCREEN + y * PK_COLS);
                lat2[idx] = l2 & ~0x100u;
                PK_FLUSH_STAT(1);
            }
        }
    }
    PK_FLUSH_STAT(0);
}
