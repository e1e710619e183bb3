// pk_kernels.hip — MI355X (gfx950) kernels around the step kernel (K1 lives in pk_step.hip):
//
//   K2 pk_render_kernel  rasterises the scanlines latched during the last (rendered) frame into
//                        the persistent 144x160 u8 grey screen (replaces PyBoy's renderer +
//                        screen.screen_ndarray(), pokegym/environment.py:268).
//   K5 pk_reset_*        per-env copy of the parsed template savestate (pyboy_binding.py:66-69).
//   gather/scatter       one env's RAM image <-> a dense buffer (pk_snapshot / pk_load_env / peeks).
//   pk_bank_*            savestate bank: listed envs <-> slots of machine state in device memory
//                        (get_random_state / load_*_state / save_state, environment.py:51, :208-227).
//   pk_done_kernel       termination flags when the reward stack is off (environment.py:1612-1613).
//
// Everything here is integer byte work; no MFMA.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/pokegym_amd.h"
#include "pk_layout.h"
#include "pk_render.h"

// ---------------------------------------------------------------------------------------------
// K2: rasterise the latched lines of the rendered frame.  One wave = one (group, scanline),
// lane = env: the 64 lanes read the same VRAM offsets of their interleaved images (coalesced).
// The line is rasterised in registers (pk_render.h render_line_regs; K1's flush_lines keeps the
// byte-array render_line).  With D.on the wave of scanline 0 also writes its envs' termination
// flags, what pk_done_kernel writes, so a rendered step without the reward stack needs no launch
// for them.
__global__ void __launch_bounds__(64) pk_render_kernel(PkStepArgs A, PkDoneArgs D) {
    const u32 y = blockIdx.x % PK_ROWS;
    const u32 gid = A.env0 / PK_LANES + blockIdx.x / PK_ROWS;
    const u32 lane = threadIdx.x;
    const u32 env = gid * PK_LANES + lane;
    if (env >= A.env1) return;
    if (D.on && y == 0u) {
        const u8 done = D.time_reg[env] >= D.max_steps ? 1 : 0;
        if (D.term) D.term[env] = done;
        if (D.trunc) D.trunc[env] = done;
        if (D.rew) D.rew[env] = 0.0;
    }
    const u32 rf = A.regs[PK_R_RFLAGS * A.npad + env];
    u8* out = A.screen + (size_t)env * PK_SCREEN + y * PK_COLS;
    const u32 idx = (gid * PK_ROWS + y) * PK_LANES + lane;
    const u32 l2 = A.lat[2u * A.lat_stride + idx];
    if (rf & 1u) {  // frame ended with the LCD off: blank_screen() (white); its latched lines are dropped
        uint4 wv;
        wv.x = wv.y = wv.z = wv.w = 0xFFFFFFFFu;
        for (u32 q = 0; q < PK_COLS; q += 16) *reinterpret_cast<uint4*>(out + q) = wv;
        if (l2 & 0x100u) A.lat[2u * A.lat_stride + idx] = l2 & ~0x100u;
        return;
    }
    if (!(l2 & 0x100u)) return;
    const MemW m = memw_view(A.mem, gid, lane, A.ilv_sh);
    render_line_regs(m, y, A.lat[idx], A.lat[A.lat_stride + idx], (int)(l2 & 0xFFu) - 1, out);
    A.lat[2u * A.lat_stride + idx] = l2 & ~0x100u;
}

// Re-arm every env's 144 latched lines for K2 (pk_render_latched): the window line counter of each
// line follows from the latched LCDC/WY/WX as K1 derives it at latch time (pyboy renderer: the
// window counter advances on lines where the window is enabled, started and on screen).
__global__ void __launch_bounds__(256) pk_arm_latches_kernel(PkStepArgs A) {
    const u32 env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= A.n) return;
    const u32 gid = env / PK_LANES, lane = env % PK_LANES;
    int lw = -1;
    for (u32 y = 0; y < PK_ROWS; y++) {
        const u32 idx = (gid * PK_ROWS + y) * PK_LANES + lane;
        const u32 l0 = A.lat[idx], l1 = A.lat[A.lat_stride + idx];
        const u32 wy = l1 & 0xFFu, wx = bfe8(l0, 24);
        if ((l0 & 0x20u) && wy <= y && (int)wx - 7 < (int)PK_COLS) lw += 1;
        A.lat[2u * A.lat_stride + idx] = (u32)(lw + 1) | 0x100u;
    }
    A.regs[PK_R_RFLAGS * A.npad + env] &= ~1u;
}

// ---------------------------------------------------------------------------------------------
// K5: reset selected envs from the template (regs + RAM image + screen + line latches).


// The reset kernels work on a device-built list of the envs to reset (pk_list_kernel: ids of the
// masked envs, count in device memory), so a step where few or no envs finish costs a few
// near-empty launches instead of a scan of every env's 49.7 KB image — and no host sync.
__global__ void __launch_bounds__(256) pk_list_kernel(const u8* mask, u32 env0, u32 env1, u32* cnt, u32* ids) {
    const u32 e = env0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= env1 || (mask && !mask[e])) return;
    ids[atomicAdd(cnt, 1u)] = e;
}

// template RAM image -> listed envs: thread = env (list order, so a wave's stores to one image
// row land in one 64-byte line when its envs share a group), block = a strided set of rows
__global__ void __launch_bounds__(256) pk_reset_mem_kernel(PkResetArgs A) {
    const u32 cnt = *A.cnt;
    for (u32 k = threadIdx.x; k < cnt; k += blockDim.x) {
        const u32 env = A.ids[k];
        const Mem m = mem_view(A.mem, env, A.ilv_sh);
        for (u32 p = blockIdx.x; p < PK_PHYS; p += gridDim.x) st_phys(m, p, A.tmpl_mem[p]);
    }
}

__global__ void __launch_bounds__(256) pk_reset_regs_kernel(PkResetArgs A) {
    const u32 cnt = *A.cnt;
    for (u32 k = blockIdx.x * blockDim.x + threadIdx.x; k < cnt; k += gridDim.x * blockDim.x) {
        const u32 env = A.ids[k];
        for (u32 f = 0; f < PK_NREGS; f++) A.regs[f * A.npad + env] = A.tmpl_regs[f];
        const u32 gid = env / PK_LANES, lane = env % PK_LANES;
        for (u32 j = 0; j < 3u; j++)
            for (u32 y = 0; y < PK_ROWS; y++)
                A.lat[j * A.lat_stride + (gid * PK_ROWS + y) * PK_LANES + lane] = A.tmpl_lat[j * PK_ROWS + y];
        const uint4* s = reinterpret_cast<const uint4*>(A.tmpl_screen);
        uint4* d = reinterpret_cast<uint4*>(A.screen + (size_t)env * PK_SCREEN);
        for (u32 q = 0; q < PK_SCREEN / 16u; q++) d[q] = s[q];
    }
}

// gather one env's RAM image into a compact buffer (for pk_snapshot / pk_peek)
__global__ void pk_gather_env_kernel(const u8* mem, u32 env, u32 sh, u8* out) {
    const Mem m = mem_view(const_cast<u8*>(mem), env, sh);
    for (u32 p = blockIdx.x * blockDim.x + threadIdx.x; p < PK_PHYS; p += gridDim.x * blockDim.x)
        out[p] = ld_phys(m, p);
}

// gather envs [env0, env0 + count) into out[count][PK_PHYS] (bulk snapshots): one thread per
// (phys row, env) with env fastest, so each wave reads consecutive interleaved bytes
__global__ void __launch_bounds__(256) pk_gather_range_kernel(const u8* mem, u32 env0, u32 count, u32 sh, u8* out) {
    const size_t total = (size_t)count * PK_PHYS;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const u32 k = (u32)(t % count), p = (u32)(t / count);
        const u32 env = env0 + k;
        out[(size_t)k * PK_PHYS + p] = mem[pk_img_off(env, p, sh)];
    }
}

__global__ void pk_scatter_env_kernel(u8* mem, u32 env, u32 sh, const u8* in) {
    const Mem m = mem_view(mem, env, sh);
    for (u32 p = blockIdx.x * blockDim.x + threadIdx.x; p < PK_PHYS; p += gridDim.x * blockDim.x)
        st_phys(m, p, in[p]);
}

// ---------------------------------------------------------------------------------------------
// host-side launchers (called by the C ABI in pk_capi.cpp)
// d.on: also write the range's termination flags (pk_launch_done's work)
hipError_t pk_launch_render_done(const PkStepArgs& a, const PkDoneArgs& d, hipStream_t s) {
    const u32 grid = ((a.env1 - a.env0 + PK_LANES - 1u) / PK_LANES) * PK_ROWS;
    hipLaunchKernelGGL(pk_render_kernel, dim3(grid), dim3(PK_LANES), 0, s, a, d);
    return hipGetLastError();
}

hipError_t pk_launch_render(const PkStepArgs& a, hipStream_t s) {
    PkDoneArgs d;
    memset(&d, 0, sizeof d);
    return pk_launch_render_done(a, d, s);
}

hipError_t pk_launch_render_latched(const PkStepArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(pk_arm_latches_kernel, dim3((a.env1 + 255) / 256), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return pk_launch_render(a, s);
}

hipError_t pk_launch_list(const u8* mask, u32 env0, u32 env1, u32* cnt, u32* ids, hipStream_t s) {
    hipLaunchKernelGGL(pk_list_kernel, dim3((env1 - env0 + 255) / 256), dim3(256), 0, s, mask, env0, env1, cnt, ids);
    return hipGetLastError();
}

// reset the envs listed in (a.cnt, a.ids)
hipError_t pk_launch_reset(const PkResetArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(pk_reset_mem_kernel, dim3(4096), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pk_reset_regs_kernel, dim3((a.env1 - a.env0 + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t pk_launch_gather_env(const u8* mem, u32 env, u32 sh, u8* out, hipStream_t s) {
    hipLaunchKernelGGL(pk_gather_env_kernel, dim3(64), dim3(256), 0, s, mem, env, sh, out);
    return hipGetLastError();
}

hipError_t pk_launch_gather_range(const u8* mem, u32 env0, u32 count, u32 sh, u8* out, hipStream_t s) {
    hipLaunchKernelGGL(pk_gather_range_kernel, dim3(2048), dim3(256), 0, s, mem, env0, count, sh, out);
    return hipGetLastError();
}

hipError_t pk_launch_scatter_env(u8* mem, u32 env, u32 sh, const u8* in, hipStream_t s) {
    hipLaunchKernelGGL(pk_scatter_env_kernel, dim3(64), dim3(256), 0, s, mem, env, sh, in);
    return hipGetLastError();
}

__global__ void pk_done_kernel(const u32* time_reg, u32 n, u32 max_steps, u8* term, u8* trunc, double* rew) {
    const u32 e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const u8 done = time_reg[e] >= max_steps ? 1 : 0;
    if (term) term[e] = done;
    if (trunc) trunc[e] = done;
    if (rew) rew[e] = 0.0;
}

hipError_t pk_launch_done(const u32* time_reg, u32 n, u32 max_steps, u8* term, u8* trunc, double* rew, hipStream_t s) {
    hipLaunchKernelGGL(pk_done_kernel, dim3((n + 255) / 256), dim3(256), 0, s, time_reg, n, max_steps, term, trunc, rew);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Savestate bank (pk_bank_save / pk_bank_load / pk_reset_from): envs <-> slots, every env naming
// its own slot.  Like K5 the kernels work on device-built lists, so the cost follows the envs
// touched and a call that touches none is a few near-empty launches.

// thread = env of the range: validate its slot before anything is written (a slot >= n_slots, or
// an empty one where the slot is the source — for a resume, A.ep, one without an episode part
// too — is counted and takes no part), record it in src[],
// and list the env — on the bank list, or (PK_BANK_RESET) on the range's template reset list when
// it reloads without a usable slot
__global__ void __launch_bounds__(256) pk_bank_list_kernel(PkBankArgs A) {
    const u32 e = A.env0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= A.env1) return;
    int32_t s = -1;
    bool tmpl = false;
    if (A.mode != PK_BANK_RESET || !A.sel || A.sel[e]) {
        s = A.slot_of_env[e];
        if (s < 0) {
            s = -1;
            tmpl = A.mode == PK_BANK_RESET;
        } else if ((u32)s >= A.n_slots || (A.mode != PK_BANK_SAVE && !A.b_filled[s]) ||
                   (A.mode == PK_BANK_LOAD && A.ep && !A.b_ep_filled[s])) {
            atomicAdd(A.b_rejects, 1u);
            s = -1;
            tmpl = A.mode == PK_BANK_RESET;
        }
    }
    A.src[e] = s;
    if (s >= 0) A.ids[atomicAdd(A.cnt, 1u)] = e;
    if (tmpl) A.tids[atomicAdd(A.tcnt, 1u)] = e;
}

// thread = sub-block (1 << ilv_sh envs) of the range: list it when one of its envs takes part
__global__ void __launch_bounds__(256) pk_bank_subs_kernel(PkBankArgs A) {
    const u32 sb = (A.env0 >> A.ilv_sh) + blockIdx.x * blockDim.x + threadIdx.x;
    const u32 e0 = sb << A.ilv_sh;
    for (u32 j = 0; j < (1u << A.ilv_sh); j++)
        if (e0 + j < A.env1 && A.src[e0 + j] >= 0) {
            A.subs[atomicAdd(A.cnt + 1, 1u)] = sb;
            return;
        }
}

// The RAM image, slot <-> env, as a tiled transposition through LDS.  A slot's image is linear
// and an env's is interleaved with its sub-block's (pk_img_off), so a lane walking its own slot
// would gather one byte per access.  Instead a workgroup takes one listed sub-block and a chunk of
// PK_BANK_TILE >> sh phys rows: on the slot side consecutive lanes move consecutive 16-byte
// pieces of one slot's chunk (coalesced), on the image side lane = 4 neighbouring envs of one
// row, so a wave's accesses to the image rows land in whole lines — the property
// pk_reset_mem_kernel documents.  Envs of the sub-block that take no part (src < 0, or outside
// the range) are never written: a group of 4 envs that is not complete is stored byte by byte.
// The tile keeps one env's rows together, padded by a word per env against bank conflicts.
// PK_BANK_SAVE stores the byte at PK_P_UNUSED as 0, as a parsed v9 state has it.
//
// The host-simulation build (tests/hostsim) gives a kernel concurrent threads and a working
// __syncthreads only when it is launched under a name that starts with PK_K1_KERNEL
// (hostsim_rt.cpp pk_sim_launch), hence the alias.
#define PK_K1_KERNEL_BANK_IMAGE pk_bank_image_kernel
template <bool SAVE>
__global__ void __launch_bounds__(256) pk_bank_image_kernel(PkBankArgs A) {
    __shared__ __attribute__((aligned(16))) u32 tile[PK_BANK_TILE / 4u + PK_LANES];
    u8* tile8 = reinterpret_cast<u8*>(tile);
    const u32 sh = A.ilv_sh, W = 1u << sh, R = PK_BANK_TILE >> sh, S = R / 4u + 1u;
    const u32 chunks = (PK_PHYS + R - 1u) / R;
    const u32 total = A.cnt[1] * chunks;
    const u32 G = W >= 4u ? 4u : W, gpr = W / G;   // envs per image-side item, items per row
    const u32 j0 = (threadIdx.x % gpr) * G;        // blockDim.x is a multiple of gpr: fixed per thread
    for (u32 w = blockIdx.x; w < total; w += gridDim.x) {
        const u32 e0 = A.subs[w / chunks] << sh, p0 = (w % chunks) * R;
        const u32 rows = PK_PHYS - p0 < R ? PK_PHYS - p0 : R, nq = rows / 16u;
        u8* img = A.mem + pk_img_off(e0, p0, sh);
        const bool word = G == 4u && (reinterpret_cast<uintptr_t>(img) & 3u) == 0u;
        u32 part = 0;   // which of this thread's envs take part
        for (u32 i = 0; i < G; i++)
            if (e0 + j0 + i < A.env1 && A.src[e0 + j0 + i] >= 0) part |= 1u << i;
        if (SAVE) {   // image rows -> tile
            for (u32 t = threadIdx.x; t < rows * gpr; t += blockDim.x) {
                const u32 r = t / gpr;
                const u8* d = img + ((size_t)r << sh) + j0;
                u32 v = 0;
                if (word) v = *reinterpret_cast<const u32*>(d);
                else for (u32 i = 0; i < G; i++) v |= (u32)d[i] << (8u * i);
                for (u32 i = 0; i < G; i++)
                    if (part >> i & 1u) tile8[(j0 + i) * S * 4u + r] = (u8)(v >> (8u * i));
            }
        }
        if (SAVE) __syncthreads();
        // slot side: 16-byte pieces, slot -> tile (load) or tile -> slot (save)
        for (u32 t = threadIdx.x; t < W * nq; t += blockDim.x) {
            const u32 j = t / nq, q = t - j * nq;
            const int32_t s = e0 + j < A.env1 ? A.src[e0 + j] : -1;
            if (s < 0) continue;
            uint4* bp = reinterpret_cast<uint4*>(A.b_mem + (size_t)s * PK_PHYS + p0) + q;
            u32* tp = tile + j * S + q * 4u;
            if (SAVE) {
                uint4 v;
                v.x = tp[0]; v.y = tp[1]; v.z = tp[2]; v.w = tp[3];
                if (p0 + q * 16u == (PK_P_UNUSED & ~15u)) v.w &= 0x00FFFFFFu;
                *bp = v;
            } else {
                const uint4 v = *bp;
                tp[0] = v.x; tp[1] = v.y; tp[2] = v.z; tp[3] = v.w;
            }
        }
        __syncthreads();
        if (!SAVE) {  // tile -> image rows
            for (u32 t = threadIdx.x; t < rows * gpr; t += blockDim.x) {
                const u32 r = t / gpr;
                u8* d = img + ((size_t)r << sh) + j0;
                u32 v = 0;
                for (u32 i = 0; i < G; i++)
                    if (part >> i & 1u) v |= (u32)tile8[(j0 + i) * S * 4u + r] << (8u * i);
                if (word && part == 0xFu) *reinterpret_cast<u32*>(d) = v;
                else for (u32 i = 0; i < G; i++)
                    if (part >> i & 1u) d[i] = (u8)(v >> (8u * i));
            }
            __syncthreads();   // the next tile's slot side overwrites what this one still reads
        }
    }
}

// registers, latches and screen of the listed envs, 16 threads per env so the screen's 16-byte
// pieces of one env go out side by side.  PK_BANK_LOAD writes what pk_load_env writes (registers
// 0..PK_R_MISC: the step counter and the render bookkeeping survive), PK_BANK_RESET every register,
// as a template reset does.  PK_BANK_SAVE stores what parse_v9 makes of the env's pk_snapshot: the
// register bits a v9 state has no room for dropped, PK_R_MISC as after a load, the step
// counters 0, and the latch words rebuilt from the current LCDC / palettes as the import does.
__global__ void __launch_bounds__(256) pk_bank_state_kernel(PkBankArgs A) {
    const u32 cnt = A.cnt[0], sub = threadIdx.x & 15u;
    for (u32 k = (blockIdx.x * blockDim.x + threadIdx.x) >> 4; k < cnt; k += (gridDim.x * blockDim.x) >> 4) {
        const u32 env = A.ids[k], s = (u32)A.src[env];
        const u32 gid = env / PK_LANES, lane = env % PK_LANES;
        u32* br = A.b_regs + (size_t)s * PK_BANK_REGS;
        u32* bl = A.b_lat + (size_t)s * 3u * PK_ROWS;
        uint4* bs = reinterpret_cast<uint4*>(A.b_screen + (size_t)s * PK_SCREEN);
        uint4* es = reinterpret_cast<uint4*>(A.screen + (size_t)env * PK_SCREEN);
        if (A.mode == PK_BANK_SAVE) {
            for (u32 f = sub; f < PK_BANK_REGS; f += 16u) {
                u32 v = f <= PK_R_MISC ? A.regs[f * A.npad + env] : 0u;
                if (f == PK_R_SP || f == PK_R_PC) v &= 0xFFFFu;
                if (f == PK_R_CPU) v &= 0x00FFFF17u;
                if (f == PK_R_MISC) v = 0x0Fu | (0x0Fu << 8);
                br[f] = v;
            }
            const u32 lcdc = A.regs[PK_R_LCD0 * A.npad + env] & 0xEFu;
            const u32 pal = A.regs[PK_R_LCD2 * A.npad + env] << 8;
            for (u32 i = sub; i < 3u * PK_ROWS; i += 16u) {
                const u32 j = i / PK_ROWS, y = i - j * PK_ROWS;
                u32 v = A.lat[j * A.lat_stride + (gid * PK_ROWS + y) * PK_LANES + lane];
                if (j == 0u) v = (v & 0xFFFFFF10u) | lcdc;
                else if (j == 1u) v = (v & 0xFFu) | pal;
                else v = 0u;
                bl[i] = v;
            }
            for (u32 q = sub; q < PK_SCREEN / 16u; q += 16u) bs[q] = es[q];
            if (sub == 0u) {
                A.b_filled[s] = 1;
                if (A.b_ep_filled) A.b_ep_filled[s] = A.ep ? 1 : 0;
            }
        } else {
            const u32 nr = A.mode == PK_BANK_RESET ? (u32)PK_NREGS : (u32)PK_R_MISC + 1u;
            for (u32 f = sub; f < nr; f += 16u) A.regs[f * A.npad + env] = br[f];
            for (u32 i = sub; i < 3u * PK_ROWS; i += 16u) {
                const u32 j = i / PK_ROWS, y = i - j * PK_ROWS;
                A.lat[j * A.lat_stride + (gid * PK_ROWS + y) * PK_LANES + lane] = bl[i];
            }
            for (u32 q = sub; q < PK_SCREEN / 16u; q += 16u) es[q] = bs[q];
        }
    }
}

// build the range's bank lists (and, PK_BANK_RESET, its template reset list); the counters are zero
hipError_t pk_launch_bank_list(const PkBankArgs& a, hipStream_t s) {
    const u32 count = a.env1 - a.env0;
    hipLaunchKernelGGL(pk_bank_list_kernel, dim3((count + 255u) / 256u), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const u32 nsub = (count + (1u << a.ilv_sh) - 1u) >> a.ilv_sh;
    hipLaunchKernelGGL(pk_bank_subs_kernel, dim3((nsub + 255u) / 256u), dim3(256), 0, s, a);
    return hipGetLastError();
}

// move the listed envs' state (a.mode)
hipError_t pk_launch_bank_copy(const PkBankArgs& a, hipStream_t s) {
    const u32 count = a.env1 - a.env0, R = PK_BANK_TILE >> a.ilv_sh;
    const u32 nsub = (count + (1u << a.ilv_sh) - 1u) >> a.ilv_sh;
    const uint64_t items = (uint64_t)nsub * ((PK_PHYS + R - 1u) / R);
    const u32 grid = items < 4096u ? (u32)items : 4096u;
    if (a.mode == PK_BANK_SAVE) hipLaunchKernelGGL((PK_K1_KERNEL_BANK_IMAGE<true>), dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((PK_K1_KERNEL_BANK_IMAGE<false>), dim3(grid), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const u32 sgrid = (count * 16u + 255u) / 256u;
    hipLaunchKernelGGL(pk_bank_state_kernel, dim3(sgrid < 4096u ? sgrid : 4096u), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Exploration archive (pk_archive_update / pk_archive_explore / pk_cell_keys): cells of the best
// episode per key, kept next to the bank.  The result of an update is the one of walking the envs
// in ascending order (include/pokegym_amd.h states the model); the kernels reach it without any
// order among threads: integer adds, 64-bit max / min on order-preserving words and a scan.  The
// phases are separate launches, so no kernel waits for another thread or workgroup, and every
// probe loop ends after one pass over its table at the latest (the tables are at most half full).
typedef uint64_t u64;
typedef unsigned long long ull;

#ifndef __HIPCC__
// host versions for the host-simulation build, whose shim has the 32-bit atomicAdd only.  Its
// "wave" is one lane (the ballot is this lane's bit 0), so a shuffle returns the lane's own value.
static inline ull atomicAdd(ull* p, ull v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
static inline ull atomicCAS(ull* p, ull cmp, ull v) {
    __atomic_compare_exchange_n(p, &cmp, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
    return cmp;
}
static inline ull atomicMax(ull* p, ull v) {
    ull old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old < v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
}
static inline ull atomicMin(ull* p, ull v) {
    ull old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old > v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
}
static inline u32 atomicMin(u32* p, u32 v) {
    u32 old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old > v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
}
static inline u32 __shfl(u32 v, int) { return v; }
static inline ull __shfl_xor(ull v, int) { return v; }
static inline u32 pk_lane() { return 0u; }
#else
__device__ static inline u32 pk_lane() { return threadIdx.x & 63u; }
#endif

// IEEE order of non-NaN doubles as unsigned order, -0.0 and +0.0 the same word; never 0
__device__ static inline u64 pk_arch_enc(double d) {
    d += 0.0;
    u64 b;
    memcpy(&b, &d, 8);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ static inline u64 pk_arch_mix(u64 z) {   // splitmix64's finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// One round of the wave pre-reduction: the pending lanes (todo) that share the target of the first
// pending lane form a group (match, its lanes mm); lead marks that first lane, which is the
// group's lowest env.  False when no lane is pending.  Every lane of the wave calls it.
__device__ static inline bool pk_arch_group(bool todo, u32 t, bool& match, bool& lead, u64& mm) {
    const u64 m = __builtin_amdgcn_ballot_w64(todo);
    if (!m) return false;
    const u32 leader = (u32)__builtin_ffsll((long long)m) - 1u;
    const u32 lt = __shfl(t, (int)leader);
    match = todo && t == lt;
    mm = __builtin_amdgcn_ballot_w64(match);
    lead = pk_lane() == leader;
    return true;
}

// the words an item brings to an update or a merge: whether it takes part, its encoded score and
// length << 32 | index.  An item is an env (REC = false) or record e of a merge: its length comes from
// the record, pay says whether it brings a payload (an env always does: its own state), and reject
// that it is counted as a reject (a foreign format, a payload row past the array, a NaN score).
template <bool REC>
__device__ static inline bool pk_arch_item(const PkArchArgs& A, u32 e, u64& key, u64& enc, u64& le, bool& pay, bool& reject) {
    pay = true;
    reject = false;
    if (e >= A.env1) return false;
    double sc;
    u32 len;
    if (REC) {
        const pk_xrec& r = A.rec[e];
        key = r.key;
        if (key == PK_ARCH_NOKEY) return false;
        sc = r.score;
        pay = r.payload >= 0;
        if (r.format != A.format || (pay && (u32)r.payload >= A.n_payloads) || sc != sc) {
            reject = true;
            return false;
        }
        len = r.length;
    } else {
        if (A.mask && !A.mask[e]) return false;
        key = A.keys[e];
        sc = A.scores[e];
        if (key == PK_ARCH_NOKEY || sc != sc) return false;
        len = A.time_reg[e];
    }
    enc = pk_arch_enc(sc);
    le = ((u64)len << 32) | e;
    return true;
}

// phase 1, thread = env: find the key's cell in the index, else claim a scratch entry for it; count
// the visit, and bring the score to the target's max word — for a known cell only where it beats
// the stored record (a better score, or the same score in fewer steps).  A merge (REC) adds the
// record's own visit and pick counts, to the sent words as well; only a record with a payload is a
// candidate, and for a new key the first such record is the one that makes the cell: what the
// records of a new key count is settled in phase 2, when that first record is known.  Records
// seldom share a cell, so a merge skips the wave pre-reduction.
template <bool REC>
__global__ void __launch_bounds__(256) pk_arch_claim_kernel(PkArchArgs A) {
    const u32 e = A.env0 + blockIdx.x * blockDim.x + threadIdx.x;
    u64 key = PK_ARCH_NOKEY, enc = 0, le = 0;
    u32 t = PK_ARCH_NONE;
    bool cand = false, pay, reject;
    if (pk_arch_item<REC>(A, e, key, enc, le, pay, reject)) {
        const u32 h = (u32)pk_arch_mix(key);
        u32 pos = h & A.i_mask;
        for (u32 p = 0; p <= A.i_mask; p++, pos = (pos + 1u) & A.i_mask) {
            const u64 k = A.i_key[pos];
            if (k == key) t = A.i_cell[pos];
            if (k == key || k == PK_ARCH_NOKEY) break;
        }
        if (t != PK_ARCH_NONE) {
            const u64 renc = pk_arch_enc(A.a_score[t]);
            cand = pay && (enc > renc || (enc == renc && (u32)(le >> 32) < A.a_len[t]));
        } else {
            pos = h & A.s_mask;
            for (u32 p = 0; p <= A.s_mask; p++, pos = (pos + 1u) & A.s_mask) {
                ull* sk = reinterpret_cast<ull*>(A.s_key + pos);
                u64 k = *sk;
                if (k == PK_ARCH_NOKEY) k = atomicCAS(sk, (ull)PK_ARCH_NOKEY, (ull)key);
                if (k == PK_ARCH_NOKEY || k == key) {
                    t = A.n_cells + pos;
                    cand = pay;
                    break;
                }
            }
        }
    }
    if (e < A.env1) A.tgt[e] = t;
    if (REC) {
        if (reject) atomicAdd(A.b_rejects, 1u);
        if (t == PK_ARCH_NONE) return;
        if (t < A.n_cells) {
            const u32 rv = A.rec[e].visits, rp = A.rec[e].picks;
            if (rv) {
                atomicAdd(A.a_visits + t, rv);
                atomicAdd(A.x_sent_visits + t, rv);
            }
            if (rp) {
                atomicAdd(A.a_picks + t, rp);
                atomicAdd(A.x_sent_picks + t, rp);
            }
            if (cand) atomicMax(reinterpret_cast<ull*>(A.c_max + t), (ull)enc);
        } else if (cand) {
            atomicMax(reinterpret_cast<ull*>(A.s_max + (t - A.n_cells)), (ull)enc);
            atomicMin(A.s_first + (t - A.n_cells), e);
        }
        return;
    }
    bool todo = t != PK_ARCH_NONE, match, lead;
    u64 mm;
    for (u32 it = 0; it <= PK_ARCH_PRE; it++) {
        u32 n = 1;
        u64 best = cand ? enc : 0;
        if (it < PK_ARCH_PRE) {   // a group per round; after the last round every lane goes alone
            if (!pk_arch_group(todo, t, match, lead, mm)) break;
            best = match ? best : 0;
            for (int o = 32; o; o >>= 1) {
                const u64 other = __shfl_xor((ull)best, o);
                best = other > best ? other : best;
            }
            n = (u32)__builtin_popcountll(mm);
        } else {
            match = lead = todo;
        }
        if (lead && match) {
            if (t < A.n_cells) {
                atomicAdd(A.a_visits + t, n);
                if (best) atomicMax(reinterpret_cast<ull*>(A.c_max + t), (ull)best);
            } else {
                const u32 j = t - A.n_cells;
                atomicAdd(A.s_cnt + j, n);
                atomicMax(reinterpret_cast<ull*>(A.s_max + j), (ull)best);
                atomicMin(A.s_first + j, e);
            }
        }
        todo = todo && !match;
    }
}

// phase 2, thread = env: among the envs that hold the target's best score, the least length, then
// the least env; and flag the env that is the first of a new key.  In a merge (REC) the first
// record of a new key is its first record with a payload: the records before it (or all, when no
// record of the key has a payload) found no cell and count as overflow, those from it on bring
// their visits and picks to the entry.
template <bool REC>
__global__ void __launch_bounds__(256) pk_arch_best_kernel(PkArchArgs A) {
    const u32 e = A.env0 + blockIdx.x * blockDim.x + threadIdx.x;
    u64 key, enc = 0, le = 0;
    u32 t = e < A.env1 ? A.tgt[e] : PK_ARCH_NONE;
    bool todo = false, match, lead, pay, reject;
    if (t != PK_ARCH_NONE) {
        pk_arch_item<REC>(A, e, key, enc, le, pay, reject);
        const u32 j = t - A.n_cells;
        if (REC && t >= A.n_cells) {
            const u32 first = A.s_first[j];
            if (first == PK_ARCH_NONE || e < first) {
                atomicAdd(reinterpret_cast<ull*>(A.hdr + PK_AH_OVERFLOW), 1ull);
                A.tgt[e] = t = PK_ARCH_NONE;
            } else {
                atomicAdd(A.s_cnt + j, 1u);
                atomicAdd(A.s_vis + j, A.rec[e].visits);
                atomicAdd(A.s_pick + j, A.rec[e].picks);
            }
        }
    }
    if (t != PK_ARCH_NONE) {
        const u32 j = t - A.n_cells;
        todo = pay && enc == (t < A.n_cells ? A.c_max[t] : A.s_max[j]);
        A.flag[e] = t >= A.n_cells && A.s_first[j] == e ? 1 : 0;
    } else if (e < A.env1) {
        A.flag[e] = 0;
    }
    if (REC) {
        if (todo) atomicMin(reinterpret_cast<ull*>(t < A.n_cells ? A.c_le + t : A.s_le + (t - A.n_cells)), (ull)le);
        return;
    }
    u64 mm;
    for (u32 it = 0; it <= PK_ARCH_PRE; it++) {
        u64 least = le;
        if (it < PK_ARCH_PRE) {
            if (!pk_arch_group(todo, t, match, lead, mm)) break;
            least = match ? least : ~0ull;
            for (int o = 32; o; o >>= 1) {
                const u64 other = __shfl_xor((ull)least, o);
                least = other < least ? other : least;
            }
        } else {
            match = lead = todo;
        }
        if (lead && match) atomicMin(reinterpret_cast<ull*>(t < A.n_cells ? A.c_le + t : A.s_le + (t - A.n_cells)), (ull)least);
        todo = todo && !match;
    }
}

// phase 3, one workgroup: number the new keys in the order of their first envs (a scan of the
// flags), give them the free cells, and count the envs of the keys that found the archive full
#define PK_K1_KERNEL_ARCH_RANK pk_arch_rank_kernel
__global__ void __launch_bounds__(256) pk_arch_rank_kernel(PkArchArgs A) {
    __shared__ u32 sums[256];
    const u32 tid = threadIdx.x, count = A.env1 - A.env0, chunk = (count + 255u) / 256u;
    const u32 b = A.env0 + (tid * chunk < count ? tid * chunk : count);
    const u32 end = A.env1 - b < chunk ? A.env1 : b + chunk;
    const u32 used0 = (u32)A.hdr[PK_AH_USED];
    u32 s = 0;
    for (u32 e = b; e < end; e++) s += A.flag[e];
    sums[tid] = s;
    __syncthreads();
    for (u32 o = 1; o < 256u; o <<= 1) {
        const u32 v = tid >= o ? sums[tid - o] : 0u;
        __syncthreads();
        sums[tid] += v;
        __syncthreads();
    }
    u32 r = used0 + sums[tid] - s;
    const u32 total = used0 + sums[255];
    ull lost = 0;
    for (u32 e = b; e < end; e++) {
        if (!A.flag[e]) continue;
        const u32 j = A.tgt[e] - A.n_cells;
        if (r < A.n_cells) {
            A.s_cell[j] = r;
        } else {
            A.s_cell[j] = PK_ARCH_NONE;
            lost += A.s_cnt[j];
        }
        r++;
    }
    if (lost) atomicAdd(reinterpret_cast<ull*>(A.hdr + PK_AH_OVERFLOW), lost);
    if (tid == 0) A.hdr[PK_AH_USED] = total < A.n_cells ? total : A.n_cells;
}

// phase 4, thread = env: the first env of an accepted new key writes the cell and enters the key
// into the index; the winner of a target writes the record; every env gets its line of the slot map.
// On a handle with archive exchange an update's winner marks its cell dirty.  A merge (REC) starts a
// new cell with the counts its records brought, all of them sent words too, lists each winner's
// cell and payload row for the mover, never touches dirty, and writes cell_out in the map's place.
template <bool REC>
__global__ void __launch_bounds__(256) pk_arch_commit_kernel(PkArchArgs A) {
    const u32 e = A.env0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= A.env1) return;
    const u32 t = A.tgt[e];
    int32_t slot = -1, cell = -1;
    u64 key, enc, le;
    bool pay, reject;
    if (t != PK_ARCH_NONE) {
        pk_arch_item<REC>(A, e, key, enc, le, pay, reject);
        u32 c = t;
        bool win;
        if (t < A.n_cells) {
            win = pay && enc == A.c_max[t] && le == A.c_le[t];
        } else {
            const u32 j = t - A.n_cells;
            c = A.s_cell[j];
            win = c != PK_ARCH_NONE && pay && enc == A.s_max[j] && le == A.s_le[j];
            if (c != PK_ARCH_NONE && A.s_first[j] == e) {
                A.a_key[c] = key;
                A.a_visits[c] = REC ? A.s_vis[j] : A.s_cnt[j];
                A.a_picks[c] = REC ? A.s_pick[j] : 0u;
                if (REC) {
                    A.x_sent_visits[c] = A.s_vis[j];
                    A.x_sent_picks[c] = A.s_pick[j];
                }
                u32 pos = (u32)pk_arch_mix(key) & A.i_mask;
                for (u32 p = 0; p <= A.i_mask; p++, pos = (pos + 1u) & A.i_mask) {
                    ull* ik = reinterpret_cast<ull*>(A.i_key + pos);
                    if (*ik != PK_ARCH_NOKEY) continue;
                    if (atomicCAS(ik, (ull)PK_ARCH_NOKEY, (ull)key) == PK_ARCH_NOKEY) {
                        A.i_cell[pos] = c;
                        break;
                    }
                }
            }
        }
        if (win) {
            A.a_score[c] = REC ? A.rec[e].score : A.scores[e];
            A.a_len[c] = (u32)(le >> 32);
            slot = (int32_t)(A.slot0 + c);
            cell = (int32_t)c;
            if (REC) {
                const u32 k = atomicAdd(A.x_cnt, 1u);
                A.x_cell[k] = c;
                A.x_pay[k] = (u32)A.rec[e].payload;
            } else if (A.x_dirty) {
                A.x_dirty[c] = 1u;
            }
        }
    }
    if (!REC) A.map[e] = slot;
    else if (A.out) A.out[e] = cell;
}

// explore, one workgroup: the weights of the cells in use (Go-Explore's 1 / sqrt(n + 1) in fixed
// point, integers only) and their inclusive prefix sums; the call takes its number
#define PK_K1_KERNEL_ARCH_SCAN pk_arch_scan_kernel
__device__ static inline u64 pk_arch_weight(u32 visits, u32 picks) {
    const u64 x = ((u64)visits + picks + 1u) << 16;     // < 2^50: exact as a double
    u64 r = (u64)sqrt((double)x);
    if (r * r > x) r--;
    if ((r + 1u) * (r + 1u) <= x) r++;
    return (1ull << 32) / r;
}
__global__ void __launch_bounds__(256) pk_arch_scan_kernel(PkArchArgs A) {
    __shared__ u64 sums[256];
    const u32 tid = threadIdx.x, used = (u32)A.hdr[PK_AH_USED], chunk = (used + 255u) / 256u;
    const u32 b = tid * chunk < used ? tid * chunk : used;
    const u32 end = used - b < chunk ? used : b + chunk;
    u64 s = 0;
    for (u32 c = b; c < end; c++) s += pk_arch_weight(A.a_visits[c], A.a_picks[c]);
    sums[tid] = s;
    __syncthreads();
    for (u32 o = 1; o < 256u; o <<= 1) {
        const u64 v = tid >= o ? sums[tid - o] : 0u;
        __syncthreads();
        sums[tid] += v;
        __syncthreads();
    }
    u64 run = sums[tid] - s;
    for (u32 c = b; c < end; c++) {
        run += pk_arch_weight(A.a_visits[c], A.a_picks[c]);
        A.prefix[c] = run;
    }
    if (tid == 0) {
        A.hdr[PK_AH_TOTAL] = sums[255];
        A.hdr[PK_AH_CUR] = A.hdr[PK_AH_DRAWS];
        A.hdr[PK_AH_DRAWS] += 1u;
    }
}

// explore, thread = env: draw a cell by the prefix sums and count the pick.  The picks only enter
// the weights of the next call's scan, so every draw of a call sees one distribution.
__global__ void __launch_bounds__(256) pk_arch_draw_kernel(PkArchArgs A) {
    const u32 e = A.env0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= A.env1) return;
    int32_t slot = -1;
    if (!A.mask || A.mask[e]) {
        const u32 used = (u32)A.hdr[PK_AH_USED];
        if (!used) {
            atomicAdd(A.b_rejects, 1u);
        } else {
            const u64 x = A.seed + 0x9E3779B97F4A7C15ull * ((A.hdr[PK_AH_CUR] << 32) + e + 1u);
            const u64 r = pk_arch_mix(x) % A.hdr[PK_AH_TOTAL];
            u32 lo = 0, hi = used - 1u;
            for (u32 it = 0; it < 17u && lo < hi; it++) {   // used <= 2^16
                const u32 mid = (lo + hi) >> 1;
                if (A.prefix[mid] > r) hi = mid;
                else lo = mid + 1u;
            }
            atomicAdd(A.a_picks + lo, 1u);
            slot = (int32_t)(A.slot0 + lo);
        }
    }
    A.map[e] = slot;
}

// the caller's slot_of_env_out: the slot the bank accepted for the env, -1 for every other env
__global__ void __launch_bounds__(256) pk_arch_out_kernel(PkArchArgs A) {
    const u32 e = A.env0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (e < A.env1) A.out[e] = A.src[e];
}

// pk_cell_keys, thread = env: map | (x >> shift) << 8 | (y >> shift) << 16 | badges << 24
__global__ void __launch_bounds__(256) pk_cell_keys_kernel(const u8* mem, u32 sh, u32 shift, u64* keys, u32 env0, u32 env1) {
    const u32 e = env0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= env1) return;
    const u32 w = PK_P_WRAM - 0xC000u;
    const u64 map = mem[pk_img_off(e, w + 0xD35Eu, sh)], x = mem[pk_img_off(e, w + 0xD362u, sh)];
    const u64 y = mem[pk_img_off(e, w + 0xD361u, sh)], badges = mem[pk_img_off(e, w + 0xD356u, sh)];
    keys[e] = map | (x >> shift) << 8 | (y >> shift) << 16 | badges << 24;
}

static inline dim3 pk_arch_grid(const PkArchArgs& a) { return dim3((a.env1 - a.env0 + 255u) / 256u); }

// phases 1-4 of pk_archive_update; the per-call words are cleared
hipError_t pk_launch_arch_update(const PkArchArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((pk_arch_claim_kernel<false>), pk_arch_grid(a), dim3(256), 0, s, a);
    hipLaunchKernelGGL((pk_arch_best_kernel<false>), pk_arch_grid(a), dim3(256), 0, s, a);
    hipLaunchKernelGGL(PK_K1_KERNEL_ARCH_RANK, dim3(1), dim3(256), 0, s, a);
    hipLaunchKernelGGL((pk_arch_commit_kernel<false>), pk_arch_grid(a), dim3(256), 0, s, a);
    return hipGetLastError();
}

// the same four phases over the records of a pk_archive_merge (a.rec, items [0, a.env1)); leaves the
// list of winners (x_cnt, x_cell, x_pay) for pk_launch_xchg_move
hipError_t pk_launch_arch_merge(const PkArchArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((pk_arch_claim_kernel<true>), pk_arch_grid(a), dim3(256), 0, s, a);
    hipLaunchKernelGGL((pk_arch_best_kernel<true>), pk_arch_grid(a), dim3(256), 0, s, a);
    hipLaunchKernelGGL(PK_K1_KERNEL_ARCH_RANK, dim3(1), dim3(256), 0, s, a);
    hipLaunchKernelGGL((pk_arch_commit_kernel<true>), pk_arch_grid(a), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t pk_launch_arch_draw(const PkArchArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(PK_K1_KERNEL_ARCH_SCAN, dim3(1), dim3(256), 0, s, a);
    hipLaunchKernelGGL(pk_arch_draw_kernel, pk_arch_grid(a), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t pk_launch_arch_out(const PkArchArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(pk_arch_out_kernel, pk_arch_grid(a), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t pk_launch_cell_keys(const u8* mem, u32 sh, u32 shift, u64* keys, u32 env0, u32 env1, hipStream_t s) {
    hipLaunchKernelGGL(pk_cell_keys_kernel, dim3((env1 - env0 + 255u) / 256u), dim3(256), 0, s, mem, sh, shift, keys, env0, env1);
    return hipGetLastError();
}

// pk_frame_keys, workgroup = env: the screen downscaled to blocks of bw x bh pixels, each quantised to
// `levels` levels, and the 64-bit key of that cell image (include/pokegym_amd.h states the model).
// The screen is read once: lane l of pass k loads 16-byte piece PK_CELLS_WG * k + l, eight passes in
// flight, and leaves the pixel sums of the piece's two halves (8 pixels each, <= 24) as two bytes in
// LDS.  Behind one barrier, thread i adds the half sums of block i, quantises, writes the cell and
// forms the block's 64-bit term.  The terms are added through LDS in two steps, not by shuffles: the
// host-simulation build's wave is one lane.  A workgroup is one wave, so its barriers cost nothing
// and a CU holds as many screens in flight as it holds waves.
#ifndef PK_CELLS_WG
#define PK_CELLS_WG 64u
#endif
#define PK_CELLS_PASSES ((PK_CELL_PIECES + PK_CELLS_WG - 1u) / PK_CELLS_WG)
#define PK_K1_KERNEL_FRAME_KEYS pk_frame_keys_kernel
__global__ void __launch_bounds__(PK_CELLS_WG) pk_frame_keys_kernel(PkCellArgs A) {
    __shared__ uint16_t half[PK_CELL_PIECES];   // piece p: left half sum | right half sum << 8
    __shared__ u64 red[PK_CELLS_WG];
    const u32 tid = threadIdx.x, e = A.env0 + blockIdx.x;
    const uint4* src = reinterpret_cast<const uint4*>(A.screen + (size_t)e * PK_SCREEN);
#pragma unroll
    for (u32 k0 = 0; k0 < PK_CELLS_PASSES; k0 += 8u) {
        uint4 w[8];
#pragma unroll
        for (u32 j = 0; j < 8u; j++) {
            const u32 p = (k0 + j) * PK_CELLS_WG + tid;
            if (k0 + j < PK_CELLS_PASSES && p < PK_CELL_PIECES) w[j] = src[p];
        }
#pragma unroll
        for (u32 j = 0; j < 8u; j++) {
            const u32 p = (k0 + j) * PK_CELLS_WG + tid;
            if (k0 + j >= PK_CELLS_PASSES || p >= PK_CELL_PIECES) continue;
            // v = byte >> 6 per pixel; two dwords added bytewise (<= 6 a byte), then the four bytes summed
            const u32 lo = ((w[j].x >> 6) & 0x03030303u) + ((w[j].y >> 6) & 0x03030303u);
            const u32 hi = ((w[j].z >> 6) & 0x03030303u) + ((w[j].w >> 6) & 0x03030303u);
            half[p] = (uint16_t)(((lo * 0x01010101u) >> 24) | ((hi * 0x01010101u) >> 24) << 8);
        }
    }
    __syncthreads();
    // half sum h = 20 y + x / 8 is byte h of the array: a block is tw of them in each of its bh rows
    const u8* hb = reinterpret_cast<const u8*>(half);
    const u32 nbx = PK_COLS / A.bw, tw = A.bw / 8u, nblk = nbx * (PK_ROWS / A.bh);
    const u32 div = 3u * A.bw * A.bh + 1u;
    u64 acc = 0;
    for (u32 i = tid; i < nblk; i += PK_CELLS_WG) {
        const u32 h0 = (i / nbx) * A.bh * PK_CELL_TILES_X + (i % nbx) * tw;
        u32 s = 0;
        for (u32 r = 0; r < A.bh; r++)
            for (u32 c = 0; c < tw; c++) s += hb[h0 + r * PK_CELL_TILES_X + c];
        const u32 q = s * A.levels / div;       // s * levels <= 3 * 23,040 * 256 < 2^25
        if (A.cells) A.cells[(size_t)e * nblk + i] = (u8)q;
        acc += pk_arch_mix(PK_CELL_GOLD * (i + 1u) + q);
    }
    red[tid] = acc;
    __syncthreads();
    const u32 span = PK_CELLS_WG / 8u;
    if (tid < 8u) {
        u64 s = 0;
        for (u32 j = 0; j < span; j++) s += red[tid * span + j];
        red[tid * span] = s;
    }
    __syncthreads();
    if (tid == 0) {
        u64 sum = 0;
        for (u32 j = 0; j < 8u; j++) sum += red[j * span];
        const u64 salt = A.salt ? A.salt[e] : 0;
        if (A.salt) sum += pk_arch_mix(salt);
        u64 key = pk_arch_mix(sum);
        if (key == PK_ARCH_NOKEY) key = PK_ARCH_NOKEY - 1u;
        if (A.salt && salt == PK_ARCH_NOKEY) key = PK_ARCH_NOKEY;   // "no cell" passes through
        A.keys[e] = key;
    }
}

hipError_t pk_launch_frame_keys(const PkCellArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(PK_K1_KERNEL_FRAME_KEYS, dim3(a.env1 - a.env0), dim3(PK_CELLS_WG), 0, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Frame stack (pk_fstack_push): the downscaled screen pushed onto, or filled into, every env's stack
// of D planes, in place (include/pokegym_amd.h states the model).  thread = one piece of PX
// consecutive output pixels of one row: it reads the S x S source pixels of each from the screen and
// the older bytes of the same pixels from the stack into registers, then writes.  No thread reads
// what another writes, so there is no barrier and no second buffer.  A workgroup is one wave and
// works on one env (the mask byte is wave-uniform); consecutive lanes take consecutive pieces, so a
// wave's loads and stores are consecutive 16-byte (8-byte at S = 4 in CHW) pieces of a plane.
//   CHW  PX = 16 (S = 1, 2) or 8 (S = 4): D - 1 pieces read, D written, one per plane.
//   HWC  PX = 16 / D: the D bytes of the PX pixels are one 16-byte piece, a pixel's bytes newest
//        first, so a push is a shift by one byte: (old << 8) | new on a dword at D = 4.
#ifndef PK_FS_WG
#define PK_FS_WG 64u
#endif

template <u32 B> __device__ __forceinline__ void pk_fs_ld(const u8* p, u32* w) {
    if constexpr (B == 32u) {
        pk_fs_ld<16u>(p, w);
        pk_fs_ld<16u>(p + 16, w + 4);
    } else if constexpr (B == 16u) {
        const uint4 v = *reinterpret_cast<const uint4*>(p);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else if constexpr (B == 8u) {
        const uint2 v = *reinterpret_cast<const uint2*>(p);
        w[0] = v.x; w[1] = v.y;
    } else if constexpr (B == 4u) {
        w[0] = *reinterpret_cast<const u32*>(p);
    } else {
        w[0] = *reinterpret_cast<const uint16_t*>(p);
    }
}

template <u32 B> __device__ __forceinline__ void pk_fs_st(u8* p, const u32* w) {
    if constexpr (B == 16u) *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
    else *reinterpret_cast<uint2*>(p) = make_uint2(w[0], w[1]);
}

__device__ __forceinline__ u32 pk_fs_byte(const u32* w, u32 j) { return (w[j >> 2] >> (8u * (j & 3u))) & 0xFFu; }

// the PX new pixels of a piece, packed four to a word: the rounded mean of each S x S block, or its
// top left pixel
template <u32 S, u32 PX> __device__ __forceinline__ void pk_fs_plane(const u8* src, u32 pick, u32* nw) {
    constexpr u32 B = S * PX, NB = (B + 3u) / 4u, NW = (PX + 3u) / 4u;
    u32 w[S][NB];
    pk_fs_ld<B>(src, w[0]);
#pragma unroll
    for (u32 dy = 1; dy < S; dy++) {
#pragma unroll
        for (u32 j = 0; j < NB; j++) w[dy][j] = 0;
        if (!pick) pk_fs_ld<B>(src + dy * PK_COLS, w[dy]);
    }
#pragma unroll
    for (u32 i = 0; i < NW; i++) nw[i] = 0;
#pragma unroll
    for (u32 i = 0; i < PX; i++) {
        u32 sum = 0;
#pragma unroll
        for (u32 dy = 0; dy < S; dy++)
#pragma unroll
            for (u32 dx = 0; dx < S; dx++) sum += pk_fs_byte(w[dy], S * i + dx);
        const u32 v = pick ? pk_fs_byte(w[0], S * i) : (sum + S * S / 2u) / (S * S);
        nw[i >> 2] |= v << (8u * (i & 3u));
    }
}

template <u32 S, u32 PX, bool HWC> __global__ void __launch_bounds__(PK_FS_WG) pk_fstack_kernel(PkStackArgs A) {
    constexpr u32 H = PK_ROWS / S, W = PK_COLS / S, PPR = W / PX, P = H * PPR, NW = (PX + 3u) / 4u;
    constexpr u32 BPE = (P + PK_FS_WG - 1u) / PK_FS_WG;
    const u32 e = A.env0 + blockIdx.x / BPE, p = (blockIdx.x % BPE) * PK_FS_WG + threadIdx.x;
    if (e >= A.env1 || p >= P) return;
    const u32 m = A.mask ? A.mask[e] : 0u;
    if (A.fill_only && A.mask && !m) return;
    const bool fill = A.fill_only || m;
    const u32 y = p / PPR, x0 = (p % PPR) * PX;
    const u8* src = A.screen + (size_t)e * PK_SCREEN + (size_t)(S * y) * PK_COLS + S * x0;
    u32 nw[NW];
    if constexpr (!HWC) {
        u8* dst = A.stack + (size_t)e * A.depth * (H * W) + (size_t)p * PX;
        u32 old[PK_FS_MAX_DEPTH][NW];          // old[k]: what plane k takes
        pk_fs_plane<S, PX>(src, A.mode, nw);   // its loads and the older pieces' are all issued before a store
#pragma unroll
        for (u32 k = 1; k < PK_FS_MAX_DEPTH; k++) {
            if (k >= A.depth) continue;
            if (fill) {
#pragma unroll
                for (u32 i = 0; i < NW; i++) old[k][i] = nw[i];
            } else {
                pk_fs_ld<PX>(dst + (size_t)(k - 1u) * (H * W), old[k]);
            }
        }
        pk_fs_st<PX>(dst, nw);
#pragma unroll
        for (u32 k = 1; k < PK_FS_MAX_DEPTH; k++)
            if (k < A.depth) pk_fs_st<PX>(dst + (size_t)k * (H * W), old[k]);
    } else {
        constexpr u32 D = 16u / PX;
        u8* dst = A.stack + ((size_t)e * (H * W) + (size_t)p * PX) * D;
        u32 o[4] = {0u, 0u, 0u, 0u}, r[4];
        if (!fill) pk_fs_ld<16u>(dst, o);
        pk_fs_plane<S, PX>(src, A.mode, nw);
        if constexpr (D == 2u) {
#pragma unroll
            for (u32 j = 0; j < 4u; j++) {
                const u32 nn = pk_fs_byte(nw, 2u * j) | pk_fs_byte(nw, 2u * j + 1u) << 16;
                r[j] = fill ? nn * 0x0101u : (((o[j] << 8) & 0xFF00FF00u) | nn);
            }
        } else if constexpr (D == 4u) {
#pragma unroll
            for (u32 j = 0; j < 4u; j++) {
                const u32 nn = pk_fs_byte(nw, j);
                r[j] = fill ? nn * 0x01010101u : ((o[j] << 8) | nn);
            }
        } else {
#pragma unroll
            for (u32 j = 0; j < 2u; j++) {
                const u32 nn = pk_fs_byte(nw, j);
                r[2u * j] = fill ? nn * 0x01010101u : ((o[2u * j] << 8) | nn);
                r[2u * j + 1u] = fill ? nn * 0x01010101u : ((o[2u * j + 1u] << 8) | (o[2u * j] >> 24));
            }
        }
        pk_fs_st<16u>(dst, r);
    }
}

template <u32 S, u32 PX, bool HWC> static hipError_t pk_fs_launch(const PkStackArgs& a, hipStream_t s) {
    constexpr u32 P = (PK_ROWS / S) * (PK_COLS / S / PX), BPE = (P + PK_FS_WG - 1u) / PK_FS_WG;
    hipLaunchKernelGGL((pk_fstack_kernel<S, PX, HWC>), dim3((a.env1 - a.env0) * BPE), dim3(PK_FS_WG), 0, s, a);
    return hipGetLastError();
}

// scale 1, 2, 4; depth 1..8 in CHW and 1, 2, 4, 8 in HWC (pk_fstack_create checks): at depth 1 the
// two layouts are the same bytes
hipError_t pk_launch_fstack(const PkStackArgs& a, hipStream_t s) {
    const u32 d = a.layout && a.depth > 1u ? a.depth : 0u;
    switch (a.scale * 16u + d) {
    case 16u: return pk_fs_launch<1u, 16u, false>(a, s);
    case 32u: return pk_fs_launch<2u, 16u, false>(a, s);
    case 64u: return pk_fs_launch<4u, 8u, false>(a, s);
    case 16u + 2u: return pk_fs_launch<1u, 8u, true>(a, s);
    case 16u + 4u: return pk_fs_launch<1u, 4u, true>(a, s);
    case 16u + 8u: return pk_fs_launch<1u, 2u, true>(a, s);
    case 32u + 2u: return pk_fs_launch<2u, 8u, true>(a, s);
    case 32u + 4u: return pk_fs_launch<2u, 4u, true>(a, s);
    case 32u + 8u: return pk_fs_launch<2u, 2u, true>(a, s);
    case 64u + 2u: return pk_fs_launch<4u, 8u, true>(a, s);
    case 64u + 4u: return pk_fs_launch<4u, 4u, true>(a, s);
    case 64u + 8u: return pk_fs_launch<4u, 2u, true>(a, s);
    }
    return hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------------------------
// RAM probes (pk_probe_eval): the program's values read from every env's RAM image, turned into a
// reward, a done flag and a feature row (include/pokegym_amd.h states the model).  Lane = env, a
// workgroup is one wave of 64 envs, and the program is walked wave-uniformly: a byte load of the
// wave reads runs of W = 1 << ilv_sh consecutive bytes of the interleaved image (pk_img_off), for
// any W.  (A four-envs-per-thread instance with dword loads was measured and not kept)
// The state words are probe-major (state[j * npad + env]), so a wave loads and stores consecutive
// words; mask, rew and term likewise.  The feature rows i32[n][m] go through LDS, PK_PROBE_CHUNK
// probes at a time: the tile's rows are padded by one word, and the wave then writes every env's
// chunk as consecutive words.  No thread reads what another writes outside the tile, and there are
// no atomics.  The barriers are reached by every thread (no early return): the host-simulation
// build runs a workgroup as 64 threads joined at them.
// The reward arithmetic must round every product and sum once: contraction is switched off here
// for both compilers, the pragma of clang in the two helpers, that of gcc around the kernel.
#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

__device__ __forceinline__ double pk_pr_mul(double a, double b) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    return a * b;
}

__device__ __forceinline__ double pk_pr_add(double a, double b) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    return a + b;
}

// (the host-simulation build joins the threads of a workgroup at barriers only for kernels launched
// under a PK_K1_KERNEL name)
#define PK_K1_KERNEL_PROBE pk_probe_kernel
__global__ void __launch_bounds__(PK_PROBE_WG) pk_probe_kernel(PkProbeArgs A) {
    constexpr u32 C = PK_PROBE_CHUNK, LD = C + 1u;
    __shared__ int32_t tile[PK_PROBE_WG * LD];
    __shared__ u8 takes[PK_PROBE_WG];
    const u32 tid = threadIdx.x, sh = A.ilv_sh;
    const u32 base = A.env0 + blockIdx.x * PK_PROBE_WG, e = base + tid;
    const bool in = e < A.env1, mk = in && A.mask && A.mask[e] != 0;
    const bool part = A.rebase_only ? in && (!A.mask || mk) : in;   // part implies e < env1: the env's
    const bool reb = A.rebase_only ? part : mk;                     // loads stay inside the images
    takes[tid] = part;
    const u8* img = A.mem + pk_img_off(part ? e : base, 0u, sh);
    double r = 0.0;
    u32 done = 0u;

    for (u32 j0 = 0; j0 < A.m; j0 += C) {
        const u32 j1 = min(j0 + C, A.m);
        for (u32 j = j0; j < j1; j++) {
            const pk_probe P = A.prog[j];
            u32 v = 0u;
            for (u32 k = 0; k < P.count; k++) {
                const u32 a = (u32)P.addr + k * (u32)P.stride;
                const u32 phys = a >= 0xFF80u ? PK_P_HRAM + (a - 0xFF80u) : PK_P_WRAM + (a & 0x1FFFu);
                const u8* p = img + ((size_t)phys << sh);
                u32 x = 0u;
                if (P.kind == PK_PV_BITS) {
#pragma unroll 8
                    for (u32 b = 0; b < P.len; b++)
                        x += (u32)__builtin_popcount(part ? (u32)p[(size_t)b << sh] : 0u);
                } else {
                    for (u32 b = 0; b < P.len; b++) {
                        const u32 byte = part ? (u32)p[(size_t)b << sh] : 0u;
                        x = P.kind == PK_PV_LE ? x | byte << (8u * b)
                          : P.kind == PK_PV_BE ? x << 8 | byte
                                               : x * 100u + (byte >> 4) * 10u + (byte & 15u);
                    }
                }
                v = P.reduce == PK_PR_MAX ? max(v, x) : v + x;
            }
            if (P.op != PK_PO_NONE && part) {
                u32* sp = A.state + (size_t)j * A.npad + e;
                const u32 s = *sp;
                u32 sn = v;
                if (!reb) {
                    double c = 0.0;
                    if (P.op == PK_PO_DELTA) {
                        c = pk_pr_mul(P.weight, (double)((int64_t)v - (int64_t)s));
                    } else if (P.op == PK_PO_NEWMAX) {
                        if (v > s) c = pk_pr_mul(P.weight, (double)(v - s));
                        sn = max(s, v);
                    } else if (v != s) {
                        c = P.weight;
                    }
                    r = pk_pr_add(r, c);
                }
                *sp = sn;
            }
            const u32 arg = P.arg;
            done |= P.cmp == PK_PC_EQ ? v == arg : P.cmp == PK_PC_NE ? v != arg
                  : P.cmp == PK_PC_GE ? v >= arg : P.cmp == PK_PC_LE ? v <= arg : 0u;
            tile[tid * LD + (j - j0)] = (int32_t)v;
        }
        if (A.feat) {
            __syncthreads();
            const u32 cols = j1 - j0;
            for (u32 q = tid; q < PK_PROBE_WG * cols; q += PK_PROBE_WG) {
                const u32 row = q / cols, c = q % cols;
                if (takes[row]) A.feat[(size_t)(base + row) * A.m + j0 + c] = tile[row * LD + c];
            }
            __syncthreads();
        }
    }
    if (part && !reb) {
        if (A.rew) A.rew[e] = A.set ? r : pk_pr_add(A.rew[e], r);
        if (A.term) A.term[e] = (u8)(A.set ? done : (A.term[e] | done));
    }
}

#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC pop_options
#endif

hipError_t pk_launch_probe(const PkProbeArgs& a, hipStream_t s) {
    const u32 count = a.env1 - a.env0;
    hipLaunchKernelGGL(PK_K1_KERNEL_PROBE, dim3((count + PK_PROBE_WG - 1u) / PK_PROBE_WG), dim3(PK_PROBE_WG), 0, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Tile view (pk_tiles_eval): the screen as 18 x 20 tile ids (or hashes of the tiles' data) and the
// object plane, from the registers, the VRAM image and the OAM image a step leaves
// (include/pokegym_amd.h states the model).  A workgroup of PK_TILES_WG threads takes PK_TILES_ENVS
// neighbouring envs; thread t works for env t % PK_TILES_ENVS on the cells t / PK_TILES_ENVS,
// + PK_TILES_SLOTS, ...  So 16 neighbouring lanes hold the 16 envs of one cell: envs in the same game
// state read 16 consecutive bytes of the interleaved image (pk_img_off; any interleave works, a
// narrower one than 16 splits the run), and the cells of a wave's four lane groups are neighbours
// in the map.  The registers come from the SoA arrays.
//   1. slot 0 of every env reads the mask byte and, if the env takes part, LCD0 / LCD1 into LDS.
//   2. every thread clears its cells' object words, stages its share of the env's 160 OAM bytes
//      (once), and computes the BG / window plane of its cells into LDS: the map bytes of all its
//      cells first, then in hash mode the 16 data bytes of each.
//   3. a thread per object takes the object's one or two cells with an LDS atomicMin of
//      X << 8 | index: the smaller X wins, then the lower index, whatever the order of the threads.
//   4. every thread turns its cells' winners into the plane's values; the key terms are XORed per
//      thread and reduced through LDS.
//   5. the view leaves as consecutive dwords: an env's planes are one run of P * 720 bytes (rows of
//      40 bytes back to back), and the envs of a workgroup follow each other.
// An env that is masked out costs its mask byte: its threads issue no other load and no store.
// Every barrier is reached by every thread (no early return), and the kernel is launched under a
// PK_K1_KERNEL_ name, so the host-simulation build joins its threads at them.  LDS rows are padded
// to an odd number of dwords.
#define PK_TILES_NC ((PK_TILE_CELLS + PK_TILES_SLOTS - 1u) / PK_TILES_SLOTS)   // cells per thread, 23
#define PK_TILES_LD0 (PK_TILE_CELLS + 2u)     // u16 per env of the BG plane's row: 181 dwords
#define PK_TILES_LD1 (PK_TILE_CELLS + 1u)     // u32 per env of the object plane's row
#define PK_TILES_OAMLD 41u                    // u32 per env of the staged OAM: 40 entries and a pad

// the hash of the 16 data bytes of tile `id` (VRAM offset id * 16), cut to `bits` bits
__device__ __forceinline__ u32 pk_tiles_hash(const u8* img, u32 sh, u32 id, u32 bits) {
    const u8* p = img + ((size_t)(PK_P_VRAM + id * 16u) << sh);
    u32 w[4];
#pragma unroll
    for (u32 j = 0; j < 4u; j++)
        w[j] = (u32)p[(size_t)(4u * j) << sh] | (u32)p[(size_t)(4u * j + 1u) << sh] << 8
             | (u32)p[(size_t)(4u * j + 2u) << sh] << 16 | (u32)p[(size_t)(4u * j + 3u) << sh] << 24;
    const u64 h = pk_arch_mix(((u64)w[0] | (u64)w[1] << 32) ^ pk_arch_mix(((u64)w[2] | (u64)w[3] << 32) + PK_CELL_GOLD));
    return (u32)h & ((1u << bits) - 1u);
}

#define PK_K1_KERNEL_TILES pk_tiles_kernel
__global__ void __launch_bounds__(PK_TILES_WG) pk_tiles_kernel(PkTilesArgs A) {
    __shared__ uint16_t bg[PK_TILES_ENVS * PK_TILES_LD0];
    __shared__ u32 obj[PK_TILES_ENVS * PK_TILES_LD1];   // X << 8 | index of the cell's winner, then its value
    __shared__ u32 oam[PK_TILES_ENVS * PK_TILES_OAMLD];
    __shared__ u64 red[PK_TILES_WG];
    __shared__ u32 lcd[2u * PK_TILES_ENVS];
    __shared__ u8 takes[PK_TILES_ENVS];
    const u32 tid = threadIdx.x, el = tid % PK_TILES_ENVS, slot = tid / PK_TILES_ENVS, sh = A.ilv_sh;
    const u32 base = A.env0 + blockIdx.x * PK_TILES_ENVS, e = base + el;
    const bool two = A.planes > 1u;

    if (slot == 0u) {
        const bool t = e < A.env1 && (!A.mask || A.mask[e] != 0);   // t implies e < env1: the env's loads
        takes[el] = t;                                              // stay inside the arrays
        lcd[el] = t ? A.regs[(size_t)PK_R_LCD0 * A.npad + e] : 0u;
        lcd[PK_TILES_ENVS + el] = t ? A.regs[(size_t)PK_R_LCD1 * A.npad + e] : 0u;
    }
    __syncthreads();
    const bool part = takes[el] != 0;
    const u32 lcdc = lcd[el] & 0xFFu, l1 = lcd[PK_TILES_ENVS + el];
    const u32 scy = l1 & 0xFFu, scx = (l1 >> 8) & 0xFFu, wy = (l1 >> 16) & 0xFFu, wx = l1 >> 24;
    const bool lcd_on = (lcdc & 0x80u) != 0, obj_on = two && part && lcd_on && (lcdc & 0x02u);
    const u8* img = A.mem + pk_img_off(part ? e : base, 0u, sh);
    u64 acc = 0;

    if (two) {
#pragma unroll
        for (u32 k = 0; k < PK_TILES_NC; k++) {
            const u32 cell = slot + k * PK_TILES_SLOTS;
            if (cell < PK_TILE_CELLS) obj[el * PK_TILES_LD1 + cell] = 0xFFFFFFFFu;
        }
        if (obj_on) {       // 160 bytes over the env's 16 threads
            u8* ob = reinterpret_cast<u8*>(oam + el * PK_TILES_OAMLD);
#pragma unroll
            for (u32 k = 0; k < 160u / PK_TILES_SLOTS; k++) {
                const u32 b = slot + k * PK_TILES_SLOTS;
                ob[b] = img[(size_t)(PK_P_OAM + b) << sh];
            }
        }
    }
    {
        const bool bg_on = part && lcd_on && (lcdc & 0x01u);
        const bool win_on = (lcdc & 0x20u) != 0 && wx <= 166u;
        u32 id[PK_TILES_NC];
#pragma unroll
        for (u32 k = 0; k < PK_TILES_NC; k++) {
            const u32 cell = slot + k * PK_TILES_SLOTS;
            id[k] = PK_TILE_NONE;
            if (!bg_on || cell >= PK_TILE_CELLS) continue;
            const u32 y = cell / PK_TILE_COLS * 8u, x = cell % PK_TILE_COLS * 8u;
            const bool win = win_on && y >= wy && x + 7u >= wx;
            const u32 row = win ? (y - wy) >> 3 : ((y + scy) & 255u) >> 3;
            const u32 col = win ? (x + 7u - wx) >> 3 : ((x + scx) & 255u) >> 3;
            const u32 map = (lcdc & (win ? 0x40u : 0x08u)) ? 0x1C00u : 0x1800u;
            const u32 t = img[(size_t)(PK_P_VRAM + map + row * 32u + col) << sh];
            id[k] = (lcdc & 0x10u) || t >= 128u ? t : 256u + t;
        }
#pragma unroll
        for (u32 k = 0; k < PK_TILES_NC; k++) {
            const u32 cell = slot + k * PK_TILES_SLOTS;
            if (cell >= PK_TILE_CELLS) continue;
            u32 v = id[k];
            if (A.bits && v != PK_TILE_NONE) v = pk_tiles_hash(img, sh, v, A.bits);
            bg[el * PK_TILES_LD0 + cell] = (uint16_t)v;
            acc ^= pk_arch_mix((u64)v + (u64)(cell + 1u) * PK_CELL_GOLD);
        }
    }
    __syncthreads();

    if (two) {
        const u32 tall = lcdc & 0x04u;
        for (u32 i = slot; i < 40u; i += PK_TILES_SLOTS) {
            if (!obj_on) continue;
            const u32 o = oam[el * PK_TILES_OAMLD + i];          // Y | X << 8 | T << 16 | attr << 24
            const int r = ((int)(o & 0xFFu) - 16 + 4) >> 3, c = ((int)((o >> 8) & 0xFFu) - 8 + 4) >> 3;
            if (c < 0 || c >= (int)PK_TILE_COLS) continue;
            const u32 claim = ((o >> 8) & 0xFFu) << 8 | i;
            u32* rowp = obj + el * PK_TILES_LD1 + c;
            if (r >= 0 && r < (int)PK_TILE_ROWS) atomicMin(rowp + r * (int)PK_TILE_COLS, claim);
            if (tall && r + 1 >= 0 && r + 1 < (int)PK_TILE_ROWS) atomicMin(rowp + (r + 1) * (int)PK_TILE_COLS, claim);
        }
        __syncthreads();
        const u32 tallv = lcdc & 0x04u;
#pragma unroll 1
        for (u32 k = 0; k < PK_TILES_NC; k++) {
            const u32 cell = slot + k * PK_TILES_SLOTS;
            if (cell >= PK_TILE_CELLS) continue;
            const u32 w = obj[el * PK_TILES_LD1 + cell];
            u32 v = PK_TILE_NONE;
            if (w != 0xFFFFFFFFu) {     // only cells of an env with obj_on are ever claimed
                const u32 o = oam[el * PK_TILES_OAMLD + (w & 0xFFu)];
                v = (o >> 16) & 0xFFu;
                if (tallv) {
                    const int r = ((int)(o & 0xFFu) - 16 + 4) >> 3;
                    const bool top = (int)(cell / PK_TILE_COLS) == r, flip = (o >> 30) & 1u;
                    v = top != flip ? v & 0xFEu : v | 1u;
                }
                if (A.bits) v = pk_tiles_hash(img, sh, v, A.bits);
            }
            obj[el * PK_TILES_LD1 + cell] = v;
            acc ^= pk_arch_mix((u64)v + (u64)(PK_TILE_CELLS + cell + 1u) * PK_CELL_GOLD);
        }
    }
    red[tid] = acc;
    __syncthreads();

    // the view: dword d of an env's P * 180; the keys: slot 0 XORs its env's 16 partial words
    const u32 per = A.planes * (PK_TILE_CELLS / 2u);
    u32* out = reinterpret_cast<u32*>(A.out);
    for (u32 q = tid; q < PK_TILES_ENVS * per; q += PK_TILES_WG) {
        const u32 row = q / per, d = q % per;
        if (!takes[row]) continue;
        u32 v;
        if (d < PK_TILE_CELLS / 2u) {
            const uint16_t* p = bg + row * PK_TILES_LD0 + 2u * d;
            v = (u32)p[0] | (u32)p[1] << 16;
        } else {
            const u32* p = obj + row * PK_TILES_LD1 + 2u * (d - PK_TILE_CELLS / 2u);
            v = p[0] | p[1] << 16;
        }
        out[(size_t)(base + row) * per + d] = v;
    }
    if (A.keys && slot == 0u && part) {
        u64 x = 0;
        for (u32 j = 0; j < PK_TILES_SLOTS; j++) x ^= red[j * PK_TILES_ENVS + el];
        const u64 salt = A.salt ? A.salt[e] : 0;
        u64 key = pk_arch_mix(salt ^ x);
        if (key == PK_ARCH_NOKEY) key = PK_ARCH_NOKEY - 1u;
        if (A.salt && salt == PK_ARCH_NOKEY) key = PK_ARCH_NOKEY;   // "no cell" passes through
        A.keys[e] = key;
    }
}

hipError_t pk_launch_tiles(const PkTilesArgs& a, hipStream_t s) {
    const u32 count = a.env1 - a.env0;
    hipLaunchKernelGGL(PK_K1_KERNEL_TILES, dim3((count + PK_TILES_ENVS - 1u) / PK_TILES_ENVS), dim3(PK_TILES_WG), 0, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Generic episode mover (pk_bank_checkpoint / pk_bank_resume on a handle without the reward stack;
// pk_layout.h PkGepArgs): the generic episode part of the envs on the range's bank list <-> their
// validated slots, shaped like pk_ep_move_kernel.  A stack row is linear on both sides, so a
// workgroup takes one listed env and PK_GEP_CHUNK 16-byte pieces of its row, consecutive lanes
// moving consecutive pieces; untouched envs are never scanned.  The workgroup of an env's first
// chunk also moves the strided words, one lane per word: the lane registers (lanes 0..19) and the
// probe state (lanes 64..64 + mpad), pad words written as 0 on a save and skipped on a load.
// Without a stack part there is one chunk per env and only that tail runs.  No LDS, no atomics, no
// barrier; rows are only read on the slot side of a resume, so many envs may name one slot.
__global__ void __launch_bounds__(256) pk_gep_move_kernel(PkGepArgs A) {
    const u32 np = A.npad, pieces = A.row16;
    const u32 chunks = pieces ? (pieces + PK_GEP_CHUNK - 1u) / PK_GEP_CHUNK : 1u;
    const u32 total = *A.cnt * chunks;
    for (u32 w = blockIdx.x; w < total; w += gridDim.x) {
        const u32 env = A.ids[w / chunks], c = w % chunks, s = (u32)A.src[env];
        if (pieces) {
            uint4* es = reinterpret_cast<uint4*>(A.stack + (size_t)env * pieces * 16u);
            uint4* bs = reinterpret_cast<uint4*>(A.g_stack + (size_t)s * pieces * 16u);
            const u32 q1 = (c + 1u) * PK_GEP_CHUNK < pieces ? (c + 1u) * PK_GEP_CHUNK : pieces;
            for (u32 q = c * PK_GEP_CHUNK + threadIdx.x; q < q1; q += blockDim.x) {
                if (A.save) bs[q] = es[q];
                else es[q] = bs[q];
            }
        }
        if (c != 0u) continue;
        const u32 t = threadIdx.x;
        if (t < PK_GEP_REGS) {
            u32* b = A.g_regs + (size_t)s * PK_GEP_REGS + t;
            u32* p = t < PK_NREGS ? A.regs + (size_t)t * np + env : nullptr;
            if (A.save) *b = p ? *p : 0u;
            else if (p) *p = *b;
        } else if (t >= 64u && t < 64u + A.mpad) {
            const u32 j = t - 64u;
            u32* b = A.g_probe + (size_t)s * A.mpad + j;
            u32* p = j < A.m ? A.state + (size_t)j * np + env : nullptr;
            if (A.save) *b = p ? *p : 0u;
            else if (p) *p = *b;
        }
    }
}

hipError_t pk_launch_gep_move(const PkGepArgs& a, hipStream_t s) {
    const u32 chunks = a.row16 ? (a.row16 + PK_GEP_CHUNK - 1u) / PK_GEP_CHUNK : 1u;
    const uint64_t items = (uint64_t)a.items * chunks;
    const u32 grid = items < 65536u ? (u32)(items ? items : 1u) : 65536u;
    hipLaunchKernelGGL(pk_gep_move_kernel, dim3(grid), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Archive exchange (pk_archive_pack / pk_archive_merge): cells as records and whole-slot payloads.

// pk_archive_pack, one workgroup: the records of cells [cell0, cell0 + count) and, by a scan in cell
// order like pk_arch_rank_kernel's, the payload rows — every cell in use (full), or the dirty ones
// (delta), numbered 0, 1, ... until max_payloads are given.  The cells that got a row are listed
// for the mover.  A delta pack also moves the sent words up to the counts and clears the dirty
// word of the cells it ships; a full pack writes nothing into the archive.
#define PK_K1_KERNEL_XCHG_PACK pk_xchg_pack_kernel
__global__ void __launch_bounds__(256) pk_xchg_pack_kernel(PkPackArgs P) {
    __shared__ u32 sums[256];
    const PkArchArgs& A = P.a;
    const u32 tid = threadIdx.x, chunk = (P.count + 255u) / 256u;
    const u32 b = tid * chunk < P.count ? tid * chunk : P.count;
    const u32 end = P.count - b < chunk ? P.count : b + chunk;
    const u32 used = (u32)A.hdr[PK_AH_USED];
    u32 s = 0;
    for (u32 i = b; i < end; i++) {
        const u32 c = P.cell0 + i;
        s += c < used && (!P.delta || A.x_dirty[c]) ? 1u : 0u;
    }
    sums[tid] = s;
    __syncthreads();
    for (u32 o = 1; o < 256u; o <<= 1) {
        const u32 v = tid >= o ? sums[tid - o] : 0u;
        __syncthreads();
        sums[tid] += v;
        __syncthreads();
    }
    u32 r = sums[tid] - s;
    for (u32 i = b; i < end; i++) {
        const u32 c = P.cell0 + i;
        pk_xrec o;
        memset(&o, 0, sizeof o);
        o.key = PK_ARCH_NOKEY;
        o.payload = -1;
        if (c < used) {
            const u32 v = A.a_visits[c], p = A.a_picks[c];
            o.key = A.a_key[c];
            o.score = A.a_score[c];
            o.length = A.a_len[c];
            o.format = A.format;
            o.visits = v;
            o.picks = p;
            bool want = true;
            if (P.delta) {
                o.visits = v - A.x_sent_visits[c];
                o.picks = p - A.x_sent_picks[c];
                A.x_sent_visits[c] = v;
                A.x_sent_picks[c] = p;
                want = A.x_dirty[c] != 0u;
            }
            if (want) {
                if (r < P.max_payloads) {
                    o.payload = (int32_t)r;
                    A.x_cell[r] = c;
                    A.x_pay[r] = r;
                    if (P.delta) A.x_dirty[c] = 0u;
                }
                r++;
            }
        }
        P.out[i] = o;
    }
    if (tid == 0) {
        const u32 n = sums[255] < P.max_payloads ? sums[255] : P.max_payloads;
        A.x_cnt[0] = n;
        if (P.n_payloads_out) *P.n_payloads_out = n;
    }
}

// The movers, slot -> payload (PACK) and payload -> slot.  A workgroup takes one listed item and a
// chunk of PK_XCHG_CHUNK 16-byte pieces of its payload; consecutive lanes move consecutive pieces
// with uint4 loads and stores on both sides (every part of a slot is linear and 16-byte aligned).
// No LDS, no atomics, no byte traffic besides the two "filled" marks of an unpacked slot.  The work
// loop runs over the device-built list: nothing scans a slot that does not move.
template <bool PACK>
__global__ void __launch_bounds__(256) pk_xchg_move_kernel(PkXchgArgs X) {
    const u32 chunks = (X.pay16 + PK_XCHG_CHUNK - 1u) / PK_XCHG_CHUNK;
    const u32 total = X.cnt[0] * chunks;
    for (u32 w = blockIdx.x; w < total; w += gridDim.x) {
        const u32 k = w / chunks, q0 = (w - k * chunks) * PK_XCHG_CHUNK;
        const u32 q1 = X.pay16 - q0 < PK_XCHG_CHUNK ? X.pay16 : q0 + PK_XCHG_CHUNK;
        const u32 slot = X.slot0 + X.cell[k];
        uint4* pp = reinterpret_cast<uint4*>(X.payload + (size_t)X.pay[k] * X.pay16 * 16u);
        for (u32 q = q0 + threadIdx.x; q < q1; q += blockDim.x) {
            if (q == X.head16) {
                if (PACK) {
                    pp[q] = make_uint4((u32)X.bt_origin[slot], X.bt_flags[slot], 0u, 0u);
                } else {
                    const uint4 v = pp[q];
                    X.bt_origin[slot] = (int32_t)v.x;
                    X.bt_flags[slot] = v.y;
                }
                continue;
            }
            u8* base = X.base[0];
            u32 stride = X.stride[0], off = 0;
#pragma unroll
            for (u32 p = 1; p < PK_XCHG_MAX_PARTS; p++)
                if (p < X.nparts && q >= X.off16[p]) {
                    base = X.base[p];
                    stride = X.stride[p];
                    off = X.off16[p];
                }
            uint4* sp = reinterpret_cast<uint4*>(base + (size_t)slot * stride) + (q - off);
            if (PACK) pp[q] = *sp;
            else *sp = pp[q];
        }
        if (!PACK && q0 == 0u && threadIdx.x == 0u) {
            X.b_filled[slot] = 1;
            X.b_ep_filled[slot] = 1;
        }
    }
}

hipError_t pk_launch_xchg_pack(const PkPackArgs& p, hipStream_t s) {
    hipLaunchKernelGGL(PK_K1_KERNEL_XCHG_PACK, dim3(1), dim3(256), 0, s, p);
    return hipGetLastError();
}

// move the listed payloads (x.cnt): pack = slot -> payload, else payload -> slot
hipError_t pk_launch_xchg_move(const PkXchgArgs& x, bool pack, hipStream_t s) {
    const uint64_t items = (uint64_t)x.items * ((x.pay16 + PK_XCHG_CHUNK - 1u) / PK_XCHG_CHUNK);
    const u32 grid = items < 8192u ? (u32)items : 8192u;
    if (!grid) return hipSuccess;   // no payload can move (max_payloads or n_payloads is 0)
    if (pack) hipLaunchKernelGGL((pk_xchg_move_kernel<true>), dim3(grid), dim3(256), 0, s, x);
    else hipLaunchKernelGGL((pk_xchg_move_kernel<false>), dim3(grid), dim3(256), 0, s, x);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Visit counts (pk_counts_*): a persistent table key -> count, counted into by every env of a range
// and read back as the count-based bonus beta / sqrt(count) (include/pokegym_amd.h states the
// model).  Sums and a 64-bit compare-and-swap on the key word only: nothing depends on the order of
// threads.  Whether a call may insert is decided by one word no thread of the call writes (USED, the
// keys stored when the call started), so a full table admits all new keys of a call or none; the
// keys a call inserts are counted aside (NEW) and the commit that ends the call adds them up.  The
// table is never more than three quarters full, so a probe loop ends at an empty entry.

// one atomic per wave for a count every lane may add 1 to; every lane of the wave calls it
__device__ static inline void pk_cnt_tally(bool mine, u64* word) {
    const u64 m = __builtin_amdgcn_ballot_w64(mine);
    if (m && pk_lane() == (u32)__builtin_ffsll((long long)m) - 1u)
        atomicAdd(reinterpret_cast<ull*>(word), (ull)__builtin_popcountll(m));
}

// A key word as other threads may be swapping it in.  A key word only ever goes from empty to its
// final key, so a plain load is enough on the device: a stale "empty" leads to the compare-and-swap,
// which returns the truth, and any other value is final.  The host simulation runs workgroups on
// concurrent host threads, where the same read has to be an atomic load to be defined at all.
__device__ static inline u64 pk_cnt_peek(const ull* p) {
#ifndef __HIPCC__
    return __atomic_load_n(p, __ATOMIC_RELAXED);
#else
    return *p;
#endif
}

// The entry of key: found, or — in a call that may insert — claimed by a compare-and-swap on the
// first empty entry of its probe sequence (made = this thread's swap made it).  PK_ARCH_NONE when
// the key is absent and stays so.
__device__ static inline u32 pk_cnt_find(const PkCountArgs& A, u64 key, bool insert, bool& made) {
    u32 pos = (u32)pk_arch_mix(key) & A.c_mask;
    for (u32 p = 0; p <= A.c_mask; p++, pos = (pos + 1u) & A.c_mask) {
        ull* ck = reinterpret_cast<ull*>(A.c_key + pos);
        u64 k = pk_cnt_peek(ck);
        if (k == PK_ARCH_NOKEY) {
            if (!insert) return PK_ARCH_NONE;
            k = atomicCAS(ck, (ull)PK_ARCH_NOKEY, (ull)key);
            if (k == PK_ARCH_NOKEY) {
                made = true;
                return pos;
            }
        }
        if (k == key) return pos;
    }
    return PK_ARCH_NONE;
}

#ifndef PK_CNT_PRE
#define PK_CNT_PRE PK_ARCH_PRE   // rounds of the wave pre-reduction (0: every lane adds alone, tools/measure_counts.py)
#endif
// launch one of pk_counts_update, thread = env: find or insert the key's entry, leave it in tgt, and
// count the env.  The lanes of a wave that hold one entry add their number with one atomic (the
// rounds of pk_arch_group; all 65,536 envs of a title screen hold one); a peek only finds.
__global__ void __launch_bounds__(256) pk_cnt_claim_kernel(PkCountArgs A) {
    const u32 e = A.env0 + blockIdx.x * blockDim.x + threadIdx.x;
    const bool open = A.hdr[PK_CH_USED] + (A.env1 - A.env0) <= A.limit;
    u32 t = PK_ARCH_NONE;
    bool part = false, made = false;
    if (e < A.env1 && (!A.mask || A.mask[e])) {
        const u64 key = A.keys[e];
        part = key != PK_ARCH_NOKEY;
        if (part) t = pk_cnt_find(A, key, open && !A.peek, made);
    }
    if (e < A.env1) A.tgt[e] = t;
    if (A.peek) return;
    pk_cnt_tally(made, A.hdr + PK_CH_NEW);
    pk_cnt_tally(part && t == PK_ARCH_NONE, A.hdr + PK_CH_OVERFLOW);
    bool todo = t != PK_ARCH_NONE, match, lead;
    u64 mm;
    for (u32 it = 0; it <= PK_CNT_PRE; it++) {
        u32 n = 1;
        if (it < PK_CNT_PRE) {   // a group per round; after the last round every lane goes alone
            if (!pk_arch_group(todo, t, match, lead, mm)) break;
            n = (u32)__builtin_popcountll(mm);
        } else {
            match = lead = todo;
        }
        if (lead && match) atomicAdd(reinterpret_cast<ull*>(A.c_cnt + t), (ull)n);
        todo = todo && !match;
    }
}

// launch two, thread = env: the count of the env's entry and the bonus; the first thread commits
// the call's new keys to USED
__global__ void __launch_bounds__(256) pk_cnt_bonus_kernel(PkCountArgs A) {
    const u32 e = A.env0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (e == A.env0 && !A.peek) {
        A.hdr[PK_CH_USED] += A.hdr[PK_CH_NEW];
        A.hdr[PK_CH_NEW] = 0;
    }
    if (e >= A.env1) return;
    const u32 t = A.tgt[e];
    const u64 c = t != PK_ARCH_NONE ? A.c_cnt[t] : 0;
    if (A.counts_out) A.counts_out[e] = c;
    if (A.bonus_out) A.bonus_out[e] = c ? A.beta / sqrt((double)c) : 0.0;
}

// pk_counts_add, thread = record: launch one of an update with records as items, each adding its own
// count (to the sent word as well when the counts are foreign).  Records seldom share a key, so
// only the two tallies are reduced per wave.
__global__ void __launch_bounds__(256) pk_cnt_add_kernel(PkCountArgs A) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool open = A.hdr[PK_CH_USED] + A.env1 <= A.limit;
    u32 t = PK_ARCH_NONE;
    u64 c = 0;
    bool part = false, made = false;
    if (i < A.env1) {
        const uint4 w = reinterpret_cast<const uint4*>(A.rec)[i];
        const u64 key = w.x | (u64)w.y << 32;
        c = w.z | (u64)w.w << 32;
        part = key != PK_ARCH_NOKEY && c != 0;
        if (part) t = pk_cnt_find(A, key, open, made);
    }
    pk_cnt_tally(made, A.hdr + PK_CH_NEW);
    pk_cnt_tally(part && t == PK_ARCH_NONE, A.hdr + PK_CH_OVERFLOW);
    if (t == PK_ARCH_NONE) return;
    atomicAdd(reinterpret_cast<ull*>(A.c_cnt + t), (ull)c);
    if (A.foreign) atomicAdd(reinterpret_cast<ull*>(A.c_sent + t), (ull)c);
}

// the commit that ends a pk_counts_add
__global__ void pk_cnt_commit_kernel(PkCountArgs A) {
    A.hdr[PK_CH_USED] += A.hdr[PK_CH_NEW];
    A.hdr[PK_CH_NEW] = 0;
}

// pk_counts_pack: a record per stored key whose packed count is not zero, appended in no order.  A
// workgroup takes chunks of 256 * PK_CNT_PACK_ITEMS entries, consecutive lanes consecutive entries;
// every thread keeps its records in registers, a scan through LDS numbers the workgroup's records
// and one atomic takes its rows: 2^22 entries are 2,048 atomics on the caller's word (one per wave
// was 65,536 returning atomics on one address, and the whole of the call's time).  A delta pack moves
// sent up to the count.
#define PK_CNT_PACK_ITEMS 8u
#define PK_K1_KERNEL_CNT_PACK pk_cnt_pack_kernel
__global__ void __launch_bounds__(256) pk_cnt_pack_kernel(PkCountArgs A) {
    __shared__ u32 sums[256];
    __shared__ u32 first;
    const u64 cap = (u64)A.c_mask + 1u;
    const u32 tid = threadIdx.x, per = 256u * PK_CNT_PACK_ITEMS;
    const u32 nchunks = (u32)((cap + per - 1u) / per);
    for (u32 ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        u64 key[PK_CNT_PACK_ITEMS], v[PK_CNT_PACK_ITEMS];
        u32 mine = 0;
#pragma unroll
        for (u32 j = 0; j < PK_CNT_PACK_ITEMS; j++) {
            const u64 p = (u64)ch * per + j * 256u + tid;
            key[j] = p < cap ? A.c_key[p] : PK_ARCH_NOKEY;
        }
#pragma unroll
        for (u32 j = 0; j < PK_CNT_PACK_ITEMS; j++) {
            const u64 p = (u64)ch * per + j * 256u + tid;
            v[j] = 0;
            if (key[j] != PK_ARCH_NOKEY) {
                const u64 c = A.c_cnt[p];
                v[j] = c;
                if (A.delta) {
                    v[j] = c - A.c_sent[p];
                    if (v[j]) A.c_sent[p] = c;
                }
            }
            mine += v[j] ? 1u : 0u;
        }
        sums[tid] = mine;
        __syncthreads();
        for (u32 o = 1; o < 256u; o <<= 1) {
            const u32 x = tid >= o ? sums[tid - o] : 0u;
            __syncthreads();
            sums[tid] += x;
            __syncthreads();
        }
        if (tid == 255u) first = sums[255] ? atomicAdd(A.n_out, sums[255]) : 0u;
        __syncthreads();
        u64 row = (u64)first + sums[tid] - mine;
#pragma unroll
        for (u32 j = 0; j < PK_CNT_PACK_ITEMS; j++) {
            if (!v[j]) continue;
            if (row < A.max_records)
                reinterpret_cast<uint4*>(A.pack)[row] =
                    make_uint4((u32)key[j], (u32)(key[j] >> 32), (u32)v[j], (u32)(v[j] >> 32));
            row++;
        }
        __syncthreads();   // sums and first are the next chunk's
    }
}

static inline dim3 pk_cnt_grid(uint64_t items) { return dim3((u32)((items + 255u) / 256u)); }

hipError_t pk_launch_cnt_update(const PkCountArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(pk_cnt_claim_kernel, pk_cnt_grid(a.env1 - a.env0), dim3(256), 0, s, a);
    hipLaunchKernelGGL(pk_cnt_bonus_kernel, pk_cnt_grid(a.env1 - a.env0), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t pk_launch_cnt_add(const PkCountArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(pk_cnt_add_kernel, pk_cnt_grid(a.env1), dim3(256), 0, s, a);
    hipLaunchKernelGGL(pk_cnt_commit_kernel, dim3(1), dim3(1), 0, s, a);
    return hipGetLastError();
}

hipError_t pk_launch_cnt_pack(const PkCountArgs& a, hipStream_t s) {
    const uint64_t per = 256u * PK_CNT_PACK_ITEMS, chunks = ((uint64_t)a.c_mask + per) / per;
    hipLaunchKernelGGL(PK_K1_KERNEL_CNT_PACK, dim3(chunks < 8192u ? (u32)chunks : 8192u), dim3(256), 0, s, a);
    return hipGetLastError();
}
