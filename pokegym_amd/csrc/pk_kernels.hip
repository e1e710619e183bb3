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
#include <stdint.h>

#include "pk_layout.h"
#include "pk_render.h"

// ---------------------------------------------------------------------------------------------
// K2: rasterise the latched lines of the rendered frame.  One wave = one (group, scanline),
// lane = env: the 64 lanes read the same VRAM offsets of their interleaved images (coalesced).
__global__ void __launch_bounds__(64) pk_render_kernel(PkStepArgs A) {
    const u32 y = blockIdx.x % PK_ROWS;
    const u32 gid = A.env0 / PK_LANES + blockIdx.x / PK_ROWS;
    const u32 lane = threadIdx.x;
    const u32 env = gid * PK_LANES + lane;
    if (env >= A.env1) return;
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
    const Mem m = mem_view(A.mem, env, A.ilv_sh);
    render_line(m, y, A.lat[idx], A.lat[A.lat_stride + idx], (int)(l2 & 0xFFu) - 1, out);
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
hipError_t pk_launch_render(const PkStepArgs& a, hipStream_t s) {
    const u32 grid = ((a.env1 - a.env0 + PK_LANES - 1u) / PK_LANES) * PK_ROWS;
    hipLaunchKernelGGL(pk_render_kernel, dim3(grid), dim3(PK_LANES), 0, s, a);
    return hipGetLastError();
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
