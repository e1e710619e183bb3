// pk_capi.cpp — the C ABI (include/pokegym_amd.h) over the HIP kernels in pk_kernels.hip.
//
// Owns the per-GPU device state: lane-interleaved RAM images, SoA lane registers, per-line
// render latches, the persistent grey screen, the ROM and the decode table, plus a parsed copy
// of the template savestate used by pk_reset.  Savestate import/export restates the PyBoy v9
// layout pinned on the reference's 264 savestates (oracle/gbcore.c load/save).
#include <hip/hip_runtime.h>

#include <errno.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/pokegym_amd.h"
#include "pk_ucode.h"
#include "pk_layout.h"
#include "pk_reward.h"

hipError_t pk_launch_step(const PkStepArgs& a, hipStream_t s);
hipError_t pk_launch_step_small(const PkStepArgs& a, hipStream_t s);   // pk_step.hip built with PK_K1_SMALL
hipError_t pk_launch_render(const PkStepArgs& a, hipStream_t s);
hipError_t pk_launch_render_done(const PkStepArgs& a, const PkDoneArgs& d, hipStream_t s);
hipError_t pk_launch_reset(const PkResetArgs& a, hipStream_t s);
hipError_t pk_launch_list(const uint8_t* mask, uint32_t env0, uint32_t env1, uint32_t* cnt, uint32_t* ids, hipStream_t s);
hipError_t pk_launch_render_latched(const PkStepArgs& a, hipStream_t s);
hipError_t pk_launch_gather_env(const uint8_t* mem, uint32_t env, uint32_t sh, uint8_t* out, hipStream_t s);
hipError_t pk_launch_gather_range(const uint8_t* mem, uint32_t env0, uint32_t count, uint32_t sh, uint8_t* out, hipStream_t s);
hipError_t pk_launch_scatter_env(uint8_t* mem, uint32_t env, uint32_t sh, const uint8_t* in, hipStream_t s);
hipError_t pk_launch_done(const uint32_t* time_reg, uint32_t n, uint32_t max_steps, uint8_t* term,
                          uint8_t* trunc, double* rew, hipStream_t s);
hipError_t pk_launch_reward(const PkRewardArgs& a, hipStream_t s);
hipError_t pk_launch_rreset_pre(const PkRewardArgs& a, hipStream_t s);
hipError_t pk_launch_rreset_post(const PkRewardArgs& a, hipStream_t s);
hipError_t pk_launch_obs(const PkRewardArgs& a, hipStream_t s);
hipError_t pk_launch_seen_rehash(const uint32_t* old_tab, uint32_t old_lg, uint32_t* new_tab, uint32_t new_lg,
                                 const uint32_t* rs, uint32_t n, uint32_t np, hipStream_t s);
hipError_t pk_launch_ram_copy(uint8_t* mem, uint8_t* dense, uint32_t n, uint32_t sh, uint32_t phys0, uint32_t len,
                              uint32_t to_dense, hipStream_t s);
hipError_t pk_launch_bank_list(const PkBankArgs& a, hipStream_t s);
hipError_t pk_launch_bank_copy(const PkBankArgs& a, hipStream_t s);
hipError_t pk_launch_ep_move(const PkEpArgs& a, hipStream_t s);
hipError_t pk_launch_arch_update(const PkArchArgs& a, hipStream_t s);
hipError_t pk_launch_arch_draw(const PkArchArgs& a, hipStream_t s);
hipError_t pk_launch_arch_merge(const PkArchArgs& a, hipStream_t s);
hipError_t pk_launch_xchg_pack(const PkPackArgs& p, hipStream_t s);
hipError_t pk_launch_xchg_move(const PkXchgArgs& x, bool pack, hipStream_t s);
hipError_t pk_launch_arch_out(const PkArchArgs& a, hipStream_t s);
hipError_t pk_launch_cell_keys(const uint8_t* mem, uint32_t sh, uint32_t shift, uint64_t* keys, uint32_t env0,
                               uint32_t env1, hipStream_t s);
hipError_t pk_launch_frame_keys(const PkCellArgs& a, hipStream_t s);
hipError_t pk_launch_fstack(const PkStackArgs& a, hipStream_t s);
hipError_t pk_launch_probe(const PkProbeArgs& a, hipStream_t s);
hipError_t pk_launch_tiles(const PkTilesArgs& a, hipStream_t s);
hipError_t pk_launch_gep_move(const PkGepArgs& a, hipStream_t s);
hipError_t pk_launch_cnt_update(const PkCountArgs& a, hipStream_t s);
hipError_t pk_launch_cnt_add(const PkCountArgs& a, hipStream_t s);
hipError_t pk_launch_cnt_pack(const PkCountArgs& a, hipStream_t s);
hipError_t pk_launch_traj_record(const PkTrajArgs& a, hipStream_t s);
hipError_t pk_launch_traj_reset(const PkTrajArgs& a, hipStream_t s);
hipError_t pk_launch_traj_mark(const PkTrajArgs& a, hipStream_t s);
hipError_t pk_launch_traj_move(const PkTrajArgs& a, hipStream_t s);
hipError_t pk_launch_traj_get(const PkTrajArgs& a, hipStream_t s);

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIPCHK(expr)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) return fail(-EIO, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// v9 savestate offsets
constexpr size_t S_VER = 0, S_HDR = 1, S_CPU = 5, S_VRAM = 23, S_OAM = 8215, S_LCDREG = 8375,
                 S_LCDX = 8386, S_CLOCK = 8388, S_TARGET = 8396, S_NEXTMODE = 8404,
                 S_SCAN = 8405, S_SCREEN = 9125, S_WRAM = 101285, S_FEA0 = 109477,
                 S_IO = 109573, S_HRAM = 109649, S_FF4C = 109776, S_TIMER = 109828,
                 S_MBC = 109836, S_SRAM = 109842, S_SIZE = 142610;

struct Template {
    uint32_t regs[PK_NREGS];
    std::vector<uint8_t> mem;       // PK_PHYS
    uint32_t lat[3 * PK_ROWS];
    std::vector<uint8_t> screen;    // 144*160 grey
    uint8_t hdr[4];
    uint8_t lcdx[2];
};

uint64_t rd64(const uint8_t* p) {
    uint64_t v = 0;
    for (int i = 7; i >= 0; i--) v = (v << 8) | p[i];
    return v;
}
void wr64(uint8_t* p, uint64_t v) {
    for (int i = 0; i < 8; i++) { p[i] = (uint8_t)v; v >>= 8; }
}

int parse_v9(const uint8_t* s, size_t len, Template& t) {
    if (len != S_SIZE || s[S_VER] != 9) return fail(-EINVAL, "not a PyBoy v9 savestate (len %zu)", len);
    uint64_t clock = rd64(s + S_CLOCK), target = rd64(s + S_TARGET);
    if (clock > 0xFFFFFFFFull || target > 0xFFFFFFFFull) return fail(-EINVAL, "LCD clock out of range");
    memset(t.regs, 0, sizeof t.regs);
    const uint8_t* c = s + S_CPU;  // A F B C D E HL SP PC ime halted stopped IE queued IF
    t.regs[PK_R_W0] = c[3] | (c[2] << 8) | (c[5] << 16) | ((uint32_t)c[4] << 24);
    t.regs[PK_R_W1] = c[6] | (c[7] << 8) | (c[0] << 16) | ((uint32_t)c[1] << 24);
    t.regs[PK_R_SP] = c[8] | (c[9] << 8);
    t.regs[PK_R_PC] = c[10] | (c[11] << 8);
    t.regs[PK_R_CPU] = (c[12] ? 1u : 0u) | (c[13] ? 2u : 0u) | (c[16] ? 4u : 0u) | (c[14] ? 16u : 0u) |
                       ((uint32_t)c[15] << 8) | ((uint32_t)c[17] << 16);
    t.regs[PK_R_CLOCK] = (uint32_t)clock;
    t.regs[PK_R_TARGET] = (uint32_t)target;
    const uint8_t* r = s + S_LCDREG;  // LCDC BGP OBP0 OBP1 STAT LY LYC SCY SCX WY WX
    t.regs[PK_R_LCD0] = r[0] | (r[4] << 8) | (r[5] << 16) | ((uint32_t)r[6] << 24);
    t.regs[PK_R_LCD1] = r[7] | (r[8] << 8) | (r[9] << 16) | ((uint32_t)r[10] << 24);
    t.regs[PK_R_LCD2] = r[1] | (r[2] << 8) | (r[3] << 16) | ((uint32_t)s[S_NEXTMODE] << 24);
    const uint8_t* tm = s + S_TIMER;  // DIV TIMA DIVc(le16) TIMAc(le16) TMA TAC
    t.regs[PK_R_TIM0] = tm[0] | (tm[1] << 8) | (tm[6] << 16) | ((uint32_t)tm[7] << 24);
    t.regs[PK_R_TIM1] = (tm[2] | (tm[3] << 8)) | ((uint32_t)(tm[4] | (tm[5] << 8)) << 16);
    const uint8_t* mb = s + S_MBC;
    t.regs[PK_R_MBC] = mb[0] | (mb[1] << 8) | (mb[2] << 16) | ((uint32_t)mb[3] << 24);
    t.regs[PK_R_MISC] = 0x0Fu | (0x0Fu << 8);  // no button held, ly_window = -1
    t.mem.assign(PK_PHYS, 0);
    memcpy(&t.mem[PK_P_VRAM], s + S_VRAM, 8192);
    memcpy(&t.mem[PK_P_WRAM], s + S_WRAM, 8192);
    memcpy(&t.mem[PK_P_OAM], s + S_OAM, 160);
    memcpy(&t.mem[PK_P_OAM + 0xA0], s + S_FEA0, 96);
    memcpy(&t.mem[PK_P_IO], s + S_IO, 76);
    memcpy(&t.mem[PK_P_IO + 0x4C], s + S_FF4C, 52);
    memcpy(&t.mem[PK_P_HRAM], s + S_HRAM, 127);
    memcpy(&t.mem[PK_P_SRAM], s + S_SRAM, 4 * 8192);
    t.screen.resize(PK_SCREEN);
    for (size_t i = 0; i < PK_SCREEN; i++) t.screen[i] = s[S_SCREEN + i * 4 + 1];
    for (uint32_t y = 0; y < PK_ROWS; y++) {
        const uint8_t* p = s + S_SCAN + y * 5;  // SCX SCY WX WY tiledata_select
        uint32_t lcdc = (r[0] & ~0x10u) | ((p[4] & 1u) << 4);
        t.lat[y] = lcdc | (p[0] << 8) | (p[1] << 16) | ((uint32_t)p[2] << 24);
        t.lat[PK_ROWS + y] = p[3] | (r[1] << 8) | (r[2] << 16) | ((uint32_t)r[3] << 24);
        t.lat[2 * PK_ROWS + y] = 0;
    }
    memcpy(t.hdr, s + S_HDR, 4);
    t.lcdx[0] = s[S_LCDX];
    t.lcdx[1] = s[S_LCDX + 1];
    return 0;
}

void power_on(Template& t) {
    // our own post-boot DMG state (PyBoy would execute its bundled boot ROM instead);
    // identical to oracle/gbcore.c gb_power_on
    memset(t.regs, 0, sizeof t.regs);
    t.regs[PK_R_W0] = 0x13 | (0x00 << 8) | (0xD8 << 16) | (0x00u << 24);
    t.regs[PK_R_W1] = 0x4D | (0x01 << 8) | (0x01 << 16) | (0xB0u << 24);
    t.regs[PK_R_SP] = 0xFFFE;
    t.regs[PK_R_PC] = 0x0100;
    t.regs[PK_R_CPU] = 0;
    t.regs[PK_R_CLOCK] = 0;
    t.regs[PK_R_TARGET] = 80;
    t.regs[PK_R_LCD0] = 0x91 | (0x82 << 8);
    t.regs[PK_R_LCD1] = 0;
    t.regs[PK_R_LCD2] = 0xFC | (0xFF << 8) | (0xFF << 16) | (3u << 24);
    t.regs[PK_R_TIM0] = 0xAB;
    t.regs[PK_R_TIM1] = 0;
    t.regs[PK_R_MBC] = 1;
    t.regs[PK_R_MISC] = 0x0Fu | (0x0Fu << 8);
    t.mem.assign(PK_PHYS, 0);
    t.mem[PK_P_IO] = 0xCF;
    t.screen.assign(PK_SCREEN, 0xFF);  // shade 0
    for (uint32_t y = 0; y < PK_ROWS; y++) {
        t.lat[y] = 0;
        t.lat[PK_ROWS + y] = 0;
        t.lat[2 * PK_ROWS + y] = 0;
    }
    memset(t.hdr, 0, 4);
    t.lcdx[0] = t.lcdx[1] = 0;
}

uint8_t grey_to_flag(uint8_t g) { return g == 0xFF ? 1 : 0; }

void export_v9(const Template& tp, const uint32_t* regs, const uint8_t* mem, const uint32_t* lat,
               const uint8_t* screen, uint8_t* s) {
    memset(s, 0, S_SIZE);
    s[S_VER] = 9;
    memcpy(s + S_HDR, tp.hdr, 4);
    uint32_t w0 = regs[PK_R_W0], w1 = regs[PK_R_W1];
    uint8_t* c = s + S_CPU;
    c[0] = (w1 >> 16) & 0xFF; c[1] = (w1 >> 24) & 0xFF;  // A F
    c[2] = (w0 >> 8) & 0xFF; c[3] = w0 & 0xFF;            // B C
    c[4] = (w0 >> 24) & 0xFF; c[5] = (w0 >> 16) & 0xFF;   // D E
    c[6] = w1 & 0xFF; c[7] = (w1 >> 8) & 0xFF;            // HL
    c[8] = regs[PK_R_SP] & 0xFF; c[9] = (regs[PK_R_SP] >> 8) & 0xFF;
    c[10] = regs[PK_R_PC] & 0xFF; c[11] = (regs[PK_R_PC] >> 8) & 0xFF;
    uint32_t cpu = regs[PK_R_CPU];
    c[12] = cpu & 1; c[13] = (cpu >> 1) & 1; c[14] = (cpu >> 4) & 1;
    c[15] = (cpu >> 8) & 0xFF; c[16] = (cpu >> 2) & 1; c[17] = (cpu >> 16) & 0xFF;
    memcpy(s + S_VRAM, mem + PK_P_VRAM, 8192);
    memcpy(s + S_OAM, mem + PK_P_OAM, 160);
    uint32_t l0 = regs[PK_R_LCD0], l1 = regs[PK_R_LCD1], l2 = regs[PK_R_LCD2];
    uint8_t* r = s + S_LCDREG;
    r[0] = l0 & 0xFF; r[1] = l2 & 0xFF; r[2] = (l2 >> 8) & 0xFF; r[3] = (l2 >> 16) & 0xFF;
    r[4] = (l0 >> 8) & 0xFF; r[5] = (l0 >> 16) & 0xFF; r[6] = (l0 >> 24) & 0xFF;
    r[7] = l1 & 0xFF; r[8] = (l1 >> 8) & 0xFF; r[9] = (l1 >> 16) & 0xFF; r[10] = (l1 >> 24) & 0xFF;
    s[S_LCDX] = tp.lcdx[0];
    s[S_LCDX + 1] = tp.lcdx[1];
    wr64(s + S_CLOCK, regs[PK_R_CLOCK]);
    wr64(s + S_TARGET, regs[PK_R_TARGET]);
    s[S_NEXTMODE] = (l2 >> 24) & 0xFF;
    for (uint32_t y = 0; y < PK_ROWS; y++) {
        uint32_t a = lat[y], b = lat[PK_ROWS + y];
        uint8_t* p = s + S_SCAN + y * 5;
        p[0] = (a >> 8) & 0xFF; p[1] = (a >> 16) & 0xFF; p[2] = (a >> 24) & 0xFF; p[3] = b & 0xFF;
        p[4] = (a >> 4) & 1;
    }
    for (size_t i = 0; i < PK_SCREEN; i++) {
        uint8_t g = screen[i];
        s[S_SCREEN + i * 4 + 0] = grey_to_flag(g);
        s[S_SCREEN + i * 4 + 1] = s[S_SCREEN + i * 4 + 2] = s[S_SCREEN + i * 4 + 3] = g;
    }
    memcpy(s + S_WRAM, mem + PK_P_WRAM, 8192);
    memcpy(s + S_FEA0, mem + PK_P_OAM + 0xA0, 96);
    memcpy(s + S_IO, mem + PK_P_IO, 76);
    memcpy(s + S_HRAM, mem + PK_P_HRAM, 127);   // 0xFF80-0xFFFE: never phys 0x41FF (PK_P_UNUSED, K1's dummy store)
    memcpy(s + S_FF4C, mem + PK_P_IO + 0x4C, 52);
    uint32_t t0 = regs[PK_R_TIM0], t1 = regs[PK_R_TIM1];
    uint8_t* tm = s + S_TIMER;
    tm[0] = t0 & 0xFF; tm[1] = (t0 >> 8) & 0xFF;
    tm[2] = t1 & 0xFF; tm[3] = (t1 >> 8) & 0xFF; tm[4] = (t1 >> 16) & 0xFF; tm[5] = (t1 >> 24) & 0xFF;
    tm[6] = (t0 >> 16) & 0xFF; tm[7] = (t0 >> 24) & 0xFF;
    uint32_t mbc = regs[PK_R_MBC];
    uint8_t* m = s + S_MBC;
    m[0] = mbc & 0xFF; m[1] = (mbc >> 8) & 0xFF; m[2] = (mbc >> 16) & 0xFF; m[3] = (mbc >> 24) & 0xFF;
    memcpy(s + S_SRAM, mem + PK_P_SRAM, 4 * 8192);
}

}  // namespace

struct pk_handle {
    int device = 0;
    uint32_t n = 0, npad = 0, ngroups = 0;
    uint32_t wave_lanes = 0;   // envs per wave in K1: 0 = by launch size (k1_wave_lanes), else PK_WAVE_LANES
    uint32_t simds = 1024;     // SIMDs of the device (4 per CU)
    uint32_t k1_block = 0;     // K1 workgroup size override (PK_K1_BLOCK), 0 = by geometry
    uint32_t ilv_sh = 6;       // RAM image interleave 1 << ilv_sh (pk_layout.h pk_img_off): K1's envs per wave
    int k1_prio = -1;          // K1 wave-priority variant override (PK_K1_PRIO 0/1), -1 = by shape
    uint32_t frames = 24, release = 8, flags = 0, max_steps = 20480;
    uint32_t mbc = 3, bank_mask = 0;
    uint8_t* mem = nullptr;
    uint32_t* regs = nullptr;
    uint32_t* lat = nullptr;
    uint8_t* screen = nullptr;
    uint8_t* rom = nullptr;
    uint32_t* ucode = nullptr;  // microcode table (pk_ucode.h)
    uint8_t* t_mem = nullptr;
    uint32_t* t_regs = nullptr;
    uint32_t* t_lat = nullptr;
    uint8_t* t_screen = nullptr;
    uint8_t* scratch = nullptr;  // PK_PHYS staging for one env
    int8_t* bank_slot = nullptr;  // [128] LDS slot per ROM bank (-1 = global)
    uint8_t* slot_bank = nullptr; // [PK_LDS_SLOTS]
    uint32_t nslots = 1;
    // the small-LDS K1 (pk_layout.h): its own slot tables (PK_SMALL_LDS_SLOTS banks)
    int8_t* bank_slot_s = nullptr;
    uint8_t* slot_bank_s = nullptr;
    uint32_t nslots_s = 1;
    int k1_small = -1;         // PK_K1_SMALL: -1 = for concurrent sub-batch ranges (<= 32 envs per wave), 0 never, 1 always
    size_t lat_stride = 0;
    Template tmpl;
    // reward stack (PK_F_REWARD), see pk_reward.h
    uint32_t* rs = nullptr;
    double* rsd = nullptr;
    uint32_t* seen = nullptr;
    uint32_t* mask = nullptr;
    uint32_t* cutc = nullptr;
    uint8_t* obs = nullptr;
    uint8_t* reload = nullptr;
    // reset lists (pk_list_kernel): [0] reload count, [1] obs count, then npad reload ids, npad obs ids
    uint32_t* lists = nullptr;
    unsigned long long* dbg = nullptr;  // K1 phase-cycle counters of a -DPK_STAMP build
    double* info = nullptr;       // [PK_INFO_NFIELDS][npad]
    uint8_t* info_flag = nullptr; // [npad]
    int32_t* heat = nullptr;      // [npad][444 * 436] (PK_F_HEATMAP)
    uint32_t* info_bits = nullptr; // [PK_INFO_BITS_WORDS][npad]
    uint32_t cap_log2 = 0;
    double reward_scale = 4.0;
    // savestate bank (pk_bank_create; pk_layout.h PkBankArgs): the slots, then the per-range lists
    // [2 * ngroups] counters (envs, sub-blocks), [npad] env ids, [npad] sub-block ids, and the
    // validated slot of every env
    uint32_t bank_n = 0;
    uint8_t* b_mem = nullptr;
    uint32_t* b_regs = nullptr;
    uint32_t* b_lat = nullptr;
    uint8_t* b_screen = nullptr;
    uint8_t* b_filled = nullptr;
    uint32_t* b_rejects = nullptr;
    uint32_t* b_lists = nullptr;
    int32_t* b_src = nullptr;
    // episode parts of the slots (pk_bank_enable_episodes; pk_reward.h PkEpArgs), null without them
    uint32_t* e_fields = nullptr;
    uint32_t* e_seen = nullptr;
    uint32_t* e_mask = nullptr;
    uint32_t* e_cutc = nullptr;
    uint8_t* b_ep_filled = nullptr;
    // generic episode parts of the slots (pk_bank_enable_generic_episodes; pk_layout.h PkGepArgs), on a
    // handle without the reward stack: gep_parts = the parts asked for | 0x80000000 once enabled, the
    // raw registers, and the probe words and stack rows where asked for.  b_ep_filled is the flag array
    // of these parts too, so the bank list's validation and the archive work unchanged
    uint32_t gep_parts = 0;
    uint32_t* g_regs = nullptr;
    uint32_t* g_probe = nullptr;
    uint8_t* g_stack = nullptr;
    // exploration archive (pk_archive_create; pk_layout.h PkArchArgs), arch_cells = 0 without one:
    // the persistent part, and the per-call words of an update in two blocks, one cleared to all
    // ones (empty keys, the min words) and one to zero (the max words, the counts)
    uint32_t arch_cells = 0, arch_slot0 = 0, arch_imask = 0;
    uint64_t arch_seed = 0;
    uint8_t* a_fix = nullptr;
    uint8_t* a_ones = nullptr;
    uint8_t* a_zero = nullptr;
    // archive exchange (pk_archive_exchange_enable), null without it: the per-cell sent / dirty words
    // with the per-record words of a merge, and a merge's own cleared-to-ones / cleared-to-zero blocks,
    // sized for PK_XCHG_MAX_RECORDS records
    uint8_t* x_fix = nullptr;
    uint8_t* x_ones = nullptr;
    uint8_t* x_zero = nullptr;
    // action trajectories (pk_traj_enable; pk_reward.h PkTrajArgs), traj_cap = 0 without them: the
    // envs' rows, origins and flags, and the slots' while the bank carries episode parts
    uint32_t traj_cap = 0;
    uint8_t* t_act = nullptr;
    int32_t* t_origin = nullptr;
    uint32_t* t_flags = nullptr;
    uint8_t* bt_act = nullptr;
    int32_t* bt_origin = nullptr;
    uint32_t* bt_flags = nullptr;
    // visit counts (pk_counts_create; pk_layout.h PkCountArgs), cnt_log2 = 0 without a table: the
    // header words, the three arrays of the table and the per-env entry words of an update
    uint32_t cnt_log2 = 0;
    uint8_t* c_fix = nullptr;
    // frame stack (pk_fstack_create; pk_layout.h PkStackArgs), fs_depth = 0 without one: u8[n][D * H * W]
    uint32_t fs_scale = 0, fs_depth = 0, fs_layout = 0, fs_mode = 0;
    uint8_t* fs_stack = nullptr;
    // RAM probes (pk_probe_create; pk_layout.h PkProbeArgs), pr_m = 0 without a program: the program
    // on the device and the state words u32[m][npad]
    uint32_t pr_m = 0;
    pk_probe* pr_prog = nullptr;
    uint32_t* pr_state = nullptr;
    // tile view (pk_tiles_create; pk_layout.h PkTilesArgs), tl_planes = 0 without one: u16[n][P][18][20];
    // tl_bits = 0 in PK_TILES_ID mode
    uint32_t tl_planes = 0, tl_bits = 0;
    uint16_t* tl_out = nullptr;
    // profiling: 4 events per profiled step (start, after K1, after K2, after K4+K3)
    bool prof = false;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    // every device allocation of the handle (Stage::commit): what pk_destroy frees.  The typed fields
    // above are the access path only
    std::vector<void*> owned;
};

// ---- device memory: one owner, one staged allocation ---------------------------------------------
//
// A feature allocates through a Stage.  It names the buffers it wants — the handle field, the byte
// count (0: none), a fill byte or a host source — and run() allocates them, fills or uploads them and
// synchronises once.  Until commit() the handle is untouched: a failed run(), or a Stage that goes
// out of scope, frees what was staged.  commit() publishes the pointers into the fields and the
// owner; a field that held a buffer gives it up (it leaves the owner and is freed), which is how the
// grow path of pk_set_episode_params replaces its buffers.  So a new feature stages, runs, does
// whatever else can fail, commits, and only then sets the field that says it is there.
class Stage {
  public:
    explicit Stage(pk_handle* h) : h_(h) {}
    Stage(const Stage&) = delete;
    Stage& operator=(const Stage&) = delete;
    ~Stage() { drop(); }

    template <class T>
    void want(T*& field, size_t bytes, int fill_byte = -1, const void* src = nullptr) {
        if (!bytes) return;
        reqs_.push_back(Req{(void**)&field, nullptr, bytes});
        if (fill_byte >= 0 || src) ops_.push_back(Op{(void**)&field, 0, bytes, fill_byte, src});
    }
    // further work on a part of a wanted buffer, in the order given
    template <class T>
    void fill(T*& field, size_t off, size_t bytes, int byte) { ops_.push_back(Op{(void**)&field, off, bytes, byte, nullptr}); }
    template <class T>
    void upload(T*& field, const void* src, size_t bytes) { ops_.push_back(Op{(void**)&field, 0, bytes, -1, src}); }

    // the buffer staged for a field (null: none)
    template <class T>
    T* staged(T*& field) const {
        for (const Req& r : reqs_)
            if (r.dst == (void**)&field) return (T*)r.p;
        return nullptr;
    }

    // what was asked for since the last run(); on failure everything staged so far is freed, the
    // sticky error cleared, and oom / failed_bytes say whether and which allocation it was
    hipError_t run() {
        hipError_t e = hipSuccess;
        oom = false;
        for (; ran_ < reqs_.size() && e == hipSuccess; ran_++) {
            Req& r = reqs_[ran_];
            e = hipMalloc(&r.p, r.bytes);
            if (e != hipSuccess) { r.p = nullptr; oom = true; failed_bytes = r.bytes; }
        }
        for (const Op& o : ops_) {
            if (e != hipSuccess) break;
            uint8_t* p = nullptr;
            for (const Req& r : reqs_)
                if (r.dst == o.dst) p = (uint8_t*)r.p + o.off;
            e = o.src ? hipMemcpy(p, o.src, o.bytes, hipMemcpyHostToDevice) : hipMemset(p, o.byte, o.bytes);
        }
        ops_.clear();
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) {
            drop();
            (void)hipGetLastError();
        }
        return e;
    }

    void commit() {
        for (const Req& r : reqs_) {
            if (*r.dst) {
                for (void*& q : h_->owned)
                    if (q == *r.dst) { q = h_->owned.back(); h_->owned.pop_back(); break; }
                (void)hipFree(*r.dst);
            }
            *r.dst = r.p;
            h_->owned.push_back(r.p);
        }
        reqs_.clear();
        ran_ = 0;
    }

    bool oom = false;
    size_t failed_bytes = 0;

  private:
    struct Req { void** dst; void* p; size_t bytes; };
    struct Op { void** dst; size_t off, bytes; int byte; const void* src; };
    void drop() {
        for (const Req& r : reqs_)
            if (r.p) (void)hipFree(r.p);
        reqs_.clear();
        ops_.clear();
        ran_ = 0;
    }
    pk_handle* h_;
    std::vector<Req> reqs_;
    std::vector<Op> ops_;
    size_t ran_ = 0;
};

static int prof_event(pk_handle* h, hipStream_t s) {
    if (h->ev_used == h->ev_pool.size()) {
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        h->ev_pool.push_back(e);
    }
    HIPCHK(hipEventRecord(h->ev_pool[h->ev_used++], s));
    return 0;
}

extern "C" {

static int template_reset(pk_handle* h, const uint8_t* mask, uint32_t env0, uint32_t env1, void* stream);

const char* pk_last_error(void) { return g_err.c_str(); }
int pk_abi_version(void) { return PK_ABI_VERSION; }
uint8_t* pk_screen_ptr(pk_handle* h) { return h ? h->screen : nullptr; }
uint8_t* pk_obs_ptr(pk_handle* h) { return h ? h->obs : nullptr; }
const uint32_t* pk_error_ptr(pk_handle* h) { return (h && h->rs) ? h->rs + (size_t)RS_ERR * h->npad : nullptr; }
const double* pk_info_ptr(pk_handle* h) { return h ? h->info : nullptr; }
const uint8_t* pk_info_flag_ptr(pk_handle* h) { return h ? h->info_flag : nullptr; }
int32_t* pk_heatmap_ptr(pk_handle* h) { return h ? h->heat : nullptr; }
const uint32_t* pk_info_bits_ptr(pk_handle* h) { return h ? h->info_bits : nullptr; }
uint32_t pk_num_envs(const pk_handle* h) { return h ? h->n : 0; }
uint32_t pk_info_stride(const pk_handle* h) { return h ? h->npad : 0; }

void pk_destroy(pk_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    for (hipEvent_t e : h->ev_pool) (void)hipEventDestroy(e);
    for (void* p : h->owned) (void)hipFree(p);
    delete h;
}

static uint32_t k1_wave_lanes(const struct pk_handle* h, uint32_t count);

int pk_create(const pk_config* cfg, pk_handle** out) {
    if (!cfg || !out) return fail(-EINVAL, "null argument");
    *out = nullptr;
    if (cfg->n_envs == 0) return fail(-EINVAL, "n_envs must be > 0");
    if (!cfg->rom || cfg->rom_len < 0x8000 || (cfg->rom_len & 0x3FFF))
        return fail(-EINVAL, "ROM must be a multiple of 16 KiB and >= 32 KiB");
    uint32_t banks = (uint32_t)(cfg->rom_len / 0x4000);
    if (banks & (banks - 1)) return fail(-EINVAL, "ROM bank count must be a power of two");
    uint8_t type = cfg->rom[0x147];
    uint32_t mbc;
    if (type == 0x00) mbc = 0;
    else if (type >= 0x0F && type <= 0x13) mbc = 3;
    else return fail(-ENOTSUP, "cartridge type 0x%02x not supported (ROM-only and MBC3 are)", type);
    // frame_skip 0 = no emulation (reward-stack replay tests drive RAM through pk_set_ram)
    if (cfg->frame_skip > 1024) return fail(-EINVAL, "bad frame_skip");

    pk_handle* h = new pk_handle();
    h->device = cfg->device;
    h->n = cfg->n_envs;
    h->npad = (cfg->n_envs + PK_LANES - 1) / PK_LANES * PK_LANES;
    h->ngroups = h->npad / PK_LANES;
    {
        // K1 wave shape: chosen per launch from the launch's env count (k1_wave_lanes);
        // PK_WAVE_LANES (a power of two <= 64) fixes it.
        int ncu = 0;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, cfg->device) != hipSuccess || ncu <= 0) ncu = 256;
        h->simds = 4u * (uint32_t)ncu;
        h->wave_lanes = 0;
        if (const char* wl = getenv("PK_WAVE_LANES")) {
            int v = atoi(wl);
            if (v < 1 || v > 64 || (v & (v - 1))) { delete h; return fail(-EINVAL, "PK_WAVE_LANES must be a power of two <= 64"); }
            h->wave_lanes = (uint32_t)v;
        }
        // K1 workgroup size override (parity tests run the benchmarked 512-thread shape at small n):
        // a multiple of 64 whose envs fit the 512-env HRAM mirror of a workgroup
        if (const char* bl = getenv("PK_K1_BLOCK")) {
            int v = atoi(bl);
            if (v < 64 || v > 512 || (v % 64) || (uint32_t)(v / 64) * (h->wave_lanes ? h->wave_lanes : 32u) > 512u) {
                delete h;
                return fail(-EINVAL, "PK_K1_BLOCK must be a multiple of 64 in [64, 512] with (block/64)*wave_lanes <= 512");
            }
            h->k1_block = (uint32_t)v;
        }
        if (const char* pr = getenv("PK_K1_PRIO")) h->k1_prio = atoi(pr) ? 1 : 0;
        if (const char* sm = getenv("PK_K1_SMALL")) h->k1_small = atoi(sm) ? 1 : 0;
        // image interleave = K1's envs per wave for this handle (no 64-byte line shared by two
        // waves; a wave's lanes share one sub-block base).  PK_ILV overrides it with any power of
        // two <= 64: narrower than the wave puts one wave's envs in several sub-blocks (K1 reaches
        // them through its per-lane offset), wider shares a sub-block between waves
        uint32_t ilv = k1_wave_lanes(h, h->n);
        if (const char* iv = getenv("PK_ILV")) {
            int v = atoi(iv);
            if (v < 1 || v > 64 || (v & (v - 1))) {
                delete h;
                return fail(-EINVAL, "PK_ILV must be a power of two <= 64");
            }
            ilv = (uint32_t)v;
        }
        h->ilv_sh = (uint32_t)__builtin_ctz(ilv);
    }
    h->frames = cfg->frame_skip;
    h->release = cfg->release_frame;
    h->flags = cfg->flags;
    h->max_steps = cfg->max_episode_steps ? cfg->max_episode_steps : 20480;
    h->reward_scale = cfg->reward_scale != 0.0 ? cfg->reward_scale : 4.0;
    // seen-coordinate set: one entry per step at most, load factor <= 3/4
    h->cap_log2 = 10;
    while ((1ull << h->cap_log2) * 3 < ((uint64_t)h->max_steps + 2) * 4) h->cap_log2++;
    h->mbc = mbc;
    h->bank_mask = banks - 1;
    h->lat_stride = (size_t)h->ngroups * PK_ROWS * PK_LANES;
    int rc;
    if (cfg->state) {
        if ((rc = parse_v9(cfg->state, cfg->state_len, h->tmpl))) { delete h; return rc; }
    } else {
        power_on(h->tmpl);
    }
    if (hipSetDevice(h->device) != hipSuccess) { delete h; return fail(-ENODEV, "hipSetDevice(%d) failed", cfg->device); }
    std::vector<uint32_t> uc(PK_UC_WORDS);
    pk_build_ucode(uc.data());
    int8_t bs[128], bs_s[128];
    uint8_t sb[PK_LDS_SLOTS] = {0};
    {
        // ROM banks staged in LDS by the step kernel: bank 0, then the switchable banks that hold
        // code or data, in bank order (a bank of one repeated byte — an unused bank of the
        // cartridge — only after those), so a small slot budget is not spent on an empty bank.
        // PK_STAGE_BANKS=b1,b2,... puts those banks first (experiments); PK_LDS_SLOTS=1..6 caps the count.
        const uint32_t nb = banks < 128u ? banks : 128u;   // MBC3: 7-bit bank number
        std::vector<uint32_t> order;
        std::vector<bool> used(nb, false);
        used[0] = true;
        order.push_back(0);
        if (const char* ev = getenv("PK_STAGE_BANKS")) {
            for (const char* q = ev; *q;) {
                char* end = nullptr;
                const unsigned long b = strtoul(q, &end, 10);
                if (end == q) break;
                if (b < nb && !used[b]) { used[b] = true; order.push_back((uint32_t)b); }
                q = *end ? end + 1 : end;
            }
        }
        for (int pass = 0; pass < 2; pass++)
            for (uint32_t b = 1; b < nb; b++) {
                if (used[b]) continue;
                const uint8_t* bp = cfg->rom + (size_t)b * 0x4000u;
                bool blank = true;
                for (uint32_t i = 1; i < 0x4000u && blank; i++) blank = bp[i] == bp[0];
                if (blank == (pass == 1)) { used[b] = true; order.push_back(b); }
            }
        uint32_t want = PK_LDS_SLOTS;
        if (const char* ev = getenv("PK_LDS_SLOTS")) want = (uint32_t)atoi(ev);
        if (want < 1) want = 1;
        if (want > PK_LDS_SLOTS) want = PK_LDS_SLOTS;
        if (want > nb) want = nb;
        memset(bs, -1, sizeof bs);
        for (uint32_t k = 0; k < want; k++) { sb[k] = (uint8_t)order[k]; bs[order[k]] = (int8_t)k; }
        h->nslots = want;
        // the small-LDS kernel stages the first PK_SMALL_LDS_SLOTS of the same banks
        h->nslots_s = want < PK_SMALL_LDS_SLOTS ? want : PK_SMALL_LDS_SLOTS;
        memcpy(bs_s, bs, sizeof bs);
        for (uint32_t k = h->nslots_s; k < want; k++) bs_s[order[k]] = -1;
    }
    Stage st(h);
    st.want(h->mem, (size_t)h->ngroups * PK_GROUP_STRIDE);
    st.want(h->regs, (size_t)PK_NREGS * h->npad * 4, 0);
    st.want(h->lat, 3 * h->lat_stride * 4, 0);
    st.want(h->screen, (size_t)h->npad * PK_SCREEN);
    st.want(h->rom, cfg->rom_len + 16);
    st.fill(h->rom, cfg->rom_len, 16, 0xFF);
    st.upload(h->rom, cfg->rom, cfg->rom_len);
    st.want(h->ucode, PK_UC_WORDS * 4, -1, uc.data());
    st.want(h->bank_slot, 128, -1, bs);
    st.want(h->slot_bank, PK_LDS_SLOTS, -1, sb);
    st.want(h->bank_slot_s, 128, -1, bs_s);
    st.want(h->slot_bank_s, PK_SMALL_LDS_SLOTS, -1, sb);
    st.want(h->t_mem, PK_PHYS, -1, h->tmpl.mem.data());
    st.want(h->t_regs, PK_NREGS * 4, -1, h->tmpl.regs);
    st.want(h->t_lat, 3 * PK_ROWS * 4, -1, h->tmpl.lat);
    st.want(h->t_screen, PK_SCREEN, -1, h->tmpl.screen.data());
    st.want(h->scratch, PK_PHYS + PK_NREGS * 4 + 3 * PK_ROWS * 4 + PK_SCREEN);
    st.want(h->lists, (2 * (size_t)h->ngroups + 2 * (size_t)h->npad) * 4);
#if defined(PK_STAMP) || defined(PK_WAVETIME)
    st.want(h->dbg, PK_DBG_WORDS * 8, 0);
#endif
    if (h->flags & PK_F_REWARD) {
        // nothing has been reset yet (reset_count 0); update_heat_map's last_map = -1 (:462)
        st.want(h->rs, (size_t)RS_NFIELDS * h->npad * 4, 0);
        st.fill(h->rs, (size_t)RS_HEAT_LAST * h->npad * 4, (size_t)h->npad * 4, 0xFF);
        st.fill(h->rs, (size_t)RS_MASK_MAP * h->npad * 4, (size_t)h->npad * 4, 0xFF);
        st.want(h->rsd, (size_t)RSD_NFIELDS * h->npad * 8, 0);
        st.want(h->seen, (size_t)h->npad * (1ull << h->cap_log2) * 4, 0);
        st.want(h->mask, (size_t)h->npad * PK_MASK_WORDS * 4, 0);
        st.want(h->cutc, (size_t)h->npad * PK_CUTC_CAP * 4);
        st.want(h->obs, (size_t)h->npad * PK_OBS_BYTES, 0);
        st.want(h->reload, h->npad);
        st.want(h->info, (size_t)PK_INFO_NFIELDS * h->npad * 8, 0);
        st.want(h->info_flag, h->npad, 0);
        st.want(h->info_bits, (size_t)PK_INFO_BITS_WORDS * h->npad * 4, 0);
        if (h->flags & PK_F_HEATMAP) st.want(h->heat, (size_t)h->npad * PK_HEAT_ROWS * PK_HEAT_COLS * 4, 0);
    }
    if (hipError_t e = st.run()) {
        delete h;
        if (st.oom) return fail(-ENOMEM, "hipMalloc(%zu): %s", st.failed_bytes, hipGetErrorString(e));
        return fail(-EIO, "device upload failed: %s", hipGetErrorString(e));
    }
    st.commit();
    if ((rc = template_reset(h, nullptr, 0, h->n, nullptr))) { pk_destroy(h); return rc; }
    if (hipDeviceSynchronize() != hipSuccess) { pk_destroy(h); return fail(-EIO, "initial reset failed"); }
    *out = h;
    return 0;
}

static PkRewardArgs reward_args(pk_handle* h, uint32_t env0, uint32_t env1) {
    PkRewardArgs r;
    memset(&r, 0, sizeof r);
    r.mem = h->mem; r.regs = h->regs; r.rs = h->rs; r.rsd = h->rsd; r.seen = h->seen; r.mask = h->mask;
    r.cutc = h->cutc; r.reload = h->reload; r.screen = h->screen; r.obs = h->obs;
    r.info = h->info; r.info_flag = h->info_flag; r.heat = h->heat; r.info_bits = h->info_bits;
    r.reward_scale = h->reward_scale; r.n = h->n; r.npad = h->npad; r.cap_log2 = h->cap_log2;
    r.max_steps = h->max_steps; r.reload_always = (h->flags & PK_F_RELOAD_ON_RESET) ? 1 : 0;
    r.env0 = env0; r.env1 = env1; r.ilv_sh = h->ilv_sh;
    return r;
}

// reset lists of an env range (env0 % 64 == 0): counters [2 * (env0 / 64)] (reload) and [+1] (obs),
// ids from env0 in the reload and obs id arrays — disjoint ranges (sub-batches on their own
// streams) never share a counter or an id slot
static uint32_t* list_cnt(pk_handle* h, uint32_t env0, int which) { return h->lists + 2u * (env0 / PK_LANES) + which; }
static uint32_t* list_ids(pk_handle* h, uint32_t env0, int which) {
    return h->lists + 2u * h->ngroups + (size_t)which * h->npad + env0;
}

// the template reload of the envs of [env0, env1) that the range's reset list names
static PkResetArgs reset_args(pk_handle* h, uint32_t env0, uint32_t env1) {
    PkResetArgs a;
    a.mem = h->mem; a.regs = h->regs; a.lat = h->lat; a.screen = h->screen;
    a.tmpl_mem = h->t_mem; a.tmpl_regs = h->t_regs; a.tmpl_lat = h->t_lat; a.tmpl_screen = h->t_screen;
    a.cnt = list_cnt(h, env0, 0); a.ids = list_ids(h, env0, 0); a.n = h->n; a.npad = h->npad;
    a.lat_stride = (uint32_t)h->lat_stride; a.env0 = env0; a.env1 = env1; a.ilv_sh = h->ilv_sh;
    return a;
}

// reload the template state (regs, RAM image, latches, screen) into the masked envs of [env0, env1):
// the envs are listed on the device first, so the reset costs in proportion to the envs it touches
static int template_reset(pk_handle* h, const uint8_t* mask, uint32_t env0, uint32_t env1, void* stream) {
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(list_cnt(h, env0, 0), 0, 4, s));
    HIPCHK(pk_launch_list(mask, env0, env1, list_cnt(h, env0, 0), list_ids(h, env0, 0), s));
    HIPCHK(pk_launch_reset(reset_args(h, env0, env1), s));
    return 0;
}

static int check_range(pk_handle* h, uint32_t env0, uint32_t count) {
    if (!h) return fail(-EINVAL, "null handle");
    if (count == 0 || env0 % PK_LANES || (uint64_t)env0 + count > h->n)
        return fail(-EINVAL, "env range [%u, +%u): the start must be a multiple of 64 and the end <= n = %u", env0, count, h->n);
    return 0;
}

// ---- action trajectories: the pieces the other calls use (the entry points are at the end) ------

static PkTrajArgs traj_args(pk_handle* h, uint32_t env0, uint32_t env1) {
    PkTrajArgs a;
    memset(&a, 0, sizeof a);
    a.time_reg = h->regs + (size_t)PK_R_TIME * h->npad;
    a.act = h->t_act; a.origin = h->t_origin; a.flags = h->t_flags;
    a.b_act = h->bt_act; a.b_origin = h->bt_origin; a.b_flags = h->bt_flags;
    a.e_fields = h->e_fields; a.b_ep_filled = h->b_ep_filled;
    a.e_stride = PK_EP_WORDS; a.e_time = PK_EP_REGS + PK_R_TIME;
    if (h->gep_parts) {   // a slot's length is the step counter among its raw registers
        a.e_fields = h->g_regs; a.e_stride = PK_GEP_REGS; a.e_time = PK_R_TIME;
    }
    a.cap = h->traj_cap; a.env0 = env0; a.env1 = env1;
    return a;
}

// the reset of [env0, env1) just made: the masked envs start an empty list at the slot src names
// (null: the template); with a reload array, those it leaves out kept their machine (PK_TRAJ_BROKEN)
static int traj_reset(pk_handle* h, const uint8_t* mask, const uint8_t* reload, const int32_t* src, uint32_t env0,
                      uint32_t env1, hipStream_t s) {
    if (!h->traj_cap) return 0;
    PkTrajArgs a = traj_args(h, env0, env1);
    a.mask = mask; a.reload = reload; a.src = src;
    HIPCHK(pk_launch_traj_reset(a, s));
    return 0;
}

// PK_TRAJ_BROKEN for the envs of a device-built list (cnt, ids; at most env1 - env0), or without
// one for every env of [env0, env1)
static int traj_mark(pk_handle* h, const uint32_t* cnt, const uint32_t* ids, uint32_t env0, uint32_t env1, hipStream_t s) {
    if (!h->traj_cap) return 0;
    PkTrajArgs a = traj_args(h, env0, env1);
    a.cnt = cnt; a.ids = ids; a.items = env1 - env0;
    HIPCHK(pk_launch_traj_mark(a, s));
    return 0;
}

// stages one set of trajectory parts for the three fields given: rows of cap bytes zeroed, an
// origin of -1 and a flag word as given per row
static int traj_stage(Stage& st, uint8_t*& act, int32_t*& origin, uint32_t*& flags, size_t rows, uint32_t cap,
                      const std::vector<uint32_t>& row_flags) {
    st.want(act, rows * cap, 0);
    st.want(origin, rows * 4, 0xFF);
    st.want(flags, rows * 4, -1, row_flags.data());
    const hipError_t e = st.run();
    if (e == hipSuccess) return 0;
    return fail(-ENOMEM, "trajectories of %zu rows of %u bytes: %s", rows, cap, hipGetErrorString(e));
}
static int traj_stage_envs(Stage& st, pk_handle* h, uint32_t cap, const std::vector<uint32_t>& row_flags) {
    return traj_stage(st, h->t_act, h->t_origin, h->t_flags, h->npad, cap, row_flags);
}
static int traj_stage_slots(Stage& st, pk_handle* h, uint32_t cap, uint32_t flag) {
    return traj_stage(st, h->bt_act, h->bt_origin, h->bt_flags, h->bank_n, cap, std::vector<uint32_t>(h->bank_n, flag));
}

static uint32_t traj_cap_of(uint32_t cap_log2) { return 3u << (cap_log2 - 2u); }

static int reset_envs(pk_handle* h, uint32_t env0, uint32_t count, const uint8_t* mask, const int32_t* slots, void* stream);

int pk_reset_range(pk_handle* h, uint32_t env0, uint32_t count, const uint8_t* mask, void* stream) {
    return reset_envs(h, env0, count, mask, nullptr, stream);
}

int pk_reset(pk_handle* h, const uint8_t* mask, void* stream) {
    if (!h) return fail(-EINVAL, "null handle");
    return pk_reset_range(h, 0, h->n, mask, stream);
}

int pk_get_ram(pk_handle* h, uint16_t addr, uint32_t len, uint8_t* dense, void* stream) {
    if (!h || !dense) return fail(-EINVAL, "null argument");
    bool wram = addr >= 0xC000 && (uint32_t)addr + len <= 0xFE00, hram = addr >= 0xFF80 && (uint32_t)addr + len <= 0xFFFF;
    if (!len || !(wram || hram)) return fail(-EINVAL, "pk_get_ram: [0x%04x, +%u) is not inside WRAM/echo or HRAM", addr, len);
    if (wram && (addr & 0x1FFF) + len > 0x2000) return fail(-EINVAL, "pk_get_ram: range wraps the echo mirror");
    HIPCHK(hipSetDevice(h->device));
    uint32_t phys0 = wram ? PK_P_WRAM + (addr & 0x1FFFu) : PK_P_HRAM + (addr - 0xFF80u);
    HIPCHK(pk_launch_ram_copy(h->mem, dense, h->n, h->ilv_sh, phys0, len, 1, (hipStream_t)stream));
    return 0;
}

int pk_set_ram(pk_handle* h, uint16_t addr, uint32_t len, const uint8_t* dense, void* stream) {
    if (!h || !dense) return fail(-EINVAL, "null argument");
    bool wram = addr >= 0xC000 && (uint32_t)addr + len <= 0xFE00, hram = addr >= 0xFF80 && (uint32_t)addr + len <= 0xFFFF;
    if (!len || !(wram || hram)) return fail(-EINVAL, "pk_set_ram: [0x%04x, +%u) is not inside WRAM/echo or HRAM", addr, len);
    if (wram && (addr & 0x1FFF) + len > 0x2000) return fail(-EINVAL, "pk_set_ram: range wraps the echo mirror");
    HIPCHK(hipSetDevice(h->device));
    uint32_t phys0 = wram ? PK_P_WRAM + (addr & 0x1FFFu) : PK_P_HRAM + (addr - 0xFF80u);
    HIPCHK(pk_launch_ram_copy(h->mem, const_cast<uint8_t*>(dense), h->n, h->ilv_sh, phys0, len, 0, (hipStream_t)stream));
    return traj_mark(h, nullptr, nullptr, 0, h->n, (hipStream_t)stream);
}

// K1 envs per wave for a launch of `count` envs (measured, profiles/r02_sweep_*, r02_ab/ab_prio.txt):
// the widest wave that still gives two waves per SIMD, whose priority variant hides one wave's
// fetch -> operand-read chain behind the other's datapath — 64 from 131,072 envs, 32 from 65,536
// (two 32-lane waves per SIMD beat one 64-lane wave by ~10 %), 16 for (16,384, 32,768] (configs[3]'s
// per-GPU shard: two 16-lane waves with priority +5 % over one 32-lane wave; without priority they
// were 4 % slower).  Smaller launches are latency-bound and keep one 32-lane wave per SIMD (more,
// narrower waves do not help: 4,096 envs at 4 per wave on every CU measured 2.4x slower); between
// the thresholds the narrower shape would need a second round of workgroups.  PK_WAVE_LANES fixes it.
static uint32_t k1_wave_lanes(const pk_handle* h, uint32_t count) {
    if (h->wave_lanes) return h->wave_lanes;
    const uint32_t npad = (count + PK_LANES - 1u) & ~(PK_LANES - 1u);
    if (npad / 64u >= 2u * h->simds) return 64u;
    if (npad / 32u >= 2u * h->simds) return 32u;
    if (npad / 16u > h->simds && npad / 16u <= 2u * h->simds) return 16u;
    return 32u;
}

// K1 wave shape and workgroup size of a launch.  A sub-batch range is shaped as if every env of the
// handle were resident at once: VecEnv steps its sub-batches concurrently on their own streams, and
// K1 runs one workgroup per CU (LDS), so concurrent ranges share the GPU only when each is laid
// out for its part of the CUs — e.g. the two 65,536-env halves of a 131,072-env handle run as 64-env
// waves in 512-thread workgroups, 128 CUs each, two waves per SIMD overall (shaped alone, each
// took every CU and the second range waited: 485k vs 688k env-steps/s).
// The wide (512-thread) shape puts two waves on each SIMD; those launches take K1's wave-priority
// variant (measured +5 % at 65,536 envs; with one wave per SIMD it only costs its two instructions).
static void k1_shape(const pk_handle* h, bool small, uint32_t& lanes, uint32_t& block, uint32_t& prio) {
    lanes = k1_wave_lanes(h, h->n);
    const uint32_t wg_envs = small ? PK_SMALL_WG_ENVS : PK_WG_ENVS;
    const uint32_t max_threads = small ? PK_SMALL_MAX_THREADS : PK_K1_MAX_THREADS;
    if (h->k1_block) {
        // PK_K1_BLOCK with the lanes picked for this handle: a workgroup holds at most wg_envs envs
        // (its HRAM code mirror), so a block too large for the wave width is narrowed
        block = h->k1_block < max_threads ? h->k1_block : max_threads;
        if ((block / PK_LANES) * lanes > wg_envs) block = wg_envs / lanes * PK_LANES;
    } else {
        const uint32_t waves = ((h->n + PK_LANES - 1u) / PK_LANES) * (PK_LANES / lanes);
        const uint32_t wide = wg_envs * PK_LANES / lanes < max_threads ? wg_envs * PK_LANES / lanes : max_threads;
        block = waves <= h->simds ? 256u : wide;
    }
    // wave priority pays with two waves of one workgroup per SIMD (measured +5 %); with the small
    // kernel the SIMD's second wave belongs to the other sub-batch, and priority measured -4 %
    // (profiles/r04b/summary.txt)
    prio = h->k1_prio >= 0 ? (uint32_t)h->k1_prio : (block > 256u && !small ? 1u : 0u);
}

// K1 variant of a launch: the small-LDS kernel for a range smaller than the handle (a VecEnv
// sub-batch, stepped concurrently with the others on its own stream) while waves carry <= 32 envs
// (its HRAM mirror holds 128 envs per 256-thread workgroup); measured +3 % on configs[3]'s 32,768-env
// shard in 2 sub-batches, -3..-7 % for whole-handle launches, which gain nothing from a second
// workgroup per CU but lose the staged banks (profiles/r04b, r04c)
static bool k1_small(const pk_handle* h, uint32_t env0, uint32_t env1) {
    if (h->k1_small >= 0) return h->k1_small != 0 && k1_wave_lanes(h, h->n) <= 32u;
    return (env1 - env0) < h->n && k1_wave_lanes(h, h->n) <= 32u;
}

static PkStepArgs step_args(pk_handle* h, const uint8_t* actions, uint32_t env0, uint32_t env1) {
    PkStepArgs a;
    memset(&a, 0, sizeof a);
    a.mem = h->mem; a.rom = h->rom; a.romw = reinterpret_cast<const uint32_t*>(h->rom); a.regs = h->regs; a.ucode = h->ucode; a.actions = actions;
    a.lat = h->lat; a.screen = h->screen; a.n = h->n; a.npad = h->npad;
    a.rom_bank_mask = h->bank_mask; a.mbc = h->mbc; a.frames = h->frames;
    a.release_frame = h->release; a.render_last = (h->flags & PK_F_RENDER) ? 1 : 0;
    a.lat_stride = (uint32_t)h->lat_stride;
    const bool small = k1_small(h, env0, env1);
    a.small = small ? 1u : 0u;
    a.nslots = small ? h->nslots_s : h->nslots;
    a.bank_slot = small ? h->bank_slot_s : h->bank_slot;
    a.slot_bank = small ? h->slot_bank_s : h->slot_bank;
    a.all_staged = a.nslots >= h->bank_mask + 1u ? 1u : 0u;   // pk_step.hip ALL: no unstaged-bank paths
    k1_shape(h, small, a.wave_lanes, a.block, a.prio);
    a.simds = h->simds;
    a.dbg = h->dbg;
    a.env0 = env0; a.env1 = env1;
    a.ilv_sh = h->ilv_sh;
    return a;
}

int pk_render_latched(pk_handle* h, void* stream) {
    if (!h) return fail(-EINVAL, "null handle");
    HIPCHK(hipSetDevice(h->device));
    PkStepArgs a = step_args(h, nullptr, 0, h->n);
    HIPCHK(pk_launch_render_latched(a, (hipStream_t)stream));
    return 0;
}

int pk_step_range(pk_handle* h, uint32_t env0, uint32_t count, const uint8_t* actions, double* rew, uint8_t* term,
                  uint8_t* trunc, void* stream) {
    int rc;
    if ((rc = check_range(h, env0, count))) return rc;
    if (!actions) return fail(-EINVAL, "actions_dev is required");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const uint32_t env1 = env0 + count;
    PkStepArgs a = step_args(h, actions, env0, env1);
    if (h->prof && (rc = prof_event(h, s))) return rc;
    HIPCHK(a.small ? pk_launch_step_small(a, s) : pk_launch_step(a, s));
    if (h->traj_cap) {
        PkTrajArgs t = traj_args(h, env0, env1);
        t.actions = actions;
        HIPCHK(pk_launch_traj_record(t, s));
    }
    if (h->prof && (rc = prof_event(h, s))) return rc;
    // a rendered step without the reward stack: K2 writes the termination flags too
    const bool fuse_done = a.render_last && !(h->flags & PK_F_REWARD) && (rew || term || trunc);
    if (fuse_done) {
        PkDoneArgs d;
        d.time_reg = h->regs + (size_t)PK_R_TIME * h->npad;
        d.term = term; d.trunc = trunc; d.rew = rew;
        d.max_steps = h->max_steps; d.on = 1u;
        HIPCHK(pk_launch_render_done(a, d, s));
    } else if (a.render_last) {
        HIPCHK(pk_launch_render(a, s));
    }
    if (h->prof && (rc = prof_event(h, s))) return rc;
    if (h->flags & PK_F_REWARD) {
        PkRewardArgs r = reward_args(h, env0, env1);
        r.actions = actions; r.rew = rew; r.term = term; r.trunc = trunc;
        HIPCHK(pk_launch_reward(r, s));
        HIPCHK(pk_launch_obs(r, s));
    } else if (!fuse_done && (rew || term || trunc)) {
        HIPCHK(pk_launch_done(h->regs + (size_t)PK_R_TIME * h->npad + env0, count, h->max_steps, term ? term + env0 : nullptr,
                              trunc ? trunc + env0 : nullptr, rew ? rew + env0 : nullptr, s));
    }
    if (h->prof && (rc = prof_event(h, s))) return rc;
    return 0;
}

int pk_step(pk_handle* h, const uint8_t* actions, uint8_t* screen_out, double* rew, uint8_t* term,
            uint8_t* trunc, void* stream) {
    if (!h) return fail(-EINVAL, "null handle");
    int rc = pk_step_range(h, 0, h->n, actions, rew, term, trunc, stream);
    if (rc) return rc;
    if (screen_out)
        HIPCHK(hipMemcpyAsync(screen_out, h->screen, (size_t)h->n * PK_SCREEN, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

// gather one env's full state to host: mem (PK_PHYS), regs, latches, screen
static int fetch_env(pk_handle* h, uint32_t env, std::vector<uint8_t>& mem, uint32_t* regs,
                     uint32_t* lat, std::vector<uint8_t>& screen) {
    if (env >= h->n) return fail(-EINVAL, "env %u out of range (n=%u)", env, h->n);
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(pk_launch_gather_env(h->mem, env, h->ilv_sh, h->scratch, nullptr));
    mem.resize(PK_PHYS);
    HIPCHK(hipMemcpy(mem.data(), h->scratch, PK_PHYS, hipMemcpyDeviceToHost));
    for (uint32_t f = 0; f < PK_NREGS; f++)
        HIPCHK(hipMemcpy(&regs[f], h->regs + (size_t)f * h->npad + env, 4, hipMemcpyDeviceToHost));
    uint32_t gid = env / PK_LANES, lane = env % PK_LANES;
    for (uint32_t k = 0; k < 3; k++) {
        std::vector<uint32_t> tmp((size_t)PK_ROWS * PK_LANES);
        HIPCHK(hipMemcpy(tmp.data(), h->lat + k * h->lat_stride + (size_t)gid * PK_ROWS * PK_LANES,
                         tmp.size() * 4, hipMemcpyDeviceToHost));
        for (uint32_t y = 0; y < PK_ROWS; y++) lat[k * PK_ROWS + y] = tmp[(size_t)y * PK_LANES + lane];
    }
    screen.resize(PK_SCREEN);
    HIPCHK(hipMemcpy(screen.data(), h->screen + (size_t)env * PK_SCREEN, PK_SCREEN, hipMemcpyDeviceToHost));
    return 0;
}

int pk_snapshot(pk_handle* h, uint32_t env, uint8_t* out, uint64_t len) {
    if (!h || !out) return fail(-EINVAL, "null argument");
    if (len < S_SIZE) return fail(-EINVAL, "buffer too small for a v9 state");
    std::vector<uint8_t> mem, screen;
    uint32_t regs[PK_NREGS], lat[3 * PK_ROWS];
    int rc = fetch_env(h, env, mem, regs, lat, screen);
    if (rc) return rc;
    export_v9(h->tmpl, regs, mem.data(), lat, screen.data(), out);
    return 0;
}

int pk_snapshot_range(pk_handle* h, uint32_t env0, uint32_t count, uint8_t* out, uint64_t len) {
    if (!h || !out) return fail(-EINVAL, "null argument");
    if (count == 0) return 0;
    if ((uint64_t)env0 + count > h->n) return fail(-EINVAL, "envs [%u, %u) out of range (n=%u)", env0, env0 + count, h->n);
    if (len < (uint64_t)count * S_SIZE) return fail(-EINVAL, "buffer too small for %u v9 states", count);
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    const uint32_t chunk = count < 1024u ? count : 1024u;
    // the call's own gather buffer: staged and never committed, so it goes with the Stage
    Stage tmp(h);
    uint8_t* dmem = nullptr;
    tmp.want(dmem, (size_t)chunk * PK_PHYS);
    if (hipError_t e = tmp.run()) return fail(-EIO, "pk_snapshot_range: %s", hipGetErrorString(e));
    dmem = tmp.staged(dmem);
    std::vector<uint8_t> mem((size_t)chunk * PK_PHYS), screen((size_t)chunk * PK_SCREEN);
    std::vector<uint32_t> regs((size_t)PK_NREGS * chunk), latg;
    int rc = 0;
    for (uint32_t c0 = 0; c0 < count && !rc; c0 += chunk) {
        const uint32_t e0 = env0 + c0, m = (count - c0) < chunk ? (count - c0) : chunk;
        hipError_t e = pk_launch_gather_range(h->mem, e0, m, h->ilv_sh, dmem, nullptr);
        if (e == hipSuccess) e = hipMemcpy(mem.data(), dmem, (size_t)m * PK_PHYS, hipMemcpyDeviceToHost);
        for (uint32_t f = 0; f < PK_NREGS && e == hipSuccess; f++)
            e = hipMemcpy(&regs[(size_t)f * chunk], h->regs + (size_t)f * h->npad + e0, (size_t)m * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess)
            e = hipMemcpy(screen.data(), h->screen + (size_t)e0 * PK_SCREEN, (size_t)m * PK_SCREEN, hipMemcpyDeviceToHost);
        // latches of the groups covering [e0, e0 + m)
        const uint32_t g0 = e0 / PK_LANES, g1 = (e0 + m - 1) / PK_LANES + 1, rows = (g1 - g0) * PK_ROWS * PK_LANES;
        latg.resize((size_t)3 * rows);
        for (uint32_t k = 0; k < 3 && e == hipSuccess; k++)
            e = hipMemcpy(&latg[(size_t)k * rows], h->lat + k * h->lat_stride + (size_t)g0 * PK_ROWS * PK_LANES,
                          (size_t)rows * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) { rc = fail(-EIO, "pk_snapshot_range: %s", hipGetErrorString(e)); break; }
        for (uint32_t i = 0; i < m; i++) {
            const uint32_t env = e0 + i, gi = env / PK_LANES - g0, lane = env % PK_LANES;
            uint32_t r[PK_NREGS], lat[3 * PK_ROWS];
            for (uint32_t f = 0; f < PK_NREGS; f++) r[f] = regs[(size_t)f * chunk + i];
            for (uint32_t k = 0; k < 3; k++)
                for (uint32_t y = 0; y < PK_ROWS; y++)
                    lat[k * PK_ROWS + y] = latg[(size_t)k * rows + ((size_t)gi * PK_ROWS + y) * PK_LANES + lane];
            export_v9(h->tmpl, r, &mem[(size_t)i * PK_PHYS], lat, &screen[(size_t)i * PK_SCREEN], out + (size_t)(c0 + i) * S_SIZE);
        }
    }
    return rc;
}

int pk_load_env(pk_handle* h, uint32_t env, const uint8_t* in, uint64_t len) {
    if (!h || !in) return fail(-EINVAL, "null argument");
    if (env >= h->n) return fail(-EINVAL, "env %u out of range", env);
    Template t;
    int rc = parse_v9(in, len, t);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(h->scratch, t.mem.data(), PK_PHYS, hipMemcpyHostToDevice));
    HIPCHK(pk_launch_scatter_env(h->mem, env, h->ilv_sh, h->scratch, nullptr));
    HIPCHK(hipDeviceSynchronize());
    // machine state only: the env's step counter (PK_R_TIME, pokegym `self.time`) and the per-step
    // bookkeeping slots survive a load, as in load_pyboy_state (pyboy_binding.py:59-62), which
    // leaves self.time alone; only reset() zeroes it
    for (uint32_t f = 0; f <= PK_R_MISC; f++)
        HIPCHK(hipMemcpy(h->regs + (size_t)f * h->npad + env, &t.regs[f], 4, hipMemcpyHostToDevice));
    uint32_t gid = env / PK_LANES, lane = env % PK_LANES;
    for (uint32_t k = 0; k < 3; k++)
        for (uint32_t y = 0; y < PK_ROWS; y++)
            HIPCHK(hipMemcpy(h->lat + k * h->lat_stride + ((size_t)gid * PK_ROWS + y) * PK_LANES + lane,
                             &t.lat[k * PK_ROWS + y], 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->screen + (size_t)env * PK_SCREEN, t.screen.data(), PK_SCREEN, hipMemcpyHostToDevice));
    if ((rc = traj_mark(h, nullptr, nullptr, env, env + 1, nullptr))) return rc;
    if (h->traj_cap) HIPCHK(hipDeviceSynchronize());
    return 0;
}

// guest-address view of one env's memory (PyBoy get_memory_value semantics for RAM regions and
// the special IO registers)
static int guest_phys(uint32_t addr, const uint32_t* regs, uint32_t mbc, uint32_t* phys, int* special) {
    *special = -1;
    if (addr < 0x8000) return -1;
    if (addr < 0xA000) { *phys = PK_P_VRAM + addr - 0x8000; return 0; }
    if (addr < 0xC000) {
        uint32_t m = regs[PK_R_MBC];
        if (mbc == 0 || !((m >> 16) & 0xFF)) return -2;
        *phys = PK_P_SRAM + (((m >> 8) & 3) * 0x2000) + (addr - 0xA000);
        return 0;
    }
    if (addr < 0xFE00) { *phys = PK_P_WRAM + (addr & 0x1FFF); return 0; }
    if (addr < 0xFF00) { *phys = PK_P_OAM + (addr - 0xFE00); return 0; }
    if (addr >= 0xFF80) {
        if (addr == 0xFFFF) { *special = (int)addr; return 1; }
        *phys = PK_P_HRAM + addr - 0xFF80;
        return 0;
    }
    if ((addr >= 0xFF04 && addr <= 0xFF07) || addr == 0xFF0F || (addr >= 0xFF10 && addr <= 0xFF4B)) {
        *special = (int)addr;
        return 1;
    }
    *phys = PK_P_IO + (addr - 0xFF00);
    return 0;
}

static uint8_t special_read(uint32_t a, const uint32_t* R) {
    auto b = [](uint32_t v, int sh) { return (uint8_t)((v >> sh) & 0xFF); };
    switch (a) {
        case 0xFF04: return b(R[PK_R_TIM0], 0);
        case 0xFF05: return b(R[PK_R_TIM0], 8);
        case 0xFF06: return b(R[PK_R_TIM0], 16);
        case 0xFF07: return b(R[PK_R_TIM0], 24);
        case 0xFF0F: return b(R[PK_R_CPU], 16);
        case 0xFF40: return b(R[PK_R_LCD0], 0);
        case 0xFF41: return b(R[PK_R_LCD0], 8);
        case 0xFF42: return b(R[PK_R_LCD1], 0);
        case 0xFF43: return b(R[PK_R_LCD1], 8);
        case 0xFF44: return b(R[PK_R_LCD0], 16);
        case 0xFF45: return b(R[PK_R_LCD0], 24);
        case 0xFF47: return b(R[PK_R_LCD2], 0);
        case 0xFF48: return b(R[PK_R_LCD2], 8);
        case 0xFF49: return b(R[PK_R_LCD2], 16);
        case 0xFF4A: return b(R[PK_R_LCD1], 16);
        case 0xFF4B: return b(R[PK_R_LCD1], 24);
        case 0xFFFF: return b(R[PK_R_CPU], 8);
        default: return 0;
    }
}

int pk_peek(pk_handle* h, uint32_t env, uint16_t addr, uint32_t len, uint8_t* out) {
    if (!h || !out) return fail(-EINVAL, "null argument");
    if ((uint32_t)addr + len > 0x10000u) return fail(-EINVAL, "range past 0xFFFF");
    std::vector<uint8_t> mem, screen;
    uint32_t regs[PK_NREGS], lat[3 * PK_ROWS];
    int rc = fetch_env(h, env, mem, regs, lat, screen);
    if (rc) return rc;
    std::vector<uint8_t> rom;
    for (uint32_t i = 0; i < len; i++) {
        uint32_t a = (uint32_t)addr + i, phys;
        int special;
        int k = guest_phys(a, regs, h->mbc, &phys, &special);
        if (k == 0) out[i] = mem[phys];
        else if (k == 1) out[i] = special_read(a, regs);
        else if (k == -2) out[i] = 0xFF;
        else {
            // ROM read
            uint32_t off = a < 0x4000 ? a : ((regs[PK_R_MBC] & 0xFF) & h->bank_mask) * 0x4000u + (a - 0x4000u);
            HIPCHK(hipMemcpy(&out[i], h->rom + off, 1, hipMemcpyDeviceToHost));
        }
    }
    return 0;
}

int pk_poke(pk_handle* h, uint32_t env, uint16_t addr, uint32_t len, const uint8_t* in) {
    if (!h || !in) return fail(-EINVAL, "null argument");
    if (env >= h->n) return fail(-EINVAL, "env %u out of range", env);
    if ((uint32_t)addr + len > 0x10000u) return fail(-EINVAL, "range past 0xFFFF");
    std::vector<uint8_t> mem, screen;
    uint32_t regs[PK_NREGS], lat[3 * PK_ROWS];
    int rc = fetch_env(h, env, mem, regs, lat, screen);
    if (rc) return rc;
    // flagged first: a poke that fails at a later byte has written the earlier ones
    if ((rc = traj_mark(h, nullptr, nullptr, env, env + 1, nullptr))) return rc;
    if (h->traj_cap) HIPCHK(hipDeviceSynchronize());
    for (uint32_t i = 0; i < len; i++) {
        uint32_t a = (uint32_t)addr + i, phys;
        int special;
        if (guest_phys(a, regs, h->mbc, &phys, &special) != 0)
            return fail(-ENOTSUP, "pk_poke supports RAM regions only (addr 0x%04x)", a);
        HIPCHK(hipMemcpy(h->mem + pk_img_off(env, phys, h->ilv_sh), &in[i], 1,
                         hipMemcpyHostToDevice));
    }
    return 0;
}

int pk_profile_enable(pk_handle* h, int on) {
    if (!h) return fail(-EINVAL, "null handle");
    h->prof = on != 0;
    return 0;
}

int pk_profile_read(pk_handle* h, double* emu_ms, double* render_ms, double* reward_ms, uint64_t* steps) {
    if (!h || !emu_ms || !render_ms || !reward_ms || !steps) return fail(-EINVAL, "null argument");
    HIPCHK(hipSetDevice(h->device));
    double a = 0, b = 0, c = 0;
    size_t n = h->ev_used / 4;
    if (n) HIPCHK(hipEventSynchronize(h->ev_pool[h->ev_used - 1]));
    for (size_t i = 0; i < n; i++) {
        float t1 = 0, t2 = 0, t3 = 0;
        HIPCHK(hipEventElapsedTime(&t1, h->ev_pool[4 * i], h->ev_pool[4 * i + 1]));
        HIPCHK(hipEventElapsedTime(&t2, h->ev_pool[4 * i + 1], h->ev_pool[4 * i + 2]));
        HIPCHK(hipEventElapsedTime(&t3, h->ev_pool[4 * i + 2], h->ev_pool[4 * i + 3]));
        a += t1;
        b += t2;
        c += t3;
    }
    *emu_ms = a;
    *render_ms = b;
    *reward_ms = c;
    *steps = n;
    h->ev_used = 0;
    return 0;
}

// Environment.reset(max_episode_steps, reward_scale) (environment.py:1233, :1258-1259): the episode
// length and reward scale of the following steps.  When the new episode length needs a larger
// seen-coordinate set, every env's current-episode entries are re-inserted into the larger table
// (pk_seen_rehash_kernel), so envs that are not reset keep their seen coordinates.
int pk_set_episode_params(pk_handle* h, uint32_t max_episode_steps, double reward_scale) {
    if (!h) return fail(-EINVAL, "null handle");
    if (max_episode_steps == 0) return fail(-EINVAL, "max_episode_steps must be > 0");
    HIPCHK(hipSetDevice(h->device));
    uint32_t need = 10;
    while ((1ull << need) * 3 < ((uint64_t)max_episode_steps + 2) * 4) need++;
    // with the reward stack the seen set grows; the trajectory rows follow its capacity, or without
    // a seen set keep cap >= max_episode_steps alone.  Everything new is staged and replaces the old
    // buffers at the commit, so a failure leaves the handle as it was
    if (need > h->cap_log2 && ((h->flags & PK_F_REWARD) || h->traj_cap)) {
        HIPCHK(hipDeviceSynchronize());
        Stage st(h);
        int rc;
        // new rows for the envs, every one flagged PK_TRAJ_BROKEN (its actions stay behind), and for
        // the slots where the bank has them (their episode parts are emptied below; generic parts
        // stay, so those rows are flagged too)
        if (h->traj_cap && (rc = traj_stage_envs(st, h, traj_cap_of(need), std::vector<uint32_t>(h->npad, PK_TRAJ_BROKEN))))
            return rc;
        if (h->traj_cap && h->bt_act && (rc = traj_stage_slots(st, h, traj_cap_of(need), h->gep_parts ? PK_TRAJ_BROKEN : 0u)))
            return rc;
        if (h->flags & PK_F_REWARD) {
            const size_t bytes = (size_t)h->npad * (1ull << need) * 4;
            st.want(h->seen, bytes, 0);
            if (st.run() != hipSuccess)
                return st.oom ? fail(-ENOMEM, "hipMalloc(%zu) for the seen set", bytes) : fail(-EIO, "hipMemset failed");
            hipError_t e = pk_launch_seen_rehash(h->seen, h->cap_log2, st.staged(h->seen), need, h->rs, h->n, h->npad, nullptr);
            if (e == hipSuccess) e = hipDeviceSynchronize();
            if (e != hipSuccess) return fail(-EIO, "seen-set rehash: %s", hipGetErrorString(e));
            if (h->b_ep_filled) {
                // the slots' seen tables follow the envs' size: reallocated, and every episode part
                // marked empty (a resume from an older checkpoint is then a reject)
                const size_t eb = (size_t)h->bank_n * (1ull << need) * 4;
                st.want(h->e_seen, eb, 0);
                e = st.run();
                if (e == hipSuccess) e = hipMemset(h->b_ep_filled, 0, h->bank_n);
                if (e == hipSuccess) e = hipDeviceSynchronize();
                if (e != hipSuccess) {
                    (void)hipGetLastError();
                    return fail(-ENOMEM, "episode parts of %u slots at the larger seen set (%zu bytes): %s", h->bank_n, eb,
                                hipGetErrorString(e));
                }
            }
        }
        st.commit();
        h->cap_log2 = need;
        if (h->traj_cap) h->traj_cap = traj_cap_of(need);
    }
    h->max_steps = max_episode_steps;
    h->reward_scale = reward_scale;
    return 0;
}

// diagnostic: the K1 phase-cycle counters of a -DPK_STAMP build (zeros otherwise), then reset
int pk_debug_counters(pk_handle* h, uint64_t* out, uint32_t n) {
    if (!h || !out) return fail(-EINVAL, "null argument");
    memset(out, 0, (size_t)n * 8);
    if (!h->dbg) return 0;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, h->dbg, (size_t)(n < PK_DBG_WORDS ? n : PK_DBG_WORDS) * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(h->dbg, 0, PK_DBG_WORDS * 8));
    return 0;
}

int pk_last_instr_count(pk_handle* h, uint64_t* out) {
    if (!h || !out) return fail(-EINVAL, "null argument");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    std::vector<uint32_t> v(h->n);
    HIPCHK(hipMemcpy(v.data(), h->regs + (size_t)PK_R_ICOUNT * h->npad, (size_t)h->n * 4, hipMemcpyDeviceToHost));
    uint64_t s = 0;
    for (uint32_t x : v) s += x;
    *out = s;
    return 0;
}

int pk_launch_shape(pk_handle* h, uint32_t env0, uint32_t count, uint32_t* out5) {
    int rc;
    if (!out5) return fail(-EINVAL, "null argument");
    if ((rc = check_range(h, env0, count))) return rc;
    const PkStepArgs a = step_args(h, nullptr, env0, env0 + count);
    out5[0] = a.small;
    out5[1] = a.wave_lanes;
    out5[2] = a.block;
    out5[3] = a.prio;
    out5[4] = a.all_staged;
    return 0;
}

// ---- savestate bank -------------------------------------------------------------------------

static int require_bank(const pk_handle* h) {
    if (!h->bank_n) return fail(-ENOENT, "the handle has no bank (pk_bank_create)");
    return 0;
}

int pk_bank_create(pk_handle* h, uint32_t n_slots) {
    if (!h) return fail(-EINVAL, "null handle");
    if (h->bank_n) return fail(-EEXIST, "the handle already has a bank of %u slots", h->bank_n);
    if (n_slots == 0 || n_slots > PK_BANK_MAX_SLOTS) return fail(-EINVAL, "n_slots must be 1..%u", PK_BANK_MAX_SLOTS);
    HIPCHK(hipSetDevice(h->device));
    const size_t lists = (2 * (size_t)h->ngroups + 2 * (size_t)h->npad) * 4;
    Stage st(h);
    st.want(h->b_mem, (size_t)n_slots * PK_PHYS);
    st.want(h->b_regs, (size_t)n_slots * PK_BANK_REGS * 4);
    st.want(h->b_lat, (size_t)n_slots * 3 * PK_ROWS * 4);
    st.want(h->b_screen, (size_t)n_slots * PK_SCREEN);
    st.want(h->b_filled, n_slots, 0);
    st.want(h->b_rejects, 4, 0);
    st.want(h->b_lists, lists, 0);
    st.want(h->b_src, (size_t)h->npad * 4, 0xFF);
    if (hipError_t e = st.run()) {
        if (st.oom)
            return fail(-ENOMEM, "bank of %u slots (%zu bytes each): %s", n_slots,
                        (size_t)PK_PHYS + PK_BANK_REGS * 4 + 3 * PK_ROWS * 4 + PK_SCREEN, hipGetErrorString(e));
        return fail(-EIO, "bank setup failed: %s", hipGetErrorString(e));
    }
    st.commit();
    h->bank_n = n_slots;
    return 0;
}

uint32_t pk_bank_slots(const pk_handle* h) { return h ? h->bank_n : 0; }

static int check_bank(pk_handle* h, uint32_t slot) {
    if (!h) return fail(-EINVAL, "null handle");
    if (require_bank(h)) return -ENOENT;
    if (slot >= h->bank_n) return fail(-EINVAL, "slot %u out of range (%u slots)", slot, h->bank_n);
    return 0;
}

int pk_bank_put(pk_handle* h, uint32_t slot, const uint8_t* in, uint64_t len) {
    int rc;
    if ((rc = check_bank(h, slot))) return rc;
    if (!in) return fail(-EINVAL, "null argument");
    Template t;
    if ((rc = parse_v9(in, len, t))) return rc;
    uint32_t regs[PK_BANK_REGS] = {0};
    memcpy(regs, t.regs, sizeof t.regs);
    const uint8_t one = 1;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(h->b_mem + (size_t)slot * PK_PHYS, t.mem.data(), PK_PHYS, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->b_regs + (size_t)slot * PK_BANK_REGS, regs, sizeof regs, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->b_lat + (size_t)slot * 3 * PK_ROWS, t.lat, sizeof t.lat, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->b_screen + (size_t)slot * PK_SCREEN, t.screen.data(), PK_SCREEN, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->b_filled + slot, &one, 1, hipMemcpyHostToDevice));
    if (h->b_ep_filled) HIPCHK(hipMemset(h->b_ep_filled + slot, 0, 1));   // machine state only: no episode part
    return 0;
}

int pk_bank_get(pk_handle* h, uint32_t slot, uint8_t* out, uint64_t len) {
    int rc;
    if ((rc = check_bank(h, slot))) return rc;
    if (!out) return fail(-EINVAL, "null argument");
    if (len < S_SIZE) return fail(-EINVAL, "buffer too small for a v9 state");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    uint8_t filled = 0;
    HIPCHK(hipMemcpy(&filled, h->b_filled + slot, 1, hipMemcpyDeviceToHost));
    if (!filled) return fail(-ENOENT, "slot %u is empty", slot);
    std::vector<uint8_t> mem(PK_PHYS), screen(PK_SCREEN);
    uint32_t regs[PK_BANK_REGS], lat[3 * PK_ROWS];
    HIPCHK(hipMemcpy(mem.data(), h->b_mem + (size_t)slot * PK_PHYS, PK_PHYS, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(regs, h->b_regs + (size_t)slot * PK_BANK_REGS, sizeof regs, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(lat, h->b_lat + (size_t)slot * 3 * PK_ROWS, sizeof lat, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(screen.data(), h->b_screen + (size_t)slot * PK_SCREEN, PK_SCREEN, hipMemcpyDeviceToHost));
    export_v9(h->tmpl, regs, mem.data(), lat, screen.data(), out);
    return 0;
}

// the bank lists of an env range, laid out like the reset lists (list_cnt / list_ids): counters
// [2 * (env0 / 64)] (envs) and [+1] (sub-blocks), ids from env0 — the bank's own, so a bank call
// and a reset of two ranges on two streams never share one
static PkBankArgs bank_args(pk_handle* h, uint32_t mode, const int32_t* slots, uint32_t env0, uint32_t env1) {
    PkBankArgs a;
    memset(&a, 0, sizeof a);
    a.mem = h->mem; a.regs = h->regs; a.lat = h->lat; a.screen = h->screen;
    a.b_mem = h->b_mem; a.b_regs = h->b_regs; a.b_lat = h->b_lat; a.b_screen = h->b_screen;
    a.b_filled = h->b_filled; a.b_rejects = h->b_rejects; a.b_ep_filled = h->b_ep_filled;
    a.slot_of_env = slots; a.src = h->b_src;
    a.cnt = h->b_lists + 2u * (env0 / PK_LANES);
    a.ids = h->b_lists + 2u * h->ngroups + env0;
    a.subs = h->b_lists + 2u * h->ngroups + h->npad + env0;
    a.tcnt = list_cnt(h, env0, 0); a.tids = list_ids(h, env0, 0);
    a.n_slots = h->bank_n; a.mode = mode; a.n = h->n; a.npad = h->npad; a.lat_stride = (uint32_t)h->lat_stride;
    a.env0 = env0; a.env1 = env1; a.ilv_sh = h->ilv_sh;
    return a;
}

static int bank_move(pk_handle* h, uint32_t mode, const int32_t* slots, uint32_t env0, uint32_t count, void* stream) {
    int rc;
    if ((rc = check_range(h, env0, count))) return rc;
    if (require_bank(h)) return -ENOENT;
    if (!slots) return fail(-EINVAL, "slot_of_env_dev is required");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    PkBankArgs a = bank_args(h, mode, slots, env0, env0 + count);
    HIPCHK(hipMemsetAsync(a.cnt, 0, 8, s));
    HIPCHK(pk_launch_bank_list(a, s));
    HIPCHK(pk_launch_bank_copy(a, s));
    return 0;
}

int pk_bank_save(pk_handle* h, const int32_t* slots, uint32_t env0, uint32_t count, void* stream) {
    return bank_move(h, PK_BANK_SAVE, slots, env0, count, stream);
}

int pk_bank_load(pk_handle* h, const int32_t* slots, uint32_t env0, uint32_t count, void* stream) {
    int rc = bank_move(h, PK_BANK_LOAD, slots, env0, count, stream);
    if (rc) return rc;
    // the envs that took a slot's machine (the call's own list) no longer follow from their actions
    return traj_mark(h, h->b_lists + 2u * (env0 / PK_LANES), h->b_lists + 2u * h->ngroups + env0, env0, env0 + count,
                     (hipStream_t)stream);
}

// template_reset with a slot per env: the selected envs with a usable slot reload from it (bank
// lists), the others from the handle's template — through the range's own reset list, which
// pk_bank_list_kernel fills in pk_list_kernel's place (same range, same stream as any other reset
// of the range)
static int bank_reset(pk_handle* h, const uint8_t* sel, const int32_t* slots, uint32_t env0, uint32_t env1, void* stream) {
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    PkBankArgs b = bank_args(h, PK_BANK_RESET, slots, env0, env1);
    b.sel = sel;
    HIPCHK(hipMemsetAsync(b.cnt, 0, 8, s));
    HIPCHK(hipMemsetAsync(b.tcnt, 0, 4, s));
    HIPCHK(pk_launch_bank_list(b, s));
    HIPCHK(pk_launch_reset(reset_args(h, env0, env1), s));   // the range's reset list: b.tcnt, b.tids
    HIPCHK(pk_launch_bank_copy(b, s));
    return 0;
}

// The one reset of the masked envs of a range, behind pk_reset_range and pk_reset_from.  Without
// slots the envs reload the template and their trajectories start at it; with slots they reload
// through bank_reset, and the trajectory origin is the slot pk_bank_list_kernel validated (b_src:
// -1 for the template, a rejected slot included).  With the reward stack the reload list is
// rreset_pre's (the env's first reset only, or always with PK_F_RELOAD_ON_RESET), and the reset
// ends with the observation of the masked envs.
static int reset_envs(pk_handle* h, uint32_t env0, uint32_t count, const uint8_t* mask, const int32_t* slots, void* stream) {
    int rc;
    if ((rc = check_range(h, env0, count))) return rc;
    if (slots && require_bank(h)) return -ENOENT;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const uint32_t env1 = env0 + count;
    const bool reward = (h->flags & PK_F_REWARD) != 0;
    const uint8_t* reload = reward ? h->reload : nullptr;
    PkRewardArgs r = reward_args(h, env0, env1);
    r.env_mask = mask;
    if (reward) HIPCHK(pk_launch_rreset_pre(r, s));
    const uint8_t* sel = reward ? reload : mask;
    if ((rc = slots ? bank_reset(h, sel, slots, env0, env1, stream) : template_reset(h, sel, env0, env1, stream))) return rc;
    if (reward) HIPCHK(pk_launch_rreset_post(r, s));
    if ((rc = traj_reset(h, mask, reload, slots ? h->b_src : nullptr, env0, env1, s))) return rc;
    if (!reward) return 0;
    // the observation of the reset envs only (list of the masked envs)
    HIPCHK(hipMemsetAsync(list_cnt(h, env0, 1), 0, 4, s));
    HIPCHK(pk_launch_list(mask, env0, env1, list_cnt(h, env0, 1), list_ids(h, env0, 1), s));
    r.ocnt = list_cnt(h, env0, 1);
    r.oids = list_ids(h, env0, 1);
    HIPCHK(pk_launch_obs(r, s));
    return 0;
}

int pk_reset_from(pk_handle* h, uint32_t env0, uint32_t count, const uint8_t* mask, const int32_t* slots, void* stream) {
    return reset_envs(h, env0, count, mask, slots, stream);
}

// ---- episode checkpoints in the bank ----------------------------------------------------------

int pk_bank_has_episodes(const pk_handle* h) { return (h && h->b_ep_filled) ? 1 : 0; }

int pk_bank_enable_episodes(pk_handle* h) {
    if (!h) return fail(-EINVAL, "null handle");
    if (require_bank(h)) return -ENOENT;
    if (!(h->flags & PK_F_REWARD)) return fail(-ENOTSUP, "episode checkpoints need the reward stack (PK_F_REWARD)");
    if (h->b_ep_filled) return fail(-EEXIST, "the bank already carries episode parts");
    static_assert(PK_NREGS <= PK_EP_RSD - PK_EP_REGS, "episode record layout");
    HIPCHK(hipSetDevice(h->device));
    const size_t K = h->bank_n, seen = K * (1ull << h->cap_log2) * 4;
    Stage st(h);
    int rc;
    // on a handle with trajectories the slots carry a trajectory part from the start
    if (h->traj_cap && (rc = traj_stage_slots(st, h, h->traj_cap, 0u))) return rc;
    st.want(h->e_fields, K * PK_EP_WORDS * 4, 0);
    st.want(h->e_seen, seen, 0);
    st.want(h->e_mask, K * PK_MASK_WORDS * 4, 0);
    st.want(h->e_cutc, K * PK_CUTC_CAP * 4, 0);
    st.want(h->b_ep_filled, K, 0);
    if (hipError_t e = st.run())
        return fail(-ENOMEM, "episode parts of %zu slots (%zu bytes each): %s", K,
                    (size_t)(seen / K) + (PK_MASK_WORDS + PK_CUTC_CAP + PK_EP_WORDS) * 4 + 1, hipGetErrorString(e));
    st.commit();
    return 0;
}

// ---- generic episode parts: checkpoints without the reward stack -------------------------------

static uint32_t gep_mpad(const pk_handle* h, uint32_t parts) { return (parts & PK_GEP_PROBES) ? (h->pr_m + 3u) / 4u * 4u : 0u; }
static uint32_t gep_row(const pk_handle* h, uint32_t parts) {
    return (parts & PK_GEP_STACK) ? h->fs_depth * (PK_SCREEN / (h->fs_scale * h->fs_scale)) : 0u;
}

uint32_t pk_bank_generic_parts(const pk_handle* h) { return h ? h->gep_parts : 0; }

uint64_t pk_bank_generic_episode_bytes(const pk_handle* h) {
    if (!h || !h->gep_parts) return 0;
    return (uint64_t)PK_GEP_REGS * 4u + (uint64_t)gep_mpad(h, h->gep_parts) * 4u + gep_row(h, h->gep_parts);
}

int pk_bank_enable_generic_episodes(pk_handle* h, uint32_t parts) {
    if (!h) return fail(-EINVAL, "null handle");
    if (h->flags & PK_F_REWARD)
        return fail(-ENOTSUP, "generic episode parts are for handles without the reward stack (pk_bank_enable_episodes)");
    if (require_bank(h)) return -ENOENT;
    if (parts & ~(PK_GEP_PROBES | PK_GEP_STACK)) return fail(-EINVAL, "unknown parts 0x%x", parts);
    if ((parts & PK_GEP_PROBES) && !h->pr_m) return fail(-ENOENT, "PK_GEP_PROBES: the handle has no probe program (pk_probe_create)");
    if ((parts & PK_GEP_STACK) && !h->fs_depth) return fail(-ENOENT, "PK_GEP_STACK: the handle has no frame stack (pk_fstack_create)");
    if (h->b_ep_filled) return fail(-EEXIST, "the bank already carries episode parts");
    static_assert(PK_GEP_REGS % 4u == 0u && PK_GEP_REGS >= PK_NREGS && PK_GEP_REGS <= 64u && PK_PROBE_MAX <= 64u &&
                  PK_SCREEN % 256u == 0u, "generic episode part layout");
    HIPCHK(hipSetDevice(h->device));
    const size_t K = h->bank_n, rb = K * PK_GEP_REGS * 4, pb = K * gep_mpad(h, parts) * 4, sb = K * gep_row(h, parts);
    Stage st(h);
    int rc;
    // on a handle with trajectories the slots carry a trajectory part from the start
    if (h->traj_cap && (rc = traj_stage_slots(st, h, h->traj_cap, 0u))) return rc;
    st.want(h->g_regs, rb, 0);
    st.want(h->g_probe, pb, 0);
    st.want(h->g_stack, sb, 0);
    st.want(h->b_ep_filled, K, 0);
    if (hipError_t e = st.run())
        return fail(-ENOMEM, "generic episode parts of %zu slots (%zu bytes each): %s", K, (rb + pb + sb) / K + 1,
                    hipGetErrorString(e));
    st.commit();
    h->gep_parts = parts | 0x80000000u;
    return 0;
}

// pk_bank_save / pk_bank_load with ep set (the same lists, validation and launches), then the
// episode mover over the same list, and for a resume the observation of the listed envs
static int episode_move(pk_handle* h, uint32_t mode, const int32_t* slots, uint32_t env0, uint32_t count, void* stream) {
    int rc;
    if ((rc = check_range(h, env0, count))) return rc;
    if (require_bank(h)) return -ENOENT;
    if (!h->b_ep_filled) return fail(-ENOENT, "the bank carries no episode parts (pk_bank_enable_episodes)");
    if (!slots) return fail(-EINVAL, "slot_of_env_dev is required");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    PkBankArgs a = bank_args(h, mode, slots, env0, env0 + count);
    a.ep = 1;
    HIPCHK(hipMemsetAsync(a.cnt, 0, 8, s));
    HIPCHK(pk_launch_bank_list(a, s));
    HIPCHK(pk_launch_bank_copy(a, s));
    const uint32_t save = mode == PK_BANK_SAVE ? 1u : 0u;
    if (h->gep_parts) {
        // no reward stack: the generic mover over the same list
        PkGepArgs g;
        memset(&g, 0, sizeof g);
        g.regs = h->regs; g.g_regs = h->g_regs;
        if (h->gep_parts & PK_GEP_PROBES) { g.state = h->pr_state; g.g_probe = h->g_probe; g.m = h->pr_m; }
        if (h->gep_parts & PK_GEP_STACK) { g.stack = h->fs_stack; g.g_stack = h->g_stack; }
        g.mpad = gep_mpad(h, h->gep_parts); g.row16 = gep_row(h, h->gep_parts) / 16u;
        g.cnt = a.cnt; g.ids = a.ids; g.src = a.src;
        g.npad = h->npad; g.save = save; g.items = count;
        HIPCHK(pk_launch_gep_move(g, s));
    } else {
        PkEpArgs p;
        memset(&p, 0, sizeof p);
        p.regs = h->regs; p.rs = h->rs; p.rsd = h->rsd; p.seen = h->seen; p.mask = h->mask; p.cutc = h->cutc;
        p.e_fields = h->e_fields; p.e_seen = h->e_seen; p.e_mask = h->e_mask; p.e_cutc = h->e_cutc;
        p.cnt = a.cnt; p.ids = a.ids; p.src = a.src;
        p.npad = h->npad; p.nregs = PK_NREGS; p.cap_log2 = h->cap_log2; p.save = save;
        p.items = count;
        HIPCHK(pk_launch_ep_move(p, s));
    }
    if (h->traj_cap) {
        // the trajectory part over the same list; a resumed env's step counter is the slot's by now
        PkTrajArgs t = traj_args(h, env0, env0 + count);
        t.cnt = a.cnt; t.ids = a.ids; t.src = a.src;
        t.save = save; t.items = count;
        HIPCHK(pk_launch_traj_move(t, s));
    }
    // with the reward stack a resume rebuilds the observation of the listed envs
    if (!h->gep_parts && mode == PK_BANK_LOAD) {
        PkRewardArgs r = reward_args(h, env0, env0 + count);
        r.ocnt = a.cnt;
        r.oids = a.ids;
        HIPCHK(pk_launch_obs(r, s));
    }
    return 0;
}

int pk_bank_checkpoint(pk_handle* h, const int32_t* slots, uint32_t env0, uint32_t count, void* stream) {
    return episode_move(h, PK_BANK_SAVE, slots, env0, count, stream);
}

int pk_bank_resume(pk_handle* h, const int32_t* slots, uint32_t env0, uint32_t count, void* stream) {
    return episode_move(h, PK_BANK_LOAD, slots, env0, count, stream);
}

int pk_bank_rejects(pk_handle* h, uint64_t* out) {
    if (!h || !out) return fail(-EINVAL, "null argument");
    if (require_bank(h)) return -ENOENT;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    uint32_t v = 0;
    HIPCHK(hipMemcpy(&v, h->b_rejects, 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(h->b_rejects, 0, 4));
    *out = v;
    return 0;
}

// ---- exploration archive on the bank -----------------------------------------------------------

static uint32_t pow2_at_least(uint64_t v) {
    uint32_t p = 64;
    while (p < v) p <<= 1;
    return p;
}

// the persistent block: [hdr | a_key | a_score | prefix | i_key] u64, [a_len | a_visits | a_picks |
// i_cell | tgt | map] u32, [flag] u8
static size_t arch_fix_bytes(uint32_t cells, uint32_t isize, uint32_t npad) {
    return ((size_t)PK_AH_WORDS + 3ull * cells + isize) * 8 + (3ull * cells + isize + 2ull * npad) * 4 + npad;
}

// the argument block of an archive call over [env0, env1): the per-call blocks are carved for a
// scratch table of ssize entries
static PkArchArgs arch_args(pk_handle* h, uint32_t env0, uint32_t env1, uint32_t ssize) {
    PkArchArgs a;
    memset(&a, 0, sizeof a);
    const uint32_t K = h->arch_cells, I = h->arch_imask + 1u;
    uint64_t* q = (uint64_t*)h->a_fix;
    a.hdr = q; q += PK_AH_WORDS;
    a.a_key = q; q += K;
    a.a_score = (double*)q; q += K;
    a.prefix = q; q += K;
    a.i_key = q; q += I;
    uint32_t* w = (uint32_t*)q;
    a.a_len = w; w += K;
    a.a_visits = w; w += K;
    a.a_picks = w; w += K;
    a.i_cell = w; w += I;
    a.tgt = w; w += h->npad;
    a.map = (int32_t*)w; w += h->npad;
    a.flag = (uint8_t*)w;
    q = (uint64_t*)h->a_ones;
    a.c_le = q; q += K;
    a.s_key = q; q += ssize;
    a.s_le = q; q += ssize;
    a.s_first = (uint32_t*)q;
    q = (uint64_t*)h->a_zero;
    a.c_max = q; q += K;
    a.s_max = q; q += ssize;
    a.s_cnt = (uint32_t*)q;
    a.s_cell = a.s_cnt + ssize;
    a.time_reg = h->regs + (size_t)PK_R_TIME * h->npad;
    a.b_rejects = h->b_rejects;
    a.src = h->b_src;
    a.seed = h->arch_seed;
    a.i_mask = h->arch_imask; a.s_mask = ssize - 1u;
    a.n_cells = K; a.slot0 = h->arch_slot0;
    a.env0 = env0; a.env1 = env1;
    if (h->x_fix) {   // an update marks the cells whose record it replaces
        a.x_sent_visits = (uint32_t*)h->x_fix;
        a.x_sent_picks = a.x_sent_visits + K;
        a.x_dirty = a.x_sent_picks + K;
    }
    return a;
}

uint32_t pk_archive_cells(const pk_handle* h) { return h ? h->arch_cells : 0; }

int pk_archive_create(pk_handle* h, uint32_t slot0, uint32_t n_cells, uint64_t seed) {
    if (!h) return fail(-EINVAL, "null handle");
    if (h->arch_cells) return fail(-EEXIST, "the handle already has an archive of %u cells", h->arch_cells);
    if (!h->bank_n || !h->b_ep_filled)
        return fail(-ENOENT, "an archive needs a bank with episode parts (pk_bank_create, pk_bank_enable_episodes)");
    if (n_cells == 0 || n_cells > PK_ARCH_MAX_CELLS || (uint64_t)slot0 + n_cells > h->bank_n)
        return fail(-EINVAL, "cells [%u, +%u): n_cells must be 1..%u and the slots inside the bank's %u", slot0, n_cells,
                    PK_ARCH_MAX_CELLS, h->bank_n);
    HIPCHK(hipSetDevice(h->device));
    const uint32_t I = pow2_at_least(2ull * n_cells), S = pow2_at_least(2ull * h->npad);
    const size_t fix = arch_fix_bytes(n_cells, I, h->npad);
    const size_t ones = ((size_t)n_cells + 2ull * S) * 8 + (size_t)S * 4, zero = ((size_t)n_cells + S) * 8 + 2ull * S * 4;
    Stage st(h);
    st.want(h->a_fix, fix, 0);
    // no cell has a key yet, the index is empty
    st.fill(h->a_fix, PK_AH_WORDS * 8, (size_t)n_cells * 8, 0xFF);
    st.fill(h->a_fix, ((size_t)PK_AH_WORDS + 3ull * n_cells) * 8, (size_t)I * 8, 0xFF);
    st.want(h->a_ones, ones);
    st.want(h->a_zero, zero);
    if (hipError_t e = st.run())
        return fail(-ENOMEM, "archive of %u cells (%zu bytes): %s", n_cells, fix + ones + zero, hipGetErrorString(e));
    st.commit();
    h->arch_cells = n_cells; h->arch_slot0 = slot0; h->arch_imask = I - 1u; h->arch_seed = seed;
    return 0;
}

int pk_cell_keys(pk_handle* h, uint32_t shift, uint64_t* keys, uint32_t env0, uint32_t count, void* stream) {
    int rc;
    if ((rc = check_range(h, env0, count))) return rc;
    if (!keys) return fail(-EINVAL, "keys_dev is required");
    if (shift > 7) return fail(-EINVAL, "shift must be 0..7");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(pk_launch_cell_keys(h->mem, h->ilv_sh, shift, keys, env0, env0 + count, (hipStream_t)stream));
    return 0;
}

uint32_t pk_frame_cells(uint32_t bw, uint32_t bh) {
    if (!bw || !bh || bw % 8u || bh % 8u || PK_COLS % bw || PK_ROWS % bh) return 0;
    return (PK_COLS / bw) * (PK_ROWS / bh);
}

int pk_frame_keys(pk_handle* h, uint32_t bw, uint32_t bh, uint32_t levels, const uint8_t* screen, const uint64_t* salt,
                  uint64_t* keys, uint8_t* cells, uint32_t env0, uint32_t count, void* stream) {
    int rc;
    if ((rc = check_range(h, env0, count))) return rc;
    if (!pk_frame_cells(bw, bh))
        return fail(-EINVAL, "blocks of %u x %u: bw must be a multiple of 8 that divides 160, bh one that divides 144", bw, bh);
    if (levels < 2 || levels > 256) return fail(-EINVAL, "levels must be 2..256");
    if (!keys) return fail(-EINVAL, "keys_dev is required");
    if (!screen && !(h->flags & PK_F_RENDER))
        return fail(-ENOTSUP, "the handle renders no screen (PK_F_RENDER): pass screen_dev");
    if ((uintptr_t)screen % 16u) return fail(-EINVAL, "screen_dev must be 16-byte aligned");
    HIPCHK(hipSetDevice(h->device));
    PkCellArgs a;
    a.screen = screen ? screen : h->screen; a.salt = salt; a.keys = keys; a.cells = cells;
    a.env0 = env0; a.env1 = env0 + count; a.bw = bw; a.bh = bh; a.levels = levels;
    HIPCHK(pk_launch_frame_keys(a, (hipStream_t)stream));
    return 0;
}

// ---- frame stack --------------------------------------------------------------------------------

uint32_t pk_fstack_depth(const pk_handle* h) { return h ? h->fs_depth : 0; }
uint32_t pk_fstack_scale(const pk_handle* h) { return h && h->fs_depth ? h->fs_scale : 0; }
uint8_t* pk_fstack_ptr(pk_handle* h) { return h ? h->fs_stack : nullptr; }

int pk_fstack_create(pk_handle* h, uint32_t scale, uint32_t depth, uint32_t layout, uint32_t mode) {
    if (!h) return fail(-EINVAL, "null handle");
    if (h->fs_depth) return fail(-EEXIST, "the handle already has a frame stack of depth %u", h->fs_depth);
    if (scale != 1 && scale != 2 && scale != 4) return fail(-EINVAL, "scale must be 1, 2 or 4");
    if (layout != PK_FSTACK_CHW && layout != PK_FSTACK_HWC) return fail(-EINVAL, "unknown layout %u", layout);
    if (mode != PK_FSTACK_MEAN && mode != PK_FSTACK_PICK) return fail(-EINVAL, "unknown mode %u", mode);
    if (depth == 0 || depth > PK_FS_MAX_DEPTH) return fail(-EINVAL, "depth must be 1..%u", PK_FS_MAX_DEPTH);
    if (layout == PK_FSTACK_HWC && (depth & (depth - 1u))) return fail(-EINVAL, "depth must be 1, 2, 4 or 8 with PK_FSTACK_HWC");
    HIPCHK(hipSetDevice(h->device));
    const size_t bytes = (size_t)h->n * depth * (PK_SCREEN / (scale * scale));
    Stage st(h);
    st.want(h->fs_stack, bytes, 0);
    if (hipError_t e = st.run())
        return fail(-ENOMEM, "frame stack of depth %u at scale %u (%zu bytes): %s", depth, scale, bytes, hipGetErrorString(e));
    st.commit();
    h->fs_scale = scale; h->fs_depth = depth; h->fs_layout = layout; h->fs_mode = mode;
    return 0;
}

int pk_fstack_push(pk_handle* h, const uint8_t* screen, const uint8_t* mask, uint32_t flags, uint32_t env0, uint32_t count,
                   void* stream) {
    int rc;
    if ((rc = check_range(h, env0, count))) return rc;
    if (!h->fs_depth) return fail(-ENOENT, "the handle has no frame stack (pk_fstack_create)");
    if (flags & ~PK_FSTACK_FILL_ONLY) return fail(-EINVAL, "unknown flags 0x%x", flags);
    if (!screen && !(h->flags & PK_F_RENDER))
        return fail(-ENOTSUP, "the handle renders no screen (PK_F_RENDER): pass screen_dev");
    if ((uintptr_t)screen % 16u) return fail(-EINVAL, "screen_dev must be 16-byte aligned");
    HIPCHK(hipSetDevice(h->device));
    PkStackArgs a;
    a.screen = screen ? screen : h->screen; a.mask = mask; a.stack = h->fs_stack;
    a.env0 = env0; a.env1 = env0 + count;
    a.scale = h->fs_scale; a.depth = h->fs_depth; a.layout = h->fs_layout; a.mode = h->fs_mode;
    a.fill_only = flags & PK_FSTACK_FILL_ONLY;
    HIPCHK(pk_launch_fstack(a, (hipStream_t)stream));
    return 0;
}

// ---- RAM probes ---------------------------------------------------------------------------------

uint32_t pk_probe_count(const pk_handle* h) { return h ? h->pr_m : 0; }

int pk_probe_create(pk_handle* h, const pk_probe* prog, uint32_t m) {
    if (!h || !prog) return fail(-EINVAL, "null argument");
    if (h->pr_m) return fail(-EEXIST, "the handle already has a probe program of %u probes", h->pr_m);
    if (m == 0 || m > PK_PROBE_MAX) return fail(-EINVAL, "a program has 1..%u probes, not %u", PK_PROBE_MAX, m);
    for (uint32_t j = 0; j < m; j++) {
        const pk_probe& p = prog[j];
        if (p.kind > PK_PV_BITS) return fail(-EINVAL, "probe %u: unknown kind %u", j, p.kind);
        if (p.reduce > PK_PR_MAX) return fail(-EINVAL, "probe %u: unknown reduce %u", j, p.reduce);
        if (p.op > PK_PO_CHANGE) return fail(-EINVAL, "probe %u: unknown op %u", j, p.op);
        if (p.cmp > PK_PC_LE) return fail(-EINVAL, "probe %u: unknown cmp %u", j, p.cmp);
        const uint32_t max_len = p.kind == PK_PV_BITS ? 512u : 3u;
        if (p.len == 0 || p.len > max_len) return fail(-EINVAL, "probe %u: len %u is outside 1..%u", j, p.len, max_len);
        if (p.count == 0 || p.count > PK_PROBE_MAX) return fail(-EINVAL, "probe %u: count %u is outside 1..%u", j, p.count, PK_PROBE_MAX);
        if (!(p.weight - p.weight == 0.0)) return fail(-EINVAL, "probe %u: the weight is not finite", j);
        for (uint32_t k = 0; k < p.count; k++) {     // pk_get_ram's rule, per element
            const uint32_t a = (uint32_t)p.addr + k * (uint32_t)p.stride, len = p.len;
            const bool wram = a >= 0xC000 && a + len <= 0xFE00, hram = a >= 0xFF80 && a + len <= 0xFFFF;
            if (!(wram || hram))
                return fail(-EINVAL, "probe %u element %u: [0x%04x, +%u) is not inside WRAM/echo or HRAM", j, k, a, len);
            if (wram && (a & 0x1FFF) + len > 0x2000)
                return fail(-EINVAL, "probe %u element %u: [0x%04x, +%u) wraps the echo mirror", j, k, a, len);
        }
    }
    HIPCHK(hipSetDevice(h->device));
    const size_t pbytes = (size_t)m * sizeof(pk_probe), sbytes = (size_t)m * h->npad * 4;
    Stage st(h);
    st.want(h->pr_prog, pbytes, -1, prog);
    st.want(h->pr_state, sbytes, 0);
    if (hipError_t e = st.run())
        return fail(-ENOMEM, "probe program of %u probes (%zu bytes of state): %s", m, sbytes, hipGetErrorString(e));
    st.commit();
    h->pr_m = m;
    return 0;
}

int pk_probe_eval(pk_handle* h, const uint8_t* mask, uint32_t flags, uint32_t env0, uint32_t count, double* rew,
                  uint8_t* term, int32_t* feat, void* stream) {
    int rc;
    if ((rc = check_range(h, env0, count))) return rc;
    if (!h->pr_m) return fail(-ENOENT, "the handle has no probe program (pk_probe_create)");
    if (flags & ~(PK_PROBE_REBASE_ONLY | PK_PROBE_SET)) return fail(-EINVAL, "unknown flags 0x%x", flags);
    HIPCHK(hipSetDevice(h->device));
    PkProbeArgs a;
    a.mem = h->mem; a.prog = h->pr_prog; a.state = h->pr_state;
    a.mask = mask; a.rew = rew; a.term = term; a.feat = feat;
    a.m = h->pr_m; a.npad = h->npad; a.env0 = env0; a.env1 = env0 + count; a.ilv_sh = h->ilv_sh;
    a.rebase_only = flags & PK_PROBE_REBASE_ONLY; a.set = (flags & PK_PROBE_SET) ? 1u : 0u;
    HIPCHK(pk_launch_probe(a, (hipStream_t)stream));
    return 0;
}

// ---- tile view ----------------------------------------------------------------------------------

uint32_t pk_tiles_planes(const pk_handle* h) { return h ? h->tl_planes : 0; }
uint16_t* pk_tiles_ptr(pk_handle* h) { return h ? h->tl_out : nullptr; }

int pk_tiles_create(pk_handle* h, uint32_t mode, uint32_t bits, uint32_t flags) {
    if (!h) return fail(-EINVAL, "null handle");
    if (h->tl_planes) return fail(-EEXIST, "the handle already has a tile view of %u planes", h->tl_planes);
    if (mode != PK_TILES_ID && mode != PK_TILES_HASH) return fail(-EINVAL, "unknown tile view mode %u", mode);
    if (mode == PK_TILES_HASH && (bits < 8 || bits > 15)) return fail(-EINVAL, "PK_TILES_HASH takes bits in 8..15, not %u", bits);
    if (flags & ~PK_TILES_OBJ) return fail(-EINVAL, "unknown flags 0x%x", flags);
    HIPCHK(hipSetDevice(h->device));
    const uint32_t planes = (flags & PK_TILES_OBJ) ? 2u : 1u;
    const size_t bytes = (size_t)h->n * planes * PK_TILE_CELLS * sizeof(uint16_t);
    Stage st(h);
    st.want(h->tl_out, bytes, 0xFF);
    if (hipError_t e = st.run())
        return fail(-ENOMEM, "tile view of %u planes (%zu bytes): %s", planes, bytes, hipGetErrorString(e));
    st.commit();
    h->tl_planes = planes; h->tl_bits = mode == PK_TILES_HASH ? bits : 0u;
    return 0;
}

int pk_tiles_eval(pk_handle* h, const uint8_t* mask, const uint64_t* salt, uint64_t* keys, uint32_t env0, uint32_t count,
                  void* stream) {
    int rc;
    if ((rc = check_range(h, env0, count))) return rc;
    if (!h->tl_planes) return fail(-ENOENT, "the handle has no tile view (pk_tiles_create)");
    HIPCHK(hipSetDevice(h->device));
    PkTilesArgs a;
    a.mem = h->mem; a.regs = h->regs; a.mask = mask; a.salt = salt; a.keys = keys; a.out = h->tl_out;
    a.npad = h->npad; a.env0 = env0; a.env1 = env0 + count; a.ilv_sh = h->ilv_sh;
    a.planes = h->tl_planes; a.bits = h->tl_bits;
    HIPCHK(pk_launch_tiles(a, (hipStream_t)stream));
    return 0;
}

int pk_archive_update(pk_handle* h, const uint64_t* keys, const double* scores, const uint8_t* mask, uint32_t env0,
                      uint32_t count, int32_t* slot_out, void* stream) {
    int rc;
    if ((rc = check_range(h, env0, count))) return rc;
    if (!h->arch_cells) return fail(-ENOENT, "the handle has no archive (pk_archive_create)");
    if (!keys || !scores) return fail(-EINVAL, "keys_dev and scores_dev are required");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const uint32_t S = pow2_at_least(2ull * count);
    PkArchArgs a = arch_args(h, env0, env0 + count, S);
    a.keys = keys; a.scores = scores; a.mask = mask; a.out = slot_out;
    HIPCHK(hipMemsetAsync(h->a_ones, 0xFF, ((size_t)a.n_cells + 2ull * S) * 8 + (size_t)S * 4, s));
    HIPCHK(hipMemsetAsync(h->a_zero, 0, ((size_t)a.n_cells + S) * 8 + (size_t)S * 4, s));
    HIPCHK(pk_launch_arch_update(a, s));
    if ((rc = episode_move(h, PK_BANK_SAVE, a.map, env0, count, stream))) return rc;
    if (slot_out) HIPCHK(pk_launch_arch_out(a, s));
    return 0;
}

int pk_archive_explore(pk_handle* h, const uint8_t* mask, uint32_t env0, uint32_t count, int32_t* slot_out, void* stream) {
    int rc;
    if ((rc = check_range(h, env0, count))) return rc;
    if (!h->arch_cells) return fail(-ENOENT, "the handle has no archive (pk_archive_create)");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    PkArchArgs a = arch_args(h, env0, env0 + count, 64);
    a.mask = mask; a.out = slot_out;
    HIPCHK(pk_launch_arch_draw(a, s));
    if ((rc = episode_move(h, PK_BANK_LOAD, a.map, env0, count, stream))) return rc;
    if (slot_out) HIPCHK(pk_launch_arch_out(a, s));
    return 0;
}

int pk_archive_read(pk_handle* h, uint32_t* used, uint64_t* keys, double* scores, uint32_t* lengths, uint32_t* visits,
                    uint32_t* picks, uint64_t* overflow) {
    if (!h) return fail(-EINVAL, "null handle");
    if (!h->arch_cells) return fail(-ENOENT, "the handle has no archive (pk_archive_create)");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    const PkArchArgs a = arch_args(h, 0, 0, 64);
    const size_t K = a.n_cells;
    uint64_t hdr[PK_AH_WORDS];
    HIPCHK(hipMemcpy(hdr, a.hdr, sizeof hdr, hipMemcpyDeviceToHost));
    if (used) *used = (uint32_t)hdr[PK_AH_USED];
    if (overflow) *overflow = hdr[PK_AH_OVERFLOW];
    if (keys) HIPCHK(hipMemcpy(keys, a.a_key, K * 8, hipMemcpyDeviceToHost));
    if (scores) HIPCHK(hipMemcpy(scores, a.a_score, K * 8, hipMemcpyDeviceToHost));
    if (lengths) HIPCHK(hipMemcpy(lengths, a.a_len, K * 4, hipMemcpyDeviceToHost));
    if (visits) HIPCHK(hipMemcpy(visits, a.a_visits, K * 4, hipMemcpyDeviceToHost));
    if (picks) HIPCHK(hipMemcpy(picks, a.a_picks, K * 4, hipMemcpyDeviceToHost));
    return 0;
}

// ---- archive exchange ---------------------------------------------------------------------------

uint32_t pk_archive_format(const pk_handle* h) {
    if (!h) return 0;
    return (PK_XCHG_VERSION << 24) | (h->traj_cap ? 1u << 23 : 0u) | ((h->cap_log2 & 0x7Fu) << 16) | (PK_PHYS & 0xFFFFu);
}

// The payload layout: the parts of a slot in their fixed order, each an array of the handle with
// one row per slot.  Machine part: RAM image, registers, latches, screen; episode part: record
// words, seen table, visited mask, cut coordinates; on a handle with trajectories the piece
// {origin, flags, 0, 0} and the action row.  Every row size is a multiple of 16.
static PkXchgArgs xchg_args(const pk_handle* h) {
    static_assert(PK_PHYS % 16u == 0u && (PK_BANK_REGS * 4u) % 16u == 0u && (3u * PK_ROWS * 4u) % 16u == 0u &&
                  PK_SCREEN % 16u == 0u && (PK_EP_WORDS * 4u) % 16u == 0u && (PK_MASK_WORDS * 4u) % 16u == 0u &&
                  (PK_CUTC_CAP * 4u) % 16u == 0u, "payload parts are whole 16-byte pieces");
    PkXchgArgs x;
    memset(&x, 0, sizeof x);
    uint32_t n = 0, off = 0;
    auto part = [&](void* base, uint32_t bytes) {
        x.base[n] = (uint8_t*)base;
        x.stride[n] = bytes;
        x.off16[n] = off;
        off += bytes / 16u;
        n++;
    };
    part(h->b_mem, PK_PHYS);
    part(h->b_regs, PK_BANK_REGS * 4u);
    part(h->b_lat, 3u * PK_ROWS * 4u);
    part(h->b_screen, PK_SCREEN);
    part(h->e_fields, PK_EP_WORDS * 4u);
    part(h->e_seen, 4u << h->cap_log2);
    part(h->e_mask, PK_MASK_WORDS * 4u);
    part(h->e_cutc, PK_CUTC_CAP * 4u);
    x.head16 = PK_ARCH_NONE;
    if (h->traj_cap) {
        x.head16 = off;
        part(nullptr, 16u);
        part(h->bt_act, h->traj_cap);
    }
    static_assert(PK_XCHG_MAX_PARTS >= 10u, "payload parts");
    x.nparts = n;
    x.off16[n] = off;
    x.pay16 = off;
    x.bt_origin = h->bt_origin; x.bt_flags = h->bt_flags;
    x.b_filled = h->b_filled; x.b_ep_filled = h->b_ep_filled;
    x.slot0 = h->arch_slot0;
    return x;
}

uint64_t pk_archive_payload_bytes(const pk_handle* h) {
    if (!h || !h->x_fix) return 0;
    return (uint64_t)xchg_args(h).pay16 * 16u;
}

// the exchange blocks: x_fix = [sent_visits | sent_picks | dirty][n_cells] [tgt | x_cell | x_pay][R]
// u32, flag u8[R]; x_ones = [c_le[n_cells] | s_key[S] | s_le[S]] u64, s_first u32[S]; x_zero = x_cnt
// (16 bytes), [c_max[n_cells] | s_max[S]] u64, [s_cnt | s_vis | s_pick | s_cell][S] u32 — R the most
// records of a merge, S the scratch table of a call (allocated for R)
static PkArchArgs xchg_arch_args(pk_handle* h, uint32_t n_records, uint32_t ssize) {
    PkArchArgs a = arch_args(h, 0, n_records, 64);
    const uint32_t K = h->arch_cells, R = PK_XCHG_MAX_RECORDS;
    uint32_t* w = a.x_dirty + K;
    a.tgt = w; w += R;
    a.x_cell = w; w += R;
    a.x_pay = w; w += R;
    a.flag = (uint8_t*)w;
    a.map = nullptr;
    uint64_t* q = (uint64_t*)h->x_ones;
    a.c_le = q; q += K;
    a.s_key = q; q += ssize;
    a.s_le = q; q += ssize;
    a.s_first = (uint32_t*)q;
    q = (uint64_t*)h->x_zero;
    a.x_cnt = (uint32_t*)q; q += 2;
    a.c_max = q; q += K;
    a.s_max = q; q += ssize;
    a.s_cnt = (uint32_t*)q;
    a.s_vis = a.s_cnt + ssize;
    a.s_pick = a.s_vis + ssize;
    a.s_cell = a.s_pick + ssize;
    a.s_mask = ssize - 1u;
    a.format = pk_archive_format(h);
    return a;
}

static size_t xchg_ones_bytes(uint32_t cells, uint32_t ssize) { return ((size_t)cells + 2ull * ssize) * 8 + (size_t)ssize * 4; }
// the cleared part of x_zero: everything but s_cell, which the rank phase writes before it is read
static size_t xchg_zero_bytes(uint32_t cells, uint32_t ssize) { return 16 + ((size_t)cells + ssize) * 8 + 3ull * ssize * 4; }

int pk_archive_exchange_enable(pk_handle* h) {
    if (!h) return fail(-EINVAL, "null handle");
    if (!h->arch_cells) return fail(-ENOENT, "the handle has no archive (pk_archive_create)");
    if (h->gep_parts) return fail(-ENOTSUP, "the exchange payload has no format for generic episode parts");
    if (h->x_fix) return fail(-EEXIST, "the archive already has its exchange words");
    HIPCHK(hipSetDevice(h->device));
    const uint32_t K = h->arch_cells, R = PK_XCHG_MAX_RECORDS, S = pow2_at_least(2ull * R);
    const size_t fix = (3ull * K + 3ull * R) * 4 + R, ones = xchg_ones_bytes(K, S), zero = xchg_zero_bytes(K, S) + (size_t)S * 4;
    Stage st(h);
    st.want(h->x_fix, fix, 0);
    st.want(h->x_ones, ones);
    st.want(h->x_zero, zero, 0);
    if (hipError_t e = st.run())
        return fail(-ENOMEM, "exchange words of %u cells (%zu bytes): %s", K, fix + ones + zero, hipGetErrorString(e));
    st.commit();
    return 0;
}

static int check_xchg(pk_handle* h) {
    if (!h) return fail(-EINVAL, "null handle");
    if (!h->arch_cells) return fail(-ENOENT, "the handle has no archive (pk_archive_create)");
    if (!h->x_fix) return fail(-ENOENT, "the archive has no exchange words (pk_archive_exchange_enable)");
    return 0;
}

int pk_archive_pack(pk_handle* h, uint32_t flags, uint32_t cell0, uint32_t count, uint32_t max_payloads, pk_xrec* rec,
                    uint8_t* payload, uint32_t* n_payloads, void* stream) {
    int rc;
    if ((rc = check_xchg(h))) return rc;
    if (flags & ~PK_XCHG_DELTA) return fail(-EINVAL, "unknown flags 0x%x", flags);
    if (count == 0 || (uint64_t)cell0 + count > h->arch_cells)
        return fail(-EINVAL, "cells [%u, +%u) are not inside the archive's %u", cell0, count, h->arch_cells);
    if (!rec || ((uintptr_t)rec & 15u)) return fail(-EINVAL, "rec_dev is required, 16-byte aligned");
    if ((!payload && max_payloads) || ((uintptr_t)payload & 15u))
        return fail(-EINVAL, "payload_dev is required for max_payloads > 0, 16-byte aligned");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    PkPackArgs p;
    memset(&p, 0, sizeof p);
    p.a = xchg_arch_args(h, 0, 64);
    p.out = rec; p.n_payloads_out = n_payloads;
    p.cell0 = cell0; p.count = count; p.max_payloads = max_payloads; p.delta = flags & PK_XCHG_DELTA;
    HIPCHK(pk_launch_xchg_pack(p, s));
    PkXchgArgs x = xchg_args(h);
    x.payload = payload;
    x.cnt = p.a.x_cnt; x.cell = p.a.x_cell; x.pay = p.a.x_pay;
    x.items = count < max_payloads ? count : max_payloads;
    HIPCHK(pk_launch_xchg_move(x, true, s));
    return 0;
}

int pk_archive_merge(pk_handle* h, const pk_xrec* rec, uint32_t n_records, const uint8_t* payload, uint32_t n_payloads,
                     int32_t* cell_out, void* stream) {
    int rc;
    if ((rc = check_xchg(h))) return rc;
    if (n_records == 0 || n_records > PK_XCHG_MAX_RECORDS) return fail(-EINVAL, "n_records must be 1..%u", PK_XCHG_MAX_RECORDS);
    if (!rec || ((uintptr_t)rec & 15u)) return fail(-EINVAL, "rec_dev is required, 16-byte aligned");
    if ((!payload && n_payloads) || ((uintptr_t)payload & 15u))
        return fail(-EINVAL, "payload_dev is required for n_payloads > 0, 16-byte aligned");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const uint32_t S = pow2_at_least(2ull * n_records);
    PkArchArgs a = xchg_arch_args(h, n_records, S);
    a.rec = rec; a.n_payloads = n_payloads; a.out = cell_out;
    HIPCHK(hipMemsetAsync(h->x_ones, 0xFF, xchg_ones_bytes(a.n_cells, S), s));
    HIPCHK(hipMemsetAsync(h->x_zero, 0, xchg_zero_bytes(a.n_cells, S), s));
    HIPCHK(pk_launch_arch_merge(a, s));
    PkXchgArgs x = xchg_args(h);
    x.payload = const_cast<uint8_t*>(payload);
    x.cnt = a.x_cnt; x.cell = a.x_cell; x.pay = a.x_pay;
    x.items = n_records < n_payloads ? n_records : n_payloads;
    HIPCHK(pk_launch_xchg_move(x, false, s));
    return 0;
}

// ---- action trajectories ------------------------------------------------------------------------

uint32_t pk_traj_capacity(const pk_handle* h) { return h ? h->traj_cap : 0; }

int pk_traj_enable(pk_handle* h) {
    if (!h) return fail(-EINVAL, "null handle");
    if (h->traj_cap) return fail(-EEXIST, "the handle already records trajectories");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    uint32_t lg = h->cap_log2;
    if (!(h->flags & PK_F_REWARD)) {
        // without a seen set nothing has kept cap_log2 up with pk_set_episode_params
        lg = 10;
        while ((1ull << lg) * 3 < ((uint64_t)h->max_steps + 2) * 4) lg++;
    }
    const uint32_t cap = traj_cap_of(lg);
    // an env that has already stepped has lost its first actions
    std::vector<uint32_t> flags(h->npad, 0u);
    HIPCHK(hipMemcpy(flags.data(), h->regs + (size_t)PK_R_TIME * h->npad, (size_t)h->npad * 4, hipMemcpyDeviceToHost));
    for (uint32_t& f : flags) f = f ? PK_TRAJ_BROKEN : 0u;
    Stage st(h);
    int rc;
    if ((rc = traj_stage_envs(st, h, cap, flags))) return rc;
    // slots that already hold an episode hold no actions for it
    if (h->b_ep_filled && (rc = traj_stage_slots(st, h, cap, PK_TRAJ_BROKEN))) return rc;
    st.commit();
    h->cap_log2 = lg;
    h->traj_cap = cap;
    return 0;
}

static int traj_get(pk_handle* h, bool slots, uint32_t i0, uint32_t count, int32_t* origin, uint32_t* len, uint8_t* flags,
                    uint8_t* actions, void* stream) {
    if ((uintptr_t)actions & 15u) return fail(-EINVAL, "actions_dev must be 16-byte aligned");
    HIPCHK(hipSetDevice(h->device));
    PkTrajArgs a = traj_args(h, i0, i0 + count);
    a.slots = slots ? 1u : 0u;
    a.o_origin = origin; a.o_len = len; a.o_flags = flags; a.o_act = actions;
    HIPCHK(pk_launch_traj_get(a, (hipStream_t)stream));
    return 0;
}

int pk_traj_get(pk_handle* h, uint32_t env0, uint32_t count, int32_t* origin, uint32_t* len, uint8_t* flags, uint8_t* actions,
                void* stream) {
    int rc;
    if ((rc = check_range(h, env0, count))) return rc;
    if (!h->traj_cap) return fail(-ENOENT, "the handle records no trajectories (pk_traj_enable)");
    return traj_get(h, false, env0, count, origin, len, flags, actions, stream);
}

int pk_bank_traj_get(pk_handle* h, uint32_t slot0, uint32_t count, int32_t* origin, uint32_t* len, uint8_t* flags,
                     uint8_t* actions, void* stream) {
    if (!h) return fail(-EINVAL, "null handle");
    if (!h->traj_cap) return fail(-ENOENT, "the handle records no trajectories (pk_traj_enable)");
    if (require_bank(h)) return -ENOENT;
    if (count == 0 || (uint64_t)slot0 + count > h->bank_n)
        return fail(-EINVAL, "slots [%u, +%u) are not inside the bank's %u", slot0, count, h->bank_n);
    return traj_get(h, true, slot0, count, origin, len, flags, actions, stream);
}

// ---- visit counts -------------------------------------------------------------------------------

static uint64_t counts_limit(uint32_t lg) { return 3ull << (lg - 2u); }

// a table of 2^lg entries in the block c_fix: header | keys | counts | sent | per-env entry words
static PkCountArgs counts_layout(uint8_t* c_fix, uint32_t lg) {
    PkCountArgs a;
    memset(&a, 0, sizeof a);
    const size_t cap = (size_t)1 << lg;
    a.hdr = (uint64_t*)c_fix;
    a.c_key = a.hdr + PK_CH_WORDS;
    a.c_cnt = a.c_key + cap;
    a.c_sent = a.c_cnt + cap;
    a.tgt = (uint32_t*)(a.c_sent + cap);
    a.c_mask = (uint32_t)(cap - 1u);
    a.limit = counts_limit(lg);
    return a;
}
static PkCountArgs counts_args(const pk_handle* h) { return counts_layout(h->c_fix, h->cnt_log2); }

static hipError_t counts_wipe(const PkCountArgs& a, hipStream_t s) {
    const size_t cap = (size_t)a.c_mask + 1u;
    hipError_t e = hipMemsetAsync(a.hdr, 0, PK_CH_WORDS * 8, s);
    if (e == hipSuccess) e = hipMemsetAsync(a.c_key, 0xFF, cap * 8, s);
    if (e == hipSuccess) e = hipMemsetAsync(a.c_cnt, 0, cap * 16, s);
    return e;
}

uint64_t pk_counts_limit(const pk_handle* h) { return h && h->cnt_log2 ? counts_limit(h->cnt_log2) : 0; }

int pk_counts_create(pk_handle* h, uint32_t cap_log2) {
    if (!h) return fail(-EINVAL, "null handle");
    if (h->cnt_log2) return fail(-EEXIST, "the handle already has a count table of 2^%u entries", h->cnt_log2);
    if (cap_log2 < PK_CNT_MIN_LOG2 || cap_log2 > PK_CNT_MAX_LOG2)
        return fail(-EINVAL, "cap_log2 must be %u..%u", PK_CNT_MIN_LOG2, PK_CNT_MAX_LOG2);
    if (counts_limit(cap_log2) < h->n)
        return fail(-EINVAL, "a table of 2^%u entries takes %llu keys, fewer than the handle's %u envs", cap_log2,
                    (unsigned long long)counts_limit(cap_log2), h->n);
    HIPCHK(hipSetDevice(h->device));
    const size_t bytes = PK_CH_WORDS * 8 + ((size_t)24 << cap_log2) + (size_t)h->npad * 4;
    Stage st(h);
    st.want(h->c_fix, bytes);
    hipError_t e = st.run();
    if (e == hipSuccess) e = counts_wipe(counts_layout(st.staged(h->c_fix), cap_log2), nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(-ENOMEM, "count table of 2^%u entries (%zu bytes): %s", cap_log2, bytes, hipGetErrorString(e));
    }
    st.commit();
    h->cnt_log2 = cap_log2;
    return 0;
}

int pk_counts_update(pk_handle* h, const uint64_t* keys, const uint8_t* mask, uint32_t env0, uint32_t count, double beta,
                     uint32_t flags, uint64_t* counts_out, double* bonus_out, void* stream) {
    int rc;
    if ((rc = check_range(h, env0, count))) return rc;
    if (!h->cnt_log2) return fail(-ENOENT, "the handle has no count table (pk_counts_create)");
    if (!keys) return fail(-EINVAL, "keys_dev is required");
    if (flags & ~PK_COUNTS_PEEK) return fail(-EINVAL, "unknown flags 0x%x", flags);
    HIPCHK(hipSetDevice(h->device));
    PkCountArgs a = counts_args(h);
    a.keys = keys; a.mask = mask; a.counts_out = counts_out; a.bonus_out = bonus_out;
    a.env0 = env0; a.env1 = env0 + count; a.beta = beta; a.peek = flags & PK_COUNTS_PEEK;
    HIPCHK(pk_launch_cnt_update(a, (hipStream_t)stream));
    return 0;
}

int pk_counts_add(pk_handle* h, const pk_crec* rec, uint32_t n_records, uint32_t flags, void* stream) {
    if (!h) return fail(-EINVAL, "null handle");
    if (!h->cnt_log2) return fail(-ENOENT, "the handle has no count table (pk_counts_create)");
    if (!rec || ((uintptr_t)rec & 15u)) return fail(-EINVAL, "rec_dev is required and must be 16-byte aligned");
    if (n_records == 0 || n_records > (1u << 30)) return fail(-EINVAL, "n_records must be 1..2^30");
    if (flags & ~PK_COUNTS_FOREIGN) return fail(-EINVAL, "unknown flags 0x%x", flags);
    HIPCHK(hipSetDevice(h->device));
    PkCountArgs a = counts_args(h);
    a.rec = rec; a.env1 = n_records; a.foreign = flags & PK_COUNTS_FOREIGN;
    HIPCHK(pk_launch_cnt_add(a, (hipStream_t)stream));
    return 0;
}

int pk_counts_pack(pk_handle* h, uint32_t flags, pk_crec* rec, uint64_t max_records, uint32_t* n_out, void* stream) {
    if (!h) return fail(-EINVAL, "null handle");
    if (!h->cnt_log2) return fail(-ENOENT, "the handle has no count table (pk_counts_create)");
    if (!rec || ((uintptr_t)rec & 15u)) return fail(-EINVAL, "rec_dev is required and must be 16-byte aligned");
    if (!n_out) return fail(-EINVAL, "n_out_dev is required");
    if (max_records < counts_limit(h->cnt_log2))
        return fail(-EINVAL, "max_records %llu: a pack needs room for the table's limit of %llu records",
                    (unsigned long long)max_records, (unsigned long long)counts_limit(h->cnt_log2));
    if (flags & ~PK_COUNTS_DELTA) return fail(-EINVAL, "unknown flags 0x%x", flags);
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    PkCountArgs a = counts_args(h);
    a.pack = rec; a.n_out = n_out; a.max_records = max_records; a.delta = flags & PK_COUNTS_DELTA;
    HIPCHK(hipMemsetAsync(n_out, 0, 4, s));
    HIPCHK(pk_launch_cnt_pack(a, s));
    return 0;
}

int pk_counts_read(pk_handle* h, uint64_t* used, uint64_t* overflow) {
    if (!h) return fail(-EINVAL, "null handle");
    if (!h->cnt_log2) return fail(-ENOENT, "the handle has no count table (pk_counts_create)");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    uint64_t hdr[PK_CH_WORDS];
    HIPCHK(hipMemcpy(hdr, h->c_fix, sizeof hdr, hipMemcpyDeviceToHost));
    if (used) *used = hdr[PK_CH_USED];
    if (overflow) *overflow = hdr[PK_CH_OVERFLOW];
    return 0;
}

int pk_counts_clear(pk_handle* h, void* stream) {
    if (!h) return fail(-EINVAL, "null handle");
    if (!h->cnt_log2) return fail(-ENOENT, "the handle has no count table (pk_counts_create)");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(counts_wipe(counts_args(h), (hipStream_t)stream));
    return 0;
}

}  // extern "C"
