// pk_layout.h — device data layout shared by the HIP kernels and the host C-ABI.
//
// One wavefront lane = one emulator ("env").  Envs are grouped 64 to a "group".
//
// Per-env RAM image ("phys" address space, PK_PHYS bytes), stored LANE-INTERLEAVED per group, with
// an interleave W = 1 << sh (sh <= 6) chosen per handle = K1's envs per wave (16, 32 or 64): a
// group's PK_GROUP_STRIDE bytes hold 64 / W sub-blocks of W envs, and inside a sub-block
//     byte(env, phys) = sub-block base[phys * W + env % W]          (pk_img_off)
// so the W lanes of a wave touching the same guest address (the common case while they run the
// same code) hit W consecutive bytes — one coalesced access — no 64-byte line is shared by two
// waves, and a 128-byte line holds 128 / W consecutive guest bytes of the wave's envs.  (W = 64 is
// the round-1/2 layout.)
//
//   phys 0x0000-0x1FFF  VRAM   (guest 0x8000-0x9FFF)
//   phys 0x2000-0x3FFF  WRAM   (guest 0xC000-0xDFFF, echo 0xE000-0xFDFF)
//   phys 0x4000-0x409F  OAM    (guest 0xFE00-0xFE9F)
//   phys 0x40A0-0x40FF  unusable RAM (guest 0xFEA0-0xFEFF)
//   phys 0x4100-0x414B  IO ports backing store (guest 0xFF00-0xFF4B; special regs live in lane regs)
//   phys 0x414C-0x417F  non-IO RAM (guest 0xFF4C-0xFF7F)
//   phys 0x4180-0x41FE  HRAM   (guest 0xFF80-0xFFFE); 0x41FF unused (IE lives in lane regs)
//   phys 0x4200-0xC1FF  cartridge SRAM, 4 banks x 8 KiB (guest 0xA000-0xBFFF)
//
// Per-env lane registers: SoA u32 arrays regs[field * npad + env] (coalesced load/store at
// kernel entry/exit; inside the kernel they live in VGPRs).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef struct { uint32_t x, y; } uint2_t;

#define PK_LANES 64u
#define PK_PHYS 0xC200u
// sub-block skew: every sub-block starts PK_SKEW bytes after the end of the previous one, so the
// same guest byte of consecutive sub-blocks (waves) is not at the same offset modulo the memory
// channel interleave (PK_PHYS << sh is a multiple of 16 KiB for sh >= 5)
#ifndef PK_SKEW
#define PK_SKEW 0u
#endif
// bytes of one 64-env group: the largest over the interleaves (sh = 0: 64 sub-blocks)
#define PK_GROUP_STRIDE (PK_PHYS * PK_LANES + PK_SKEW * PK_LANES)

// sub-block stride and group stride of interleave 1 << sh
__host__ __device__ static inline uint64_t pk_sub_stride(uint32_t sh) { return ((uint64_t)PK_PHYS << sh) + PK_SKEW; }
__host__ __device__ static inline uint64_t pk_group_stride(uint32_t sh) { return (uint64_t)(PK_LANES >> sh) * pk_sub_stride(sh); }

// byte offset of (env, phys) in the image array, interleave 1 << sh
__host__ __device__ static inline uint64_t pk_img_off(uint32_t env, uint32_t phys, uint32_t sh) {
    const uint32_t l = env & (PK_LANES - 1u);
    return (uint64_t)(env / PK_LANES) * pk_group_stride(sh) + (uint64_t)(l >> sh) * pk_sub_stride(sh)
         + ((uint64_t)phys << sh) + (l & ((1u << sh) - 1u));
}

#define PK_P_VRAM 0x0000u
#define PK_P_WRAM 0x2000u
#define PK_P_OAM 0x4000u
#define PK_P_IO 0x4100u
#define PK_P_HRAM 0x4180u
#define PK_P_SRAM 0x4200u
#define PK_P_UNUSED 0x41FFu   // no guest byte (IE lives in lane regs): K1's dummy store target.
                              // K1's branch-free write stage stores a changing byte here every
                              // iteration, so nothing may read it: the v9 export/import and every
                              // image digest cover HRAM as 0x4180-0x41FE only (127 bytes) and take
                              // IE from the cpu register (pk_capi.cpp export_v9 / import_v9).
                              // The 64-bank parity tests (test_hostsim_game_64_banks,
                              // test_game_rom_64_banks_parity) would fail if an export read it: that
                              // instance stores unmodelled values here in every iteration

#define PK_ROWS 144u
#define PK_COLS 160u
#define PK_SCREEN (PK_ROWS * PK_COLS)

// lane register fields
enum {
    PK_R_W0 = 0,     // C | B<<8 | E<<16 | D<<24
    PK_R_W1,         // L | H<<8 | A<<16 | F<<24
    PK_R_SP,
    PK_R_PC,
    PK_R_CPU,        // ime | halted<<1 | queued<<2 | crashed<<3 | stopped<<4 | IE<<8 | IF<<16
    PK_R_CLOCK,      // PyBoy lcd.clock (always < 2^18 after the frame-wrap reduction)
    PK_R_TARGET,     // lcd.clock_target
    PK_R_LCD0,       // LCDC | STAT<<8 | LY<<16 | LYC<<24
    PK_R_LCD1,       // SCY | SCX<<8 | WY<<16 | WX<<24
    PK_R_LCD2,       // BGP | OBP0<<8 | OBP1<<16 | next_stat_mode<<24
    PK_R_TIM0,       // DIV | TIMA<<8 | TMA<<16 | TAC<<24
    PK_R_TIM1,       // DIV_counter | TIMA_counter<<16
    PK_R_MBC,        // rombank | rambank<<8 | ram_enabled<<16 | memorymodel<<24
    PK_R_MISC,       // joypad directional | standard<<8 | (ly_window+1)<<16 (u8)
    PK_R_TIME,       // env-steps since reset (pokegym `self.time`, environment.py:1338)
    PK_R_ICOUNT,     // emulated instructions in the last pk_step (perf counter)
    PK_R_RFLAGS,     // render bookkeeping of the last step: blank<<0 | (lines left for K2)<<8
    PK_NREGS
};

// diagnostic buffer (-DPK_STAMP phase counters; -DPK_WAVETIME adds one PK_WT_REC-word record per K1 wave)
#ifdef PK_WAVETIME
#define PK_WT_REC 6u
#define PK_DBG_WORDS (64u + PK_WT_REC * 16384u)
#else
#define PK_DBG_WORDS 64u
#endif

// K1's LDS budget.  The default kernel stages PK_LDS_SLOTS ROM banks (16 KiB each, slot 0 = bank 0)
// and the HRAM code mirror of up to PK_WG_ENVS envs: 158 KB, one workgroup per CU, 512 threads =
// 8 waves, two per SIMD at ~233 VGPRs.  The small-LDS kernel (pk_step.hip compiled a second time
// with PK_K1_SMALL) stages 2 banks and the mirror of 128 envs in 256-thread workgroups: 78.7 KB, so
// two workgroups fit on a CU.  pk_capi.cpp launches it for the ranges of concurrent sub-batches
// (VecEnv), whose workgroups can then start on a CU where the other sub-batch is still in its tail.
#define PK_SMALL_LDS_SLOTS 2u
#define PK_SMALL_WG_ENVS 128u
#define PK_SMALL_MAX_THREADS 256
#ifdef PK_K1_SMALL
#define PK_WG_ENVS PK_SMALL_WG_ENVS
#define PK_LDS_SLOTS PK_SMALL_LDS_SLOTS
#define PK_K1_MAX_THREADS PK_SMALL_MAX_THREADS
#endif
#ifndef PK_K1_MAX_THREADS
#define PK_K1_MAX_THREADS 512
#endif
#ifndef PK_WG_ENVS
#define PK_WG_ENVS 512u
#endif
#ifndef PK_LDS_SLOTS
#define PK_LDS_SLOTS 6u
#endif

// kernel argument blocks (passed by value)
struct PkStepArgs {
    uint8_t* mem;             // lane-interleaved RAM images
    const uint8_t* rom;       // whole ROM (+16 bytes of padding: dword fetches may overrun the end)
    const uint32_t* romw;     // the same, as dwords
    uint32_t* regs;           // SoA lane registers [PK_NREGS][npad]
    const uint32_t* ucode;    // microcode table (pk_ucode.h), PK_UC_ENTRIES x 8 dwords
    const uint8_t* actions;   // [n] action ids (0..7; >=8 = no button)
    uint32_t* lat;            // [3][ngroups*144*64] per-line render latches
    uint8_t* screen;          // [n][144][160] persistent grey screen
    uint32_t n, npad;
    uint32_t rom_bank_mask;
    uint32_t mbc;             // 0 = ROM only, 3 = MBC3
    uint32_t frames;          // frame_skip (24)
    uint32_t release_frame;   // 8
    uint32_t render_last;     // rasterise the last frame
    uint32_t lat_stride;      // ngroups*144*64
    uint32_t nslots;          // ROM banks staged in LDS (slot 0 = bank 0)
    const int8_t* bank_slot;  // [128] LDS slot of each ROM bank, -1 = not staged
    const uint8_t* slot_bank; // [PK_LDS_SLOTS] bank held by each slot
    uint32_t wave_lanes;      // envs per 64-lane wave in K1 (64, 32 or 16): fewer lanes = more waves/SIMD
    uint32_t simds;           // SIMDs of the device: K1 uses 256-thread workgroups while waves <= simds
    uint32_t block;           // K1 workgroup size override (0 = by geometry; PK_K1_BLOCK, tests)
    uint32_t prio;            // K1 wave-priority variant (two waves per SIMD; PK_K1_PRIO overrides)
    unsigned long long* dbg;  // diagnostic counters (-DPK_STAMP builds only), else null
    uint32_t env0, env1;      // env range of this launch: [env0, env1), env0 % 64 == 0 (sub-batches)
    uint32_t ilv_sh;          // image interleave: 1 << ilv_sh envs (pk_img_off)
    uint32_t small;           // launch the small-LDS K1 (pk_launch_step_small)
    uint32_t all_staged;      // every ROM bank is staged in this kernel's LDS slots (the ALL instance)
};

// K2's second argument block: the termination flags of a rendered step without the reward stack
// (pk_done_kernel's outputs), written by the wave of scanline 0 when `on` is set
struct PkDoneArgs {
    const uint32_t* time_reg;    // regs + PK_R_TIME * npad
    uint8_t* term;               // caller's [n] arrays, each may be null
    uint8_t* trunc;
    double* rew;
    uint32_t max_steps;
    uint32_t on;
};

struct PkResetArgs {
    uint8_t* mem;
    uint32_t* regs;
    uint32_t* lat;
    uint8_t* screen;
    const uint8_t* tmpl_mem;     // PK_PHYS bytes
    const uint32_t* tmpl_regs;   // PK_NREGS
    const uint32_t* tmpl_lat;    // 3*144
    const uint8_t* tmpl_screen;  // 144*160
    const uint32_t* cnt;         // envs to reset: count (device memory) ...
    const uint32_t* ids;         // ... and their ids (pk_list_kernel)
    uint32_t n, npad, lat_stride;
    uint32_t env0, env1;         // env range the list was built over
    uint32_t ilv_sh;             // image interleave (pk_img_off)
};

// Savestate bank (pk_bank_* / pk_reset_from): n_slots slots of machine state in device memory, each
// what a parsed v9 template holds — the dense PK_PHYS-byte RAM image (linear, not interleaved),
// PK_BANK_REGS register words (PK_NREGS used), 3 x 144 latches and the 144 x 160 screen, one
// array per part so every part of a slot starts 16-byte aligned: 74,512 bytes per slot.
#define PK_BANK_REGS 20u
#define PK_BANK_MAX_SLOTS 65536u
// RAM-image tile of the bank <-> image transposition: PK_BANK_TILE bytes = (PK_BANK_TILE >> sh)
// phys rows of one sub-block's 1 << sh envs, padded by one word per env in LDS
#define PK_BANK_TILE 16384u
enum { PK_BANK_LOAD = 0, PK_BANK_SAVE = 1, PK_BANK_RESET = 2 };

struct PkBankArgs {
    uint8_t* mem;                // lane-interleaved RAM images
    uint32_t* regs;
    uint32_t* lat;
    uint8_t* screen;
    uint8_t* b_mem;              // [n_slots][PK_PHYS]
    uint32_t* b_regs;            // [n_slots][PK_BANK_REGS]
    uint32_t* b_lat;             // [n_slots][3 * 144]
    uint8_t* b_screen;           // [n_slots][144 * 160]
    uint8_t* b_filled;           // [n_slots]
    uint8_t* b_ep_filled;        // [n_slots] the slot also holds an episode part (pk_reward.h PkEpArgs);
                                 // null while the bank carries no episodes
    uint32_t* b_rejects;         // envs that named a slot >= n_slots or an empty slot
    const int32_t* slot_of_env;  // caller's i32[n]
    const uint8_t* sel;          // PK_BANK_RESET: envs that reload (u8[n]; null = all)
    int32_t* src;                // [npad] validated slot of every env of the range, -1 = takes no part
    uint32_t* cnt;               // the range's bank lists: [0] envs, [1] sub-blocks ...
    uint32_t* ids;               // ... env ids (from env0) ...
    uint32_t* subs;              // ... and the sub-blocks (env >> ilv_sh) that hold one
    uint32_t* tcnt;              // PK_BANK_RESET: the range's template reset list (pk_list_kernel's),
    uint32_t* tids;              // taking the reloading envs without a usable slot
    uint32_t n_slots;
    uint32_t mode;               // PK_BANK_*
    uint32_t ep;                 // pk_bank_checkpoint / pk_bank_resume: PK_BANK_SAVE marks the episode part
                                 // filled too (a plain save marks it empty), PK_BANK_LOAD also needs it filled
    uint32_t n, npad, lat_stride;
    uint32_t env0, env1;
    uint32_t ilv_sh;
};

// Exploration archive on the bank (pk_archive_*): cell c owns bank slot slot0 + c and keeps the best
// episode seen under its key.  Persistent part: the header words, the per-cell records and an
// open-addressing index key -> cell of i_mask + 1 >= 2 * n_cells entries (accepted cells only).
// Per-call part (pk_archive_update): a scratch table of s_mask + 1 >= 2 * count entries for the
// keys the index does not hold, the per-cell and per-entry winner words, and per-env words.
#define PK_ARCH_MAX_CELLS 65536u
#define PK_ARCH_NOKEY 0xFFFFFFFFFFFFFFFFull   // the reserved key: "no cell", and an empty table entry
#define PK_ARCH_NONE 0xFFFFFFFFu
#define PK_ARCH_PRE 8u                        // wave pre-reduction rounds before lanes go to memory alone
enum { PK_AH_USED = 0, PK_AH_OVERFLOW, PK_AH_DRAWS, PK_AH_CUR, PK_AH_TOTAL, PK_AH_WORDS = 8 };

struct PkArchArgs {
    uint64_t* hdr;               // [PK_AH_WORDS]: cells in use, overflow, draw calls, the running
                                 // explore's call number and total weight
    uint64_t* a_key;             // [n_cells]
    double* a_score;             // [n_cells] the record's score ...
    uint32_t* a_len;             // ... and length (the winner's PK_R_TIME)
    uint32_t* a_visits;
    uint32_t* a_picks;
    uint64_t* prefix;            // [n_cells] inclusive prefix sums of the weights (explore)
    uint64_t* i_key;             // index: key (PK_ARCH_NOKEY = empty) ...
    uint32_t* i_cell;            // ... and its cell
    uint64_t* c_max;             // per call, per cell: best candidate score (encoded), 0 = none ...
    uint64_t* c_le;              // ... and the least length << 32 | env among those with that score
    uint64_t* s_key;             // scratch entries: key, the same two winner words,
    uint64_t* s_max;
    uint64_t* s_le;
    uint32_t* s_first;           // the lowest env that reached the key, the envs that did,
    uint32_t* s_cnt;
    uint32_t* s_cell;            // and the cell the key was given (PK_ARCH_NONE: the archive was full)
    uint32_t* tgt;               // [npad] per env: its cell, n_cells + its scratch entry, or PK_ARCH_NONE
    uint8_t* flag;               // [npad] the env is the first of a new key
    int32_t* map;                // [npad] the slot map handed to the bank kernels
    const uint64_t* keys;        // caller's arrays
    const double* scores;
    const uint8_t* mask;
    const uint32_t* time_reg;    // regs + PK_R_TIME * npad
    uint32_t* b_rejects;
    const int32_t* src;          // the bank's validated slot per env (PkBankArgs.src)
    int32_t* out;                // caller's slot_of_env_out
    uint64_t seed;
    uint32_t i_mask, s_mask;
    uint32_t n_cells, slot0;
    uint32_t env0, env1;
    // archive exchange (pk_archive_exchange_enable), null without it: per cell what was already
    // sent on and whether the record changed since the last delta pack.  An update only sets dirty.
    uint32_t* x_sent_visits;     // [n_cells]
    uint32_t* x_sent_picks;      // [n_cells]
    uint32_t* x_dirty;           // [n_cells]
    // pk_archive_merge runs the four update phases with records in the place of envs (the <true>
    // instances): item i of [0, env1) is rec[i], tgt / flag / map are the merge's own arrays
    const struct pk_xrec* rec;   // caller's records
    uint32_t* s_vis;             // scratch entries: the visits and picks of the records from the
    uint32_t* s_pick;            // key's first payload on (s_cnt counts those records)
    uint32_t* x_cnt;             // the list of winners the payload mover runs over: count ...
    uint32_t* x_cell;            // ... the winner's cell ...
    uint32_t* x_pay;             // ... and its payload row
    uint32_t n_payloads;         // rows of the caller's payload array
    uint32_t format;             // this handle's pk_archive_format
};

// Archive exchange: a payload is one whole slot as linear bytes, the slot's parts in a fixed order
// at 16-byte-aligned offsets (pk_capi.cpp xchg_args states the order).  A part is an array of the
// handle with one fixed-size row per slot, so a mover's 16-byte piece q of a payload belongs to the
// part p with off16[p] <= q < off16[p + 1] and sits at base[p] + slot * stride[p] + (q - off16[p]) * 16.
// The trajectory part's origin and flag words are kept a word per slot: they travel as one piece
// {origin, flags, 0, 0} built in registers (head16).
#define PK_XCHG_MAX_PARTS 10u
#define PK_XCHG_VERSION 1u       // payload layout version, the top byte of pk_archive_format
#define PK_XCHG_MAX_RECORDS 65536u
#define PK_XCHG_CHUNK 1024u      // 16-byte pieces of one payload a workgroup moves

struct PkXchgArgs {
    uint8_t* base[PK_XCHG_MAX_PARTS];
    uint32_t stride[PK_XCHG_MAX_PARTS];   // bytes per slot of the part's array
    uint32_t off16[PK_XCHG_MAX_PARTS + 1u];
    uint32_t nparts;
    uint32_t head16;             // the piece of {origin, flags, 0, 0}; PK_ARCH_NONE without trajectories
    int32_t* bt_origin;          // [n_slots]
    uint32_t* bt_flags;          // [n_slots]
    uint8_t* b_filled;           // [n_slots] unpack marks the slot filled ...
    uint8_t* b_ep_filled;        // ... with an episode part
    uint8_t* payload;            // caller's rows of pay16 * 16 bytes
    uint32_t pay16;
    const uint32_t* cnt;         // device-built list: count, cell and payload row per item
    const uint32_t* cell;
    const uint32_t* pay;
    uint32_t slot0;
    uint32_t items;              // upper bound of listed items, sizes the grid
};

// pk_archive_pack: the one-workgroup scan that writes the records, numbers the payloads in cell
// order and lists them
struct PkPackArgs {
    PkArchArgs a;
    struct pk_xrec* out;         // caller's records [count]
    uint32_t* n_payloads_out;    // caller's word, or null
    uint32_t cell0, count, max_payloads, delta;
};

// Frame cells (pk_frame_keys): a screen is PK_CELL_PIECES 16-byte pieces, ten to a row, each piece two
// halves of 8 pixels; an 8 x 8 tile is the same half of eight pieces, ten rows of pieces apart
#define PK_CELL_PIECES (PK_SCREEN / 16u)      // 1,440
#define PK_CELL_TILES_X (PK_COLS / 8u)        // 20
#define PK_CELL_TILES (PK_SCREEN / 64u)       // 360, also the most blocks a screen has
#define PK_CELL_GOLD 0x9E3779B97F4A7C15ull

struct PkCellArgs {
    const uint8_t* screen;       // [..][144][160], 16-byte aligned: the handle's or the caller's
    const uint64_t* salt;        // caller's [n] or null; may be keys
    uint64_t* keys;              // caller's [n]
    uint8_t* cells;              // caller's [n][nbx * nby] or null
    uint32_t env0, env1;
    uint32_t bw, bh, levels;
};

// Visit counts (pk_counts_*): an open-addressing table key -> count of c_mask + 1 entries, linear
// probing from the low bits of pk_arch_mix(key), in three arrays so that a probe reads keys only.
// The header words: the distinct keys stored when the running call started (USED: what decides
// whether the call is open, written only by the commit that ends a call), the keys the running
// call has inserted so far (NEW) and the overflow count.  tgt holds, per env of an update, the entry
// launch one found or made for the env's key, for launch two to read the count from.
#define PK_CNT_MIN_LOG2 10u
#define PK_CNT_MAX_LOG2 30u
enum { PK_CH_USED = 0, PK_CH_OVERFLOW, PK_CH_NEW, PK_CH_WORDS = 8 };

struct PkCountArgs {
    uint64_t* hdr;               // [PK_CH_WORDS]
    uint64_t* c_key;             // [c_mask + 1] PK_ARCH_NOKEY = empty
    uint64_t* c_cnt;             // visits
    uint64_t* c_sent;            // the part of c_cnt a delta pack does not send: sent before, or foreign
    uint32_t* tgt;               // [npad] per env: its entry, or PK_ARCH_NONE
    const uint64_t* keys;        // pk_counts_update: caller's arrays
    const uint8_t* mask;
    uint64_t* counts_out;
    double* bonus_out;
    const struct pk_crec* rec;   // pk_counts_add: caller's records, items [0, env1)
    struct pk_crec* pack;        // pk_counts_pack: caller's records and their number
    uint32_t* n_out;
    uint64_t max_records;
    uint64_t limit;              // distinct keys the table takes: 3/4 of its entries
    double beta;
    uint32_t c_mask;
    uint32_t env0, env1;
    uint32_t peek, foreign, delta;
};

// Frame stack (pk_fstack_*): per env D planes of H x W = (144 / s) x (160 / s) bytes, plane 0 the
// newest, as u8[n][D][H][W] (CHW) or u8[n][H][W][D] (HWC).  A thread of the push owns one piece of
// consecutive output pixels of one row: 16 pixels at s = 1 and 2 and 8 at s = 4 in CHW (a 16- or
// 8-byte piece in each plane), 16 / D pixels in HWC (one 16-byte piece that holds their D bytes).
#define PK_FS_MAX_DEPTH 8u

struct PkStackArgs {
    const uint8_t* screen;       // [..][144][160], 16-byte aligned: the handle's or the caller's
    const uint8_t* mask;         // caller's [n] or null
    uint8_t* stack;              // [n][D * H * W]
    uint32_t env0, env1;
    uint32_t scale, depth, layout, mode;
    uint32_t fill_only;
};

// RAM probes (pk_probe_*): the program is the caller's pk_probe table (24 bytes a probe, at most 64)
// copied to the device once its elements are validated; the guest address of an element becomes a
// phys address in the kernel by two wave-uniform operations (the elements of one probe may lie in
// WRAM, its echo and HRAM).  The per-env state is one word per probe, probe-major:
// state[j * npad + env], so that a wave's loads and stores of a probe's state are consecutive words.
#define PK_PROBE_WG 64u
#define PK_PROBE_CHUNK 16u       // probes per pass of the feature tile in LDS

struct PkProbeArgs {
    const uint8_t* mem;          // lane-interleaved RAM images
    const struct pk_probe* prog; // [m], device
    uint32_t* state;             // [m][npad]
    const uint8_t* mask;         // caller's [n] or null
    double* rew;                 // caller's [n] or null
    uint8_t* term;               // caller's [n] or null
    int32_t* feat;               // caller's [n][m] or null
    uint32_t m, npad;
    uint32_t env0, env1;
    uint32_t ilv_sh;
    uint32_t rebase_only, set;
};

// Generic episode part of a bank slot (pk_bank_enable_generic_episodes): what an episode consists of
// on a handle without the reward stack, one array per part, every part of a slot 16-byte aligned.
//   g_regs   u32[n_slots][PK_GEP_REGS]  all PK_NREGS lane registers raw (the machine part stores
//            PK_R_TIME / PK_R_ICOUNT / PK_R_RFLAGS as 0, PK_R_MISC as "nothing held" and drops the
//            register bits a v9 state has no room for), padded to whole 16-byte pieces with 0
//   g_probe  u32[n_slots][mpad]         PK_GEP_PROBES: word j = state[j * npad + env], m padded to 4
//   g_stack  u8[n_slots][row16 * 16]    PK_GEP_STACK: the env's row of the frame stack, linear on
//            both sides in both layouts (H * W is a multiple of 16)
#define PK_GEP_REGS ((PK_NREGS + 3u) / 4u * 4u)
#define PK_GEP_CHUNK 1024u       // 16-byte pieces of a stack row one workgroup pass moves

struct PkGepArgs {
    uint32_t* regs;              // K1 lane registers [PK_NREGS][npad]
    uint32_t* state;             // probe state [m][npad]; null without PK_GEP_PROBES
    uint8_t* stack;              // [n][row16 * 16]; null without PK_GEP_STACK
    uint32_t* g_regs;            // [n_slots][PK_GEP_REGS]
    uint32_t* g_probe;           // [n_slots][mpad]
    uint8_t* g_stack;            // [n_slots][row16 * 16]
    const uint32_t* cnt;         // the range's bank list (pk_bank_list_kernel): count ...
    const uint32_t* ids;         // ... env ids ...
    const int32_t* src;          // ... and the validated slot of every env
    uint32_t npad;
    uint32_t m, mpad;            // probes carried (0 without the part) and their padded count, <= 64
    uint32_t row16;              // 16-byte pieces of a stack row, 0 without the part
    uint32_t save;               // 1 = checkpoint (env -> slot), 0 = resume (slot -> env)
    uint32_t items;              // upper bound of listed envs (the range's size): sizes the grid
};

// Tile view (pk_tiles_*): per env P planes (BG / window, objects) of PK_TILE_ROWS x PK_TILE_COLS u16
// values, u16[n][P][18][20].  A workgroup of PK_TILES_WG threads takes PK_TILES_ENVS neighbouring envs
// (a sub-block of the image, or a part of one); thread t works for env t % PK_TILES_ENVS on the
// cells t / PK_TILES_ENVS, + PK_TILES_SLOTS, ...: neighbouring lanes hold neighbouring envs of one cell.
#define PK_TILE_ROWS (PK_ROWS / 8u)           // 18
#define PK_TILE_COLS (PK_COLS / 8u)           // 20
#define PK_TILE_CELLS (PK_TILE_ROWS * PK_TILE_COLS)
#define PK_TILE_NONE 0xFFFFu
#define PK_TILES_WG 256u
#define PK_TILES_ENVS 16u
#define PK_TILES_SLOTS (PK_TILES_WG / PK_TILES_ENVS)

struct PkTilesArgs {
    const uint8_t* mem;          // lane-interleaved RAM images
    const uint32_t* regs;        // K1 lane registers [PK_NREGS][npad]: PK_R_LCD0, PK_R_LCD1
    const uint8_t* mask;         // caller's [n] or null
    const uint64_t* salt;        // caller's [n] or null
    uint64_t* keys;              // caller's [n] or null
    uint16_t* out;               // [n][planes][18][20]
    uint32_t npad;
    uint32_t env0, env1;
    uint32_t ilv_sh;
    uint32_t planes;             // 1, or 2 with PK_TILES_OBJ
    uint32_t bits;               // 0 = PK_TILES_ID, else the hash bits of PK_TILES_HASH (8..15)
};
