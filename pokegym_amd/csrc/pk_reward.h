// pk_reward.h — device layout of the reward stack (K4), reset (K5r) and obs compose (K3).
//
// Per-env reward state restating the Python attributes pokegym keeps per Environment
// (environment.py:102-197, :437-522, :1256-1331).  SoA u32 fields rs[field * npad + env], three
// f64 fields rsd[field * npad + env], and three per-env side tables:
//   seen  u32[npad][cap]    open-addressing set of (r, c, map) = self.seen_coords (:1345);
//                           slot = r | c<<8 | map<<16 | gen<<24 (gen = episode tag 1..255, a slot
//                           with another gen is empty, so a reset never clears the table)
//   mask  u32[npad][2048]   256x256-bit visited mask of the CURRENT map = screen_memory[map]
//                           (:157-160, :256-263); rebuilt from `seen` when the map changes
//   cutc  u32[npad][64]     self.cut_coords in insertion order (:1519-1525)
#pragma once
#include <stdint.h>

enum {
    RS_FLAGS = 0,     // RSF_* bits
    RS_ERR,           // first error (PK_ERR_*), sticky until reset
    RS_USED_CUT,      // self.used_cut
    RS_SEEN_N,        // len(self.seen_coords)
    RS_GEN,           // seen-set episode tag 1..255
    RS_MAX_LEVEL,     // self.max_level_sum
    RS_MAX_OPP,       // self.max_opponent_level (info only)
    RS_MAX_EVENTS,    // self.max_events
    RS_LAST_PARTY,    // self.last_party_size
    RS_DEATHS,        // self.death_count (info only)
    RS_LAST_MAP1,     // self.last_10_map_ids[0][0]
    RS_HEAT_LAST,     // update_heat_map's self.last_map (-1 = none); survives resets
    RS_CUTSTATE0,     // self.cut_state: 3 x 6 bytes, oldest first, in words CUTSTATE0..4
    RS_CUTSTATE1,
    RS_CUTSTATE2,
    RS_CUTSTATE3,
    RS_CUTSTATE4,
    RS_CUTSTATE_N,    // entries in cut_state (0..3)
    RS_CUT_TILES,     // 8 words: 256-bit set of self.cut_tiles keys
    RS_CUT_TILES_END = RS_CUT_TILES + 8,
    RS_CUTC_N = RS_CUT_TILES_END,  // entries in cutc
    RS_MOVES,         // 6 words: self.moves_obtained bitmap (165 entries)
    RS_MOVES_END = RS_MOVES + 6,
    RS_MASK_MAP = RS_MOVES_END,    // map whose visited mask is in `mask` (0xFFFFFFFF = none)
    RS_RESET_POS,     // r | c<<8 | map<<16 | 1<<24 of the reset-time render() (:1334)
    RS_RESET_COUNT,   // self.reset_count
    RS_NFIELDS
};

enum { RSD_LAST_REWARD = 0, RSD_TOTAL_HEALING, RSD_LAST_HP, RSD_COORD /* np.sum(counts_map), survives resets */,
       RSD_NFIELDS };

// RS_FLAGS bits
#define RSF_HAS_LAST 1u       // self.last_reward is not None
#define RSF_IS_DEAD 2u        // self.is_dead (survives resets)
#define RSF_CUT 4u            // self.cut
#define RSF_MENU0 8u          // seen_start_menu, pokemon, stats, bag, cancel_bag: bits 3..7
#define RSF_BAG0 0x100u       // has_{lemonade,silph_scope,lift_key,pokedoll,bicycle}_in_bag_reward: bits 8..12 (survive resets)
#define RSF_STUCK_INIT 0x2000u  // self.stuck_cnt exists (survives resets)
#define RSF_KEEP (RSF_IS_DEAD | (0x1Fu * RSF_BAG0) | RSF_STUCK_INIT)

// error codes (the reference raises; include/pokegym_amd.h PK_ERR_*)
#define PKE_MAP_KEY 1u
#define PKE_STUCK_ATTR 2u
#define PKE_MOVE_INDEX 3u
#define PKE_CUT_COORDS 4u
#define PKE_HEATMAP_INDEX 5u
#define PKE_BUS_INDEX 6u
#define PKE_CAPACITY 7u       // device table full (no reference equivalent)
#define PKE_EMPTY_PARTY 8u    // ValueError: max(party_levels) of an empty party in the info dict (:1672)

// info telemetry record (environment.py:1621-1704; field order = pokegym_amd/info.py FIELDS)
#define PK_INFO_NSTATS 58u
#define PK_INFO_NREWARD 21u
#ifndef PK_INFO_NFIELDS
#define PK_INFO_NFIELDS 79u   // == include/pokegym_amd.h
#endif
static_assert(PK_INFO_NFIELDS == PK_INFO_NSTATS + PK_INFO_NREWARD, "info record layout");

#define PK_CUTC_CAP 64u
#define PK_INFO_BITS_WORDS 5u  // 130 event-monitor bits (ram_map_leanke monitor_*_events), MONITORS order
#define PK_HEAT_ROWS 444u     // counts_map = np.zeros((444, 436)) (environment.py:448)
#define PK_HEAT_COLS 436u
#define PK_MASK_WORDS 2048u   // 256 rows x 8 words
#define PK_OBS_H 72u
#define PK_OBS_W 80u
#define PK_OBS_BYTES (PK_OBS_H * PK_OBS_W * 4u)

// Episode part of a savestate-bank slot (pk_bank_checkpoint / pk_bank_resume): what pk_bank_save
// leaves behind of an episode, so that a resumed env continues exactly as the saved one would have.
//   fields  u32[PK_EP_WORDS] per slot, AoS: the rs[] fields at PK_EP_RS, the raw lane registers at
//           PK_EP_REGS (all PK_NREGS: the machine part stores PK_R_TIME / PK_R_ICOUNT /
//           PK_R_RFLAGS as 0, PK_R_MISC as "nothing held" and drops register bits a v9 state has
//           no room for), the rsd[] fields (f64) at PK_EP_RSD.  RS_GEN, RS_RESET_COUNT and
//           RSD_COORD belong to the env, not to the episode: they are stored but never restored.
//   seen    u32[cap] per slot, normalised: a live entry carries tag 1, every other word is 0
//   mask    u32[PK_MASK_WORDS], cutc u32[PK_CUTC_CAP] per slot, as the env has them
// Every part of a slot starts 16-byte aligned.  The PK_F_HEATMAP counts_map stays with the env.
#define PK_EP_RS 0u
#define PK_EP_REGS 40u
#define PK_EP_RSD 60u
#define PK_EP_WORDS 68u
#define PK_EP_CHUNK 1024u     // 16-byte pieces of [seen | mask] one workgroup pass moves
static_assert(RS_NFIELDS <= PK_EP_REGS - PK_EP_RS && 2u * RSD_NFIELDS <= PK_EP_WORDS - PK_EP_RSD &&
              PK_EP_WORDS % 4u == 0u && PK_EP_RSD % 2u == 0u, "episode record layout");

struct PkEpArgs {
    uint32_t* regs;           // K1 lane registers [PK_NREGS][npad]
    uint32_t* rs;             // [RS_NFIELDS][npad]
    double* rsd;              // [RSD_NFIELDS][npad]
    uint32_t* seen;           // [npad][cap]
    uint32_t* mask;           // [npad][PK_MASK_WORDS]
    uint32_t* cutc;           // [npad][PK_CUTC_CAP]
    uint32_t* e_fields;       // [n_slots][PK_EP_WORDS]
    uint32_t* e_seen;         // [n_slots][cap]
    uint32_t* e_mask;         // [n_slots][PK_MASK_WORDS]
    uint32_t* e_cutc;         // [n_slots][PK_CUTC_CAP]
    const uint32_t* cnt;      // the range's bank list (pk_bank_list_kernel): count ...
    const uint32_t* ids;      // ... env ids ...
    const int32_t* src;       // ... and the validated slot of every env
    uint32_t npad, nregs;     // nregs = PK_NREGS (<= PK_EP_RSD - PK_EP_REGS)
    uint32_t cap_log2;
    uint32_t save;            // 1 = checkpoint (env -> slot), 0 = resume (slot -> env)
    uint32_t items;           // upper bound of listed envs (the range's size): sizes the grid
};

// Action trajectories (pk_traj_enable): per env the actions of its episode so far, one byte per
// step, with the bank slot the episode started from (origin, -1 = the handle's template) and
// PK_TRAJ_* flags; the length is the env's step counter PK_R_TIME clamped to the capacity
// cap = 3 << (cap_log2 - 2), a multiple of 16 that is >= max_episode_steps.  Rows are env-major,
// u8[npad][cap], so a row is linear memory and starts 16-byte aligned.  When the bank carries
// episode parts every slot has the same three parts; a slot's length is the step counter of its
// episode record (e_fields, PK_EP_REGS + PK_R_TIME; on a handle with generic episode parts the
// raw registers of g_regs, PK_R_TIME).  The flags are kept a word per env and slot:
// the mover makes no byte access.
#ifndef PK_TRAJ_BROKEN
#define PK_TRAJ_BROKEN 1u     // == include/pokegym_amd.h
#define PK_TRAJ_OVERFLOW 2u
#define PK_TRAJ_EMPTY 4u
#endif

struct PkTrajArgs {
    const uint32_t* time_reg; // regs + PK_R_TIME * npad
    uint8_t* act;             // [npad][cap]
    int32_t* origin;          // [npad]
    uint32_t* flags;          // [npad]
    uint8_t* b_act;           // [n_slots][cap], null while the bank carries no episodes
    int32_t* b_origin;        // [n_slots]
    uint32_t* b_flags;        // [n_slots]
    const uint32_t* e_fields; // the slots' episode records (their lengths): [n_slots][e_stride] words, the step
    uint32_t e_stride, e_time;// counter at word e_time — PK_EP_WORDS and PK_EP_REGS + PK_R_TIME, or the
                              // generic part's PK_GEP_REGS and PK_R_TIME (pk_layout.h PkGepArgs)
    const uint8_t* b_ep_filled;
    const uint8_t* actions;   // record: the step's actions [n]
    const uint8_t* mask;      // reset: the envs that were reset (null = all)
    const uint8_t* reload;    // reset: which of them reloaded their machine (null = all)
    const int32_t* src;       // reset: the slot an env reloaded, -1 = the template (null = template);
                              // move: the validated slot of every listed env
    const uint32_t* cnt;      // move / mark: a device-built env list (count, ids); mark without
    const uint32_t* ids;      // a list covers [env0, env1)
    int32_t* o_origin;        // get: the caller's arrays, any may be null
    uint32_t* o_len;
    uint8_t* o_flags;
    uint8_t* o_act;
    uint32_t cap;
    uint32_t env0, env1;      // env range; get with slots = 1: the slot range
    uint32_t save;            // move: 1 = env -> slot, 0 = slot -> env
    uint32_t slots;           // get: read slots (outputs indexed by slot - env0) instead of envs
    uint32_t items;           // move / mark: upper bound of listed envs, sizes the grid
};

struct PkRewardArgs {
    uint8_t* mem;             // lane-interleaved RAM images (pk_layout.h)
    uint32_t* regs;           // K1 lane registers (TIME, special IO regs)
    uint32_t* rs;             // [RS_NFIELDS][npad]
    double* rsd;              // [RSD_NFIELDS][npad]
    uint32_t* seen;           // [npad][cap]
    uint32_t* mask;           // [npad][PK_MASK_WORDS]
    uint32_t* cutc;           // [npad][PK_CUTC_CAP]
    const uint8_t* actions;   // [n]
    const uint8_t* env_mask;  // reset: envs to reset (null = all)
    uint8_t* reload;          // reset: [n] out = template reload wanted
    const uint8_t* screen;    // [npad][144][160] grey
    uint8_t* obs;             // [n][72][80][4]
    const uint32_t* ocnt;     // obs for listed envs only (reset): count (device memory) and ids,
    const uint32_t* oids;     // or null = all n envs
    double* rew;              // [n] or null
    uint8_t* term;            // [n] or null
    uint8_t* trunc;           // [n] or null
    double* info;             // [PK_INFO_NFIELDS][npad] info record, written where info_flag = 1
    uint8_t* info_flag;       // [n] 1 = this step built the reference's info dict (done or time % 10000 == 0)
    uint32_t* info_bits;      // [PK_INFO_BITS_WORDS][npad] monitor bits of the info record's step
    int32_t* heat;            // [npad][PK_HEAT_ROWS * PK_HEAT_COLS] counts_map, or null (PK_F_HEATMAP off)
    double reward_scale;
    uint32_t n, npad;
    uint32_t cap_log2;        // seen table capacity = 1 << cap_log2
    uint32_t max_steps;
    uint32_t reload_always;   // PK_F_RELOAD_ON_RESET
    uint32_t env0, env1;      // env range of this launch (sub-batches); arrays stay full-size [n]
    uint32_t ilv_sh;          // image interleave (pk_layout.h pk_img_off)
};
