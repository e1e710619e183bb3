/*
 * pokegym_amd.h — C ABI of the MI355X-native batched Pokémon Red env.step.
 *
 * Plain C: pointers and sizes only, no torch/HIP types.  `stream` arguments are hipStream_t
 * values passed as void* (NULL = the default stream).  Device buffers passed in are owned by the
 * caller (e.g. PyTorch-ROCm tensors' data_ptr()); buffers returned by pk_*_ptr() are owned by
 * the handle and live until pk_destroy.  Calls are stream-ordered and asynchronous unless noted.
 * One handle per GPU; a handle is not thread-safe.  Every function returns 0 on success or a
 * negative errno-style code; pk_last_error() describes the last failure of the calling thread.
 *
 * Each entry point replaces one piece of the reference's per-env Python/PyBoy path
 * (/root/reference/pokegym, file:line):
 *   pk_create        make_env + open_state_file        pyboy_binding.py:42-64, environment.py:121-122
 *   pk_reset         load_pyboy_state / Env.reset      pyboy_binding.py:66-69, environment.py:1233-1242
 *   pk_step          run_action_on_emulator + the      pyboy_binding.py:71-91,
 *                    per-step screen obs               environment.py:1336-1337, :268
 *   pk_peek          PyBoy get_memory_value (WRAM)     ram_map.py:1768-1770 (mem_val)
 *   pk_poke          PyBoy set_memory_value (WRAM)     ram_map.py:1772-1774 (write_mem)
 *   pk_snapshot      PyBoy save_state (v9 format)      environment.py:208-214
 *   pk_load_env      PyBoy load_state for one env      pyboy_binding.py:66-69
 *   pk_destroy       Env.close                         environment.py:412-413
 *   pk_obs_ptr       Env.render (72,80,4) observation  environment.py:256-274, :233-254
 *   pk_error_ptr     exceptions the reference raises   environment.py:739,744,568/580,1519,676
 *   pk_get_ram       per-env RAM views (RAM-only obs)  ram_map.py:1768-1770 (batched)
 *   pk_set_ram       per-env RAM writes                ram_map.py:1772-1774 (batched)
 *   pk_bank_put      the pool of start states          environment.py:51, :116 (get_random_state),
 *                                                      :122 (initial_states)
 *   pk_bank_save     save_state, kept on the device    environment.py:208-214
 *   pk_bank_load     load_first/last/random_state,     environment.py:219-227, :215-217
 *                    load_pokemon_center_state
 *   pk_reset_from    reset from a state of the pool    environment.py:116, :122, :1241-1242
 *   pk_bank_checkpoint / pk_bank_resume   no reference equivalent: a whole episode (machine state
 *                    and the Environment's per-episode attributes) saved to and continued from a slot
 *   pk_archive_update / pk_archive_explore   no reference equivalent: the best episode per cell key,
 *                    kept in bank slots, and envs resumed from cells drawn by visit count
 *   pk_traj_enable / pk_traj_get / pk_bank_traj_get   no reference equivalent: the actions of every
 *                    episode, recorded per env and carried through checkpoints, resumes and the archive
 *   pk_archive_pack / pk_archive_merge   no reference equivalent: an archive's cells as records and
 *                    whole-slot payloads, and their merge into the archive of another handle
 *   pk_frame_keys    no reference equivalent: Go-Explore's cell of a frame, the screen downscaled to a
 *                    few blocks and quantised to a few levels, as a 64-bit key for the archive
 *   pk_counts_update / pk_counts_pack / pk_counts_add   no reference equivalent: a table key -> visit count
 *                    on the device and the count-based bonus beta / sqrt(count) of every env's key
 * With PK_F_REWARD, pk_step also runs the reward stack of Environment.step
 * (environment.py:1338-1612) and pk_reset follows Environment.reset (:1233-1334).
 */
#ifndef POKEGYM_AMD_H
#define POKEGYM_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PK_ABI_VERSION 12
#define PK_STATE_V9_BYTES 142610u
#define PK_SCREEN_ROWS 144u
#define PK_SCREEN_COLS 160u

/* flags */
#define PK_F_RENDER 1u          /* rasterise the last frame of every step into the screen obs */
#define PK_F_REWARD 2u          /* reward stack + (72,80,4) obs + reference reset semantics */
#define PK_F_RELOAD_ON_RESET 4u /* reload the template state on EVERY reset (the reference
                                   reloads only on an env's first reset, environment.py:1241) */
#define PK_F_HEATMAP 8u         /* keep each env's 444x436 counts_map (environment.py:448, :648-679):
                                   int32, 774,336 B per env, persists across resets (PK_F_REWARD) */

/* per-env error codes (pk_error_ptr): where the reference's step/reset raises, the env stops
 * (reward 0, state frozen) and reports which exception the reference would have raised */
#define PK_ERR_NONE 0
#define PK_ERR_MAP_KEY 1        /* KeyError, MAP_ID_REF lookup (environment.py:739) */
#define PK_ERR_STUCK_ATTR 2     /* AttributeError, stuck_cnt read before assignment (:744) */
#define PK_ERR_MOVE_INDEX 3     /* IndexError, moves_obtained[move >= 0xA5] (:568, :580) */
#define PK_ERR_CUT_COORDS 4     /* UnboundLocalError, cut coords for an unknown facing (:1519) */
#define PK_ERR_HEATMAP_INDEX 5  /* IndexError, counts_map outside 444x436 (:676) */
#define PK_ERR_BUS_INDEX 6      /* IndexError, memory read past 0xFFFF (box scan, :574-578) */
#define PK_ERR_CAPACITY 7       /* device table full (no reference equivalent) */
#define PK_ERR_EMPTY_PARTY 8    /* ValueError, info["stats"]["highest_pokemon_level"] = max([]) (:1672) */

/* info telemetry record: the numeric scalars of info["stats"] (57) and info["reward"] (21),
 * environment.py:1621-1704, field order pokegym_amd/info.py FIELDS ("coord" is NaN without
 * PK_F_HEATMAP) */
#define PK_INFO_NFIELDS 79

typedef struct pk_config {
    uint32_t n_envs;             /* envs on this GPU */
    int32_t device;              /* HIP device ordinal */
    const uint8_t* rom;          /* host bytes of the cartridge ROM (MBC3 or ROM-only) */
    uint64_t rom_len;
    const uint8_t* state;        /* host bytes of a PyBoy v9 savestate, or NULL = power-on */
    uint64_t state_len;
    uint32_t frame_skip;         /* frames per env-step; pokegym uses 24 (pyboy_binding.py:72) */
    uint32_t release_frame;      /* button released before this frame; pokegym: 8 (:80).
                                    0 = pressed and released before the step's first frame.
                                    release_frame >= frame_skip: that frame is not part of the
                                    step, so the step releases nothing (the reference's loop
                                    never reaches i == release_frame, :79-81): the button stays
                                    down across the step's end and the next step presses its own
                                    button on top of it.  As both values are fixed per handle,
                                    a button once pressed is then held until the env's state is
                                    reloaded (reset, pk_load_env) */
    uint32_t flags;              /* PK_F_* */
    uint32_t max_episode_steps;  /* truncation horizon; pokegym default 20480 (environment.py:1233) */
    double reward_scale;         /* reset(reward_scale=4.0) (environment.py:1233); 0 = 4.0 */
} pk_config;

typedef struct pk_handle pk_handle;

int pk_create(const pk_config* cfg, pk_handle** out);
void pk_destroy(pk_handle* h);
const char* pk_last_error(void);
int pk_abi_version(void);

/* Reset envs whose env_mask_dev[e] != 0 (device u8[n]; NULL = all).  Without PK_F_REWARD:
 * reload the template state and zero the step counter.  With PK_F_REWARD: Environment.reset —
 * D778 |= 0x10, template reload on the env's first reset only (or always with
 * PK_F_RELOAD_ON_RESET), fresh episode bookkeeping, and the reset observation in pk_obs_ptr(). */
int pk_reset(pk_handle* h, const uint8_t* env_mask_dev, void* stream);

/* One env-step for all envs.
 *   actions_dev : device u8[n], values 0..7 = Down Left Right Up A B Start Select
 *                 (pyboy_binding.py:40 ACTIONS); 8 = press nothing (extension).
 *   screen_dev  : optional device u8[n][144][160] copy of the grey screen (0xFF/0x99/0x55/0x00);
 *                 the handle's own persistent buffer is pk_screen_ptr().  NULL = no copy.
 *   rew_dev     : optional device f64[n]; the step reward (PK_F_REWARD; 0 otherwise).
 *   term_dev / trunc_dev : optional device u8[n]; time >= max_episode_steps
 *                 (environment.py:1612-1613: terminated = truncated = done). */
int pk_step(pk_handle* h, const uint8_t* actions_dev, uint8_t* screen_dev, double* rew_dev,
            uint8_t* term_dev, uint8_t* trunc_dev, void* stream);

/* Sub-batch forms (PufferLib batch_size < num_envs, README.md:116-118: 72 envs stepped 24 at a
 * time): the same step / reset restricted to envs [env0, env0 + count).  env0 is a multiple of
 * 64 (a 64-env image group); the end may be anywhere up to n.  All arrays stay full-size (device
 * u8/f64[n]); only the range's elements are read or written, so disjoint ranges may run
 * concurrently on different streams (each range has its own reset lists).  A range that ends
 * inside a group leaves the rest of that group untouched; a caller that steps those envs
 * concurrently in another range cannot (no range starts inside a group), so sub-batches of any
 * size are laid out one per group-aligned slot (pokegym_amd VecEnv pads 24-env sub-batches to 64). */
int pk_step_range(pk_handle* h, uint32_t env0, uint32_t count, const uint8_t* actions_dev, double* rew_dev,
                  uint8_t* term_dev, uint8_t* trunc_dev, void* stream);
int pk_reset_range(pk_handle* h, uint32_t env0, uint32_t count, const uint8_t* env_mask_dev, void* stream);

/* Environment.reset(max_episode_steps, reward_scale) (environment.py:1233, :1258-1259): set the
 * episode length and reward scale for the following steps (all envs of the handle).  Synchronous
 * when the seen-coordinate set must grow for a longer episode (it restarts empty then); call it
 * before the reset it belongs to. */
int pk_set_episode_params(pk_handle* h, uint32_t max_episode_steps, double reward_scale);

/* Rasterise every env's 144 latched scanlines (the per-line SCX/SCY/WX/WY/tile-data latches that
 * pk_create / pk_load_env restore from a v9 savestate, or that the last rendered frame latched)
 * into the screen with K2, the HIP renderer of pk_step — PyBoy's renderer.scanline over a loaded
 * state (the reference's 264 savestate frames pin it). Stream-ordered. */
int pk_render_latched(pk_handle* h, void* stream);

/* device pointer to the persistent u8[n][144][160] grey screen */
uint8_t* pk_screen_ptr(pk_handle* h);
/* device pointer to the u8[n][72][80][4] observation (PK_F_REWARD), updated by pk_step/pk_reset */
uint8_t* pk_obs_ptr(pk_handle* h);
/* device pointer to u32[n] PK_ERR_* codes (PK_F_REWARD), sticky until the env's next reset */
const uint32_t* pk_error_ptr(pk_handle* h);
/* device pointers to the info telemetry of the last pk_step (PK_F_REWARD).  info_flag u8[n] = 1
 * where the reference's step built its info dict (done or time % 10000 == 0, environment.py:1621);
 * for those envs info f64[PK_INFO_NFIELDS][npad] (field-major, env stride = npad, the padded
 * env count: pk_info_stride) holds the record.  Replaces the info dict of Environment.step. */
const double* pk_info_ptr(pk_handle* h);
const uint8_t* pk_info_flag_ptr(pk_handle* h);
uint32_t pk_info_stride(const pk_handle* h);
/* device pointer to u32 [5][stride] event-monitor bits of the info step (ram_map_leanke.py
 * monitor_*_events, 130 bits in reward_tables.MONITORS order): the detailed_rewards_* and
 * *_events_aggregate dicts of the reference's info (environment.py:1706-1808) */
const uint32_t* pk_info_bits_ptr(pk_handle* h);
/* device pointer to the int32 [n][444][436] counts_map of every env (PK_F_HEATMAP), null without it */
int32_t* pk_heatmap_ptr(pk_handle* h);

/* Stream-ordered bulk RAM access for all envs: dense_dev[e * len + i] <-> guest address
 * addr + i of env e.  RAM regions only (0xC000-0xFDFF incl. echo, 0xFF80-0xFFFE). */
int pk_get_ram(pk_handle* h, uint16_t addr, uint32_t len, uint8_t* dense_dev, void* stream);
int pk_set_ram(pk_handle* h, uint16_t addr, uint32_t len, const uint8_t* dense_dev, void* stream);
uint32_t pk_num_envs(const pk_handle* h);

/* Synchronous host-side accessors (parity tests, reward host mirrors, debugging). */
int pk_peek(pk_handle* h, uint32_t env, uint16_t addr, uint32_t len, uint8_t* host_out);
int pk_poke(pk_handle* h, uint32_t env, uint16_t addr, uint32_t len, const uint8_t* host_in);
int pk_snapshot(pk_handle* h, uint32_t env, uint8_t* host_v9, uint64_t len);
int pk_load_env(pk_handle* h, uint32_t env, const uint8_t* host_v9, uint64_t len);
/* v9 savestates of envs [env0, env0 + count) into host_v9 (count * PK_STATE_V9_BYTES bytes,
 * env-major): the bulk form of pk_snapshot for whole-batch parity checks (synchronous) */
int pk_snapshot_range(pk_handle* h, uint32_t env0, uint32_t count, uint8_t* host_v9, uint64_t len);

/* Savestate bank: n_slots slots of machine state in device memory, for starting episodes from a
 * pool of savestates and for copying one env's state over another's without the host — the
 * batched form of the reference's state hooks (environment.py get_random_state :51, :116;
 * initial_states with load_first_state / load_last_state / load_random_state :122, :219-227;
 * save_state / load_pokemon_center_state :208-217).
 *
 * A slot holds what a parsed v9 savestate holds: the dense RAM image, the machine registers, the
 * 3 x 144 scanline latches and the 144 x 160 screen, about 74.5 KB.  The step counter and the
 * per-step bookkeeping registers are not machine state; a slot stores them as a freshly parsed
 * state has them (0).  The reward stack's bookkeeping (seen-coordinate sets, heat maps, the
 * per-episode attributes) is NOT in this machine part of a slot: a load leaves it as it is, a reset
 * rebuilds it.  A bank with episode parts (below) can carry it next to the machine part.
 *
 * pk_bank_create (synchronous): once per handle, before any other bank call; n_slots in
 * 1..65536.  On failure (second call, bad n_slots, out of memory) the handle stays usable and
 * has no bank.  pk_destroy frees the bank.  pk_bank_slots: the slot count, 0 without a bank.
 * Every other bank call on a handle without a bank fails with a negative code. */
int pk_bank_create(pk_handle* h, uint32_t n_slots);
uint32_t pk_bank_slots(const pk_handle* h);
/* Synchronous, host v9 bytes: put parses a savestate into a slot (as pk_create parses the
 * template) and marks it filled; get exports a filled slot exactly as pk_snapshot exports an env
 * (an empty slot fails).  The pool-from-files path and the parity path. */
int pk_bank_put(pk_handle* h, uint32_t slot, const uint8_t* host_v9, uint64_t len);
int pk_bank_get(pk_handle* h, uint32_t slot, uint8_t* host_v9, uint64_t len);
/* Stream-ordered, asynchronous, never a host sync.  slot_of_env_dev is a device i32[n], full
 * size and indexed by env like every array of the range forms; only [env0, env0 + count) is
 * read, env0 a multiple of 64 (pk_step_range's rule).  A negative slot: the env takes no part.
 * Disjoint ranges may run concurrently on different streams (the bank keeps its own lists per
 * range); the caller orders calls that touch the same slot.
 *   pk_bank_save   slot[slot_of_env[e]] <- env e, and marks the slot filled: pk_bank_get of the
 *                  slot then returns the bytes pk_snapshot(e) returned at that point of the stream.
 *                  Two envs naming one slot in one call is a caller error: the slot then holds an
 *                  unspecified mixture of the two.
 *   pk_bank_load   env e <- slot[slot_of_env[e]], with pk_load_env's semantics: the RAM image,
 *                  the machine registers, latches and screen; the env's step counter, per-step
 *                  bookkeeping and all reward-stack state survive.
 * A slot >= n_slots, or (load) an empty slot, never faults: that env is left untouched and the
 * bank's reject counter is incremented. */
int pk_bank_save(pk_handle* h, const int32_t* slot_of_env_dev, uint32_t env0, uint32_t count, void* stream);
int pk_bank_load(pk_handle* h, const int32_t* slot_of_env_dev, uint32_t env0, uint32_t count, void* stream);
/* pk_reset_range, except that an env that reloads its template reloads slot[slot_of_env[e]]
 * instead; a negative slot is the handle's own template.  Without PK_F_REWARD every masked env
 * reloads; with it the reload follows pk_reset's rule (the env's first reset only, or every
 * reset with PK_F_RELOAD_ON_RESET), between the same steps of Environment.reset.  An env whose
 * slot is >= n_slots or empty reloads the handle's template and is counted as a reject.
 * slot_of_env_dev == NULL is exactly pk_reset_range. */
int pk_reset_from(pk_handle* h, uint32_t env0, uint32_t count, const uint8_t* env_mask_dev,
                  const int32_t* slot_of_env_dev, void* stream);
/* Episode checkpoints.  After pk_bank_enable_episodes every slot can carry, next to its machine
 * part, the rest of an episode: the env's step counter and the lane registers the machine part
 * normalises, every per-episode attribute of the reward stack (the flags that survive resets and
 * the error code included: a frozen env checkpoints as frozen), the seen-coordinate set, the
 * visited mask of the current map and the cut coordinates.  An env resumed from such a slot and
 * fed the same actions produces the rewards, dones, observations, info records and machine
 * state of the env it was saved from, bit for bit.  Three things belong to the env and not to
 * the episode and are never restored: the tag of the env's seen table, its reset count (which
 * decides the env's template reloads) and the PK_F_HEATMAP counts_map with its running sum (the
 * "coord" info field) — the map stays with the env and keeps counting what is played on it.
 *
 * Memory: an episode part is 4 * cap + 8,448 bytes plus a 272-byte record, cap = the seen set's
 * capacity, the power of two >= max((max_episode_steps + 2) * 4 / 3, 1024): 139,792 bytes per
 * slot at the default 20,480 steps, besides the 74,512 of the machine part; size n_slots by that.
 *
 * pk_bank_enable_episodes (synchronous): once per handle, needs a bank and PK_F_REWARD; on
 * failure the handle is unchanged.  pk_bank_has_episodes: 1 after it, else 0.  Without it
 * pk_bank_checkpoint / pk_bank_resume fail with a negative code and change nothing.
 *   pk_bank_checkpoint  pk_bank_save, plus the episode part; both parts are marked filled.
 *   pk_bank_resume      pk_bank_load, plus the episode part and the step counter, then the
 *                       observation of the resumed envs is rebuilt (pk_obs_ptr shows the resumed
 *                       state before the next step).  Many envs may resume from one slot.
 * Arguments, ordering and concurrency are pk_bank_save's and pk_bank_load's.  A slot >= n_slots,
 * an empty slot or (resume) a slot without an episode part — one filled by pk_bank_put or
 * pk_bank_save, which leave the episode part empty — is a reject: the env is untouched in every
 * part and counted.  When pk_set_episode_params grows the seen set, the episode parts of all
 * slots are emptied (their tables are reallocated at the new size): a later resume from an older
 * checkpoint is a reject; the machine parts are kept. */
int pk_bank_enable_episodes(pk_handle* h);
int pk_bank_has_episodes(const pk_handle* h);
int pk_bank_checkpoint(pk_handle* h, const int32_t* slot_of_env_dev, uint32_t env0, uint32_t count, void* stream);
int pk_bank_resume(pk_handle* h, const int32_t* slot_of_env_dev, uint32_t env0, uint32_t count, void* stream);
/* Generic episode parts: checkpoints, resumes and the archive on a handle WITHOUT PK_F_REWARD, so on
 * any cartridge.  pk_bank_enable_episodes keeps refusing such a handle; this call gives its slots a
 * second kind of episode part, which carries what an episode consists of there:
 *   - every lane register raw (the step counter, the held buttons and window line, the CPU bits the
 *     machine part normalises), always;
 *   - PK_GEP_PROBES: the env's probe state words, so a resumed PK_PO_NEWMAX keeps its maximum and a
 *     resumed PK_PO_DELTA is measured from the checkpoint's value;
 *   - PK_GEP_STACK: the env's row of the frame stack, so a resumed policy sees the checkpoint's frames.
 * An env resumed from such a slot and fed the same actions produces the screens, machine states,
 * termination flags, probe rewards and features and stack rows of the env it was saved from, bit for
 * bit.  A part that was not asked for stays the destination env's, as before.
 *
 * Memory per slot, every part 16-byte aligned: 80 bytes of registers, 4 * (m rounded up to 4) bytes
 * with PK_GEP_PROBES, depth * H * W bytes with PK_GEP_STACK, besides the machine part.
 *
 * pk_bank_enable_generic_episodes (synchronous): once per handle; needs a bank, a handle without
 * PK_F_REWARD and, for each part asked for, the feature itself (pk_probe_create / pk_fstack_create
 * first).  On failure — PK_F_REWARD set, no bank, an unknown bit in parts, a part whose feature is
 * missing, a second call, out of memory — the handle is unchanged and a later correct call succeeds.
 * pk_bank_generic_parts: parts | 0x80000000 once enabled, else 0.  pk_bank_generic_episode_bytes: the
 * bytes per slot stated above, 0 without.  A handle that never calls it makes exactly the launches
 * and allocations it made before.
 *
 * After it pk_bank_has_episodes is 1, and pk_bank_checkpoint / pk_bank_resume run the list and
 * validation and the machine part's kernels as on a reward handle, then one mover for the generic
 * part and, with trajectories, the trajectory mover; there is no observation to rebuild.  Reject
 * rules, the reject counter, ordering and concurrency are unchanged: a rejected env is untouched in
 * every part, many envs may resume from one slot, pk_bank_put and pk_bank_save leave a slot's episode
 * part empty.  pk_traj_enable works before or after the call.  pk_set_episode_params never empties
 * generic parts (their size does not depend on the episode length); when it reallocates the
 * trajectory rows, the slots' rows are flagged PK_TRAJ_BROKEN.  pk_archive_create, _update, _explore
 * and _read work on top, with any keys (pk_frame_keys) and scores (accumulated probe reward).
 * pk_archive_exchange_enable fails with a negative code on such a handle and changes nothing: the
 * exchange payload has no format for generic parts. */
#define PK_GEP_PROBES 1u   /* carry the probe state words (needs pk_probe_create first) */
#define PK_GEP_STACK 2u    /* carry the frame stack planes (needs pk_fstack_create first) */
int pk_bank_enable_generic_episodes(pk_handle* h, uint32_t parts);
uint32_t pk_bank_generic_parts(const pk_handle* h);          /* parts | 0x80000000 once enabled, else 0 */
uint64_t pk_bank_generic_episode_bytes(const pk_handle* h);  /* bytes per slot of the generic part, 0 without */
/* Envs rejected by pk_bank_save / pk_bank_load / pk_reset_from / pk_bank_checkpoint /
 * pk_bank_resume since the last call; clears the counter (synchronous). */
int pk_bank_rejects(pk_handle* h, uint64_t* out);

/* Exploration archive (Go-Explore cells) on the bank: a map from 64-bit cell keys to bank slots
 * that keeps the best episode seen per cell, lives on the device and is driven without a host
 * sync.  Cell c owns bank slot slot0 + c for the life of the handle.  An archive holds, per cell,
 * key, score, length (the winner's step counter), visits and picks, and besides the cells in use,
 * an overflow count and the number of explore calls made.
 *
 * pk_archive_create (synchronous): once per handle; needs a bank with episode parts
 * (pk_bank_enable_episodes), n_cells in 1..65536 and slot0 + n_cells <= pk_bank_slots; seed seeds
 * the draws.  On failure (no episode parts, second call, bad range, out of memory) the handle is
 * unchanged.  pk_archive_cells: n_cells, 0 without an archive.  Every other archive call on a
 * handle without one fails with a negative code and does nothing.  Memory: 76 to 100 bytes per cell,
 * and per env of the handle 81 to 153 bytes of per-call words (the tables are powers of two).
 *
 * pk_cell_keys (any handle; no archive, no PK_F_REWARD needed; meaningful on Pokémon Red's WRAM
 * layout, pk_frame_keys below is the key of any cartridge): for each env of the range
 *   keys[e] = map | (x >> shift) << 8 | (y >> shift) << 16 | badges << 24
 * with map = guest 0xD35E, x = 0xD362, y = 0xD361, badges = 0xD356; shift in 0..7.  keys_dev is a
 * full-size device u64[n]; only [env0, env0 + count) is written.
 *
 * pk_archive_update: keys_dev u64[n], scores_dev f64[n], mask_dev u8[n] or NULL (= every env), full
 * size and indexed by env; the range follows pk_step_range's rule.  An env takes no part when its
 * mask byte is 0, its key is UINT64_MAX (reserved: "no cell") or its score is NaN.  The result is
 * the one of walking the envs that take part in ascending env index:
 *   - an env whose key has no cell gets the next free cell (visits = picks = 0, no record); when
 *     all n_cells are in use, overflow rises by one and the env does nothing more;
 *   - visits of the cell rises by one;
 *   - the env becomes the cell's record (score, length = its step counter) and the call's winner
 *     of the cell when the cell has no record, its score is greater, or its score is equal and
 *     its length less.  Scores compare as IEEE doubles.
 * So ties inside a call go to the lowest env, a stored record only yields to a strictly better
 * one, and new cells are numbered by the lowest env that reaches them, which also decides who
 * finds the archive full.  Every winner is then checkpointed into its cell's slot exactly as
 * pk_bank_checkpoint does it, at this point of the stream: the record and the slot never disagree.
 * slot_of_env_out_dev (optional device i32[n]) receives, over the range only, slot0 + c for the
 * winner of cell c and -1 for every other env.
 *
 * pk_archive_explore: every env of the range with mask_dev[e] != 0 (NULL = all) draws a cell and
 * resumes the episode in its slot exactly as pk_bank_resume does it (observation rebuilt).  With
 * the cells in use 0..used-1, their weights taken at the start of the call
 *   w(c) = 2^32 div isqrt((visits[c] + picks[c] + 1) << 16)          (integers)
 * P their inclusive prefix sums (u64) and T the total, env e draws
 *   r = mix(seed + 0x9E3779B97F4A7C15 * ((draw_calls << 32) + e + 1)) mod T     (mod 2^64 inside)
 * where mix is splitmix64's finaliser (z ^= z >> 30, z *= 0xBF58476D1CE4E5B9, z ^= z >> 27,
 * z *= 0x94D049BB133111EB, z ^= z >> 31), and takes the first c with P[c] > r.  After all draws
 * picks[c] has risen by the envs that drew c and draw_calls by one (per call, whatever its range):
 * all draws of a call see one distribution.  With an empty archive every masked env is a reject:
 * untouched, and counted in the bank's reject counter.  slot_of_env_out_dev (optional) receives
 * the slot each env resumed from, -1 for envs that took no part or were rejected (a cell whose
 * slot lost its episode part — pk_bank_put, pk_bank_save, a grown seen set — rejects like that).
 *
 * pk_archive_read (synchronous): host arrays of n_cells elements each, any pointer may be NULL;
 * elements from *used on are keys UINT64_MAX and zeros.  *overflow is not cleared by reading.
 *
 * Ordering: archive calls are stream-ordered and never sync the host.  The archive is one shared
 * structure: the caller orders the calls that touch it, as it orders bank calls that touch one
 * slot; calls over different ranges are allowed, but not concurrently.  Everything observable —
 * cell numbers, records, counters, draws, slot contents — is the same from run to run; only the
 * places of keys inside the hash tables depend on timing. */
int pk_archive_create(pk_handle* h, uint32_t slot0, uint32_t n_cells, uint64_t seed);
uint32_t pk_archive_cells(const pk_handle* h);
int pk_cell_keys(pk_handle* h, uint32_t shift, uint64_t* keys_dev, uint32_t env0, uint32_t count, void* stream);
int pk_archive_update(pk_handle* h, const uint64_t* keys_dev, const double* scores_dev, const uint8_t* mask_dev,
                      uint32_t env0, uint32_t count, int32_t* slot_of_env_out_dev, void* stream);
int pk_archive_explore(pk_handle* h, const uint8_t* mask_dev, uint32_t env0, uint32_t count,
                       int32_t* slot_of_env_out_dev, void* stream);
int pk_archive_read(pk_handle* h, uint32_t* used, uint64_t* keys, double* scores, uint32_t* lengths,
                    uint32_t* visits, uint32_t* picks, uint64_t* overflow);

/* Frame cells: Go-Explore's own cell, the frame downscaled and quantised, for any cartridge.  The
 * screen is cut into blocks of bw x bh pixels, bw a multiple of 8 that divides 160 (8, 16, 32, 40, 80,
 * 160) and bh one that divides 144 (8, 16, 24, 48, 72, 144); pk_frame_cells(bw, bh) is the number of
 * blocks C = (160 / bw) * (144 / bh), 0 for any other pair.  levels is in 2..256.
 *
 * pk_frame_keys, for each env e of the range, with mix splitmix64's finaliser (pk_archive_explore
 * above), G = 0x9E3779B97F4A7C15 and all sums mod 2^64:
 *   v(y, x) = screen[e][y][x] >> 6          0..3: 0xFF / 0x99 / 0x55 / 0x00 -> 3 / 2 / 1 / 0; any byte is legal
 *   block i = by * (160 / bw) + bx (row-major),  S_i = the sum of v over the block's bw * bh pixels
 *   q_i     = (S_i * levels) div (3 * bw * bh + 1)                          integers; 0..levels - 1
 *   sum     = the sum over i of mix(G * (i + 1) + q_i), plus mix(salt[e]) with a salt
 *   key     = mix(sum); UINT64_MAX becomes UINT64_MAX - 1 (the archive reserves UINT64_MAX)
 *             with a salt and salt[e] == UINT64_MAX: key = UINT64_MAX ("no cell" passes through)
 *   keys_dev[e] = key,  cells_dev[e][i] = q_i
 * The terms are added, not chained, so the result does not depend on the order of the reduction: it
 * is the same from run to run.
 *   screen_dev  NULL = the handle's own screen (pk_screen_ptr; needs PK_F_RENDER, the call fails
 *               without it), which every step rewrites and every reset, load, resume and merge
 *               restores; or a caller's device u8[n][144][160], 16-byte aligned, on any handle.
 *   salt_dev    NULL, or a full-size device u64[n], e.g. pk_cell_keys' output for a key of frame and
 *               RAM together (mix(0) = 0: a salt of 0 is the one salt that leaves the key as it is).
 *               It may be keys_dev itself: each env reads its word before writing it.
 *   keys_dev    required, full-size device u64[n].
 *   cells_dev   NULL, or a device u8[n][C]: the cell image, a small global observation.
 * Only the elements and rows of [env0, env0 + count) are written; the range follows pk_step_range's
 * rule, as pk_cell_keys' does.  One launch, stream-ordered, no host sync, no allocation; the archive
 * is not touched, so calls over disjoint ranges may run concurrently.  A failed call (bad bw, bh or
 * levels, NULL keys_dev, a misaligned screen_dev, a range past n) returns a negative code, sets
 * pk_last_error and writes nothing.  A handle that never calls it makes exactly the launches and
 * allocations it made before. */
uint32_t pk_frame_cells(uint32_t bw, uint32_t bh);
int pk_frame_keys(pk_handle* h, uint32_t bw, uint32_t bh, uint32_t levels, const uint8_t* screen_dev,
                  const uint64_t* salt_dev, uint64_t* keys_dev, uint8_t* cells_dev, uint32_t env0, uint32_t count,
                  void* stream);

/* Action trajectories: how an env got where it is.  After pk_traj_enable every env has
 *   actions  u8[capacity]  the action of every step since the env's last reset, one byte per step
 *   origin   i32           the bank slot the episode's machine was reloaded from, -1 = the handle's
 *                          template
 *   flags    u8            PK_TRAJ_* bits
 * and a length, the env's step counter clamped to the capacity.  Emulator and reward stack are
 * deterministic, so resetting an env from `origin` and stepping it through `actions` rebuilds the
 * machine, the rewards and the whole episode bookkeeping bit for bit — while flags is 0:
 *   PK_TRAJ_BROKEN    the actions no longer determine the state: the env's machine was changed
 *                     from outside (pk_bank_load, pk_load_env, pk_poke: the envs touched; pk_set_ram:
 *                     every env), its last reset did not reload the machine (with PK_F_REWARD and
 *                     without PK_F_RELOAD_ON_RESET only an env's first reset reloads; origin is -1
 *                     then), the env had already stepped when pk_traj_enable was called, or the
 *                     rows were reallocated.  Recording goes on; a reloading reset clears the flag.
 *   PK_TRAJ_OVERFLOW  the env was stepped past the capacity — only possible by stepping a done env
 *                     without resetting it; the first `capacity` actions are intact.
 *   PK_TRAJ_EMPTY     pk_bank_traj_get only: the slot holds no episode.
 * An origin names a slot's CONTENT at the time of the reset: the caller keeps the slots it resets
 * from unchanged for as long as it wants to replay (VecEnv's state-pool slots never change).
 *
 * capacity = 3 << (cap_log2 - 2) bytes, cap_log2 the log2 of the seen set's capacity (above): 768
 * at the 1,024-entry minimum, 24,576 at the default 20,480 steps; always a multiple of 16 and
 * >= max_episode_steps.  It grows exactly when pk_set_episode_params grows the seen set (on a
 * handle without PK_F_REWARD: when the same rule would): the rows are reallocated and every env is
 * flagged PK_TRAJ_BROKEN until its next reloading reset.
 *
 * pk_traj_enable (synchronous): once per handle, with or without PK_F_REWARD, before or after
 * pk_bank_enable_episodes.  On failure (second call, out of memory) the handle is unchanged.
 * pk_traj_capacity: the capacity, 0 without trajectories.  A handle that never enables them makes
 * exactly the launches and allocations it made before, and pk_traj_get / pk_bank_traj_get fail on
 * it with a negative code.  With them, pk_step_range makes one more small launch after the step
 * kernel, every reset one, and pk_bank_load / pk_set_ram / pk_load_env / pk_poke one.
 *
 * Slots: while the bank carries episode parts, every slot carries a trajectory part as well (one
 * more u8[capacity] row, origin and flags per slot; its length is the step counter of the slot's
 * episode part).  pk_bank_checkpoint moves env -> slot and pk_bank_resume slot -> env, right after
 * the episode part and over the same validated list: rejected envs are untouched, many envs may
 * resume from one slot, a resumed env's later actions are appended to the slot's.  pk_bank_put
 * and pk_bank_save leave it empty together with the episode part.  pk_archive_update and
 * pk_archive_explore checkpoint and resume through the same path: a cell's slot holds the
 * actions that reach the cell, an env that explores from it carries them on.
 *
 * pk_traj_get (stream-ordered gather): origin_dev i32[n], len_dev u32[n], flags_dev u8[n],
 * actions_dev u8[n][capacity] (16-byte aligned), full size and indexed by env; any pointer may be
 * NULL; the range follows pk_step_range's rule and only its elements are written.
 * pk_bank_traj_get: the same for slots [slot0, slot0 + count), the arrays indexed by slot - slot0
 * (actions_dev u8[count][capacity]); a slot without an episode part reads as origin -1, length
 * 0, flags PK_TRAJ_EMPTY.  In both, the bytes of a row from the length on are written as 0xFF, so
 * two results compare byte for byte. */
#define PK_TRAJ_BROKEN 1u
#define PK_TRAJ_OVERFLOW 2u
#define PK_TRAJ_EMPTY 4u
int pk_traj_enable(pk_handle* h);
uint32_t pk_traj_capacity(const pk_handle* h);
int pk_traj_get(pk_handle* h, uint32_t env0, uint32_t count, int32_t* origin_dev, uint32_t* len_dev,
                uint8_t* flags_dev, uint8_t* actions_dev, void* stream);
int pk_bank_traj_get(pk_handle* h, uint32_t slot0, uint32_t count, int32_t* origin_dev, uint32_t* len_dev,
                     uint8_t* flags_dev, uint8_t* actions_dev, void* stream);

/* Archive exchange: cells leave a handle as records and payloads and enter another handle's archive
 * by a merge — between the GPUs of a run (one handle per GPU), or to and from a file.
 *
 * A record (pk_xrec) is a cell's bookkeeping.  A payload is the cell's whole slot as
 * pk_archive_payload_bytes() linear bytes, every part at a 16-byte-aligned offset, in this order:
 *   machine part   RAM image | 20 register words | 3 x 144 latch words | 144 x 160 screen
 *   episode part   68 record words | seen table (normalised tags) | visited mask | cut coordinates
 *   trajectory     {origin, flags, 0, 0} | action row at its capacity     (handles with pk_traj_enable)
 * The total is a multiple of 16 and depends only on the handle's geometry, which
 * pk_archive_format() names: payload layout version << 24 | trajectories << 23 | cap_log2 << 16 |
 * the low 16 bits of the RAM image size.  Handles exchange cells only when their formats are equal;
 * both values change when pk_set_episode_params grows the seen set.  A slot's content does not
 * depend on the handle (dense image, normalised registers and seen tags, linear action row), so a
 * merged slot is the source slot, byte for byte.  The trajectory origin is copied verbatim: it names
 * a slot of the SOURCE's bank, so keeping the state pools of exchanging handles identical is the
 * caller's job.
 *
 * pk_archive_exchange_enable (synchronous): once per handle, needs an archive whose slots carry the
 * reward stack's episode parts (generic episode parts have no payload format: -ENOTSUP).  It allocates three
 * words per cell (sent_visits, sent_picks, dirty; all 0) and the scratch of pk_archive_merge, which
 * therefore never allocates for up to 65,536 records.  On failure the handle is unchanged.  A
 * handle that never calls it makes exactly the launches and allocations it made before; on it
 * pk_archive_pack / pk_archive_merge fail with a negative code and change nothing, and
 * pk_archive_payload_bytes is 0.  After it, pk_archive_update sets dirty[c] whenever a winner
 * replaces cell c's record — the only change on an existing path.  Records made before the call are
 * not dirty: a full pack ships them, a delta pack only their counts.
 *
 * pk_archive_pack (stream-ordered, never a host sync): cells c = cell0 .. cell0 + count - 1 in
 * order, record i = c - cell0 into rec_dev[i] (device pk_xrec[count], 16-byte aligned).
 *   - c >= the cells in use: key UINT64_MAX, zeros elsewhere, payload -1.
 *   - otherwise key, score and length are the cell's record, format this handle's.
 *   - flags == 0: visits and picks are the cell's full counts; every cell gets a payload, numbered
 *     0, 1, ... in ascending cell order until max_payloads are given, later cells get -1.  The
 *     archive is not changed in any way.
 *   - PK_XCHG_DELTA: visits = visits[c] - sent_visits[c] and then sent_visits[c] = visits[c], picks
 *     likewise (mod 2^32): what this handle counted itself since the last delta pack.  A cell gets
 *     a payload only if dirty[c] is set, in ascending cell order until max_payloads are given;
 *     those cells' dirty is cleared, the remaining dirty cells stay dirty (payload -1 this time).
 * Payload k is written to payload_dev + k * pk_archive_payload_bytes() (16-byte aligned; NULL only
 * with max_payloads == 0); *n_payloads_dev (optional device u32) receives the number written.
 * cell0 + count <= pk_archive_cells, count >= 1.
 *
 * pk_archive_merge (stream-ordered, never a host sync, no allocation): n_records in 1..65536.  The
 * result is the one of walking the records i = 0 .. n_records - 1 in ascending order:
 *   - a record with key UINT64_MAX is skipped;
 *   - a record whose format differs from this handle's, whose payload is >= n_payloads or whose
 *     score is NaN is a reject: ignored, and counted in the bank's reject counter;
 *   - if the key has no cell: with a payload and a free cell the record gets the next free cell
 *     (visits = picks = 0, no record yet); otherwise (no payload, or the archive is full) overflow
 *     rises by one and the record does nothing more;
 *   - visits[c] += rec.visits, picks[c] += rec.picks, and sent_visits[c] / sent_picks[c] rise by the
 *     same amounts, so counts that came from elsewhere are never sent on (all sums mod 2^32);
 *   - a record with a payload becomes the cell's record, and the call's winner of the cell, when
 *     the cell has no record, its score is greater, or its score is equal and its length less
 *     (pk_archive_update's rules: a stored record only yields to a strictly better one, ties
 *     inside a call go to the lower record index).
 * A merge never sets dirty: records that came from elsewhere are not sent on by a later delta pack.
 * Every winner's payload is then written into slot slot0 + c, all parts, and the slot is marked
 * filled, with an episode part: pk_bank_get, pk_bank_traj_get and a pk_bank_resume plus continuation
 * from that slot equal those of the source slot, bit for bit.  cell_out_dev (optional device
 * i32[n_records]) receives c for the winner of cell c and -1 for every other record.  A negative
 * payload is "no payload".  payload_dev may be NULL only with n_payloads == 0.
 *
 * Bad arguments (a range past pk_archive_cells, a NULL rec_dev, a misaligned pointer, n_records
 * out of range) are a negative return code, never a fault.  Everything observable is the same
 * from run to run, as for the rest of the archive, and the concurrency rule is the archive's: the
 * caller orders the calls that touch it. */
#define PK_XCHG_DELTA 1u
typedef struct pk_xrec {           /* 48 bytes, 16-byte aligned */
    uint64_t key;
    double score;
    uint32_t length, visits, picks;
    int32_t payload;               /* row of the payload array, -1 = none */
    uint32_t format;               /* pk_archive_format() of the packing handle */
    uint32_t reserved[3];          /* 0 */
} pk_xrec;
int pk_archive_exchange_enable(pk_handle* h);
uint64_t pk_archive_payload_bytes(const pk_handle* h);
uint32_t pk_archive_format(const pk_handle* h);
int pk_archive_pack(pk_handle* h, uint32_t flags, uint32_t cell0, uint32_t count, uint32_t max_payloads,
                    pk_xrec* rec_dev, uint8_t* payload_dev, uint32_t* n_payloads_dev, void* stream);
int pk_archive_merge(pk_handle* h, const pk_xrec* rec_dev, uint32_t n_records, const uint8_t* payload_dev,
                     uint32_t n_payloads, int32_t* cell_out_dev, void* stream);

/* Visit counts: a persistent table key -> count on the device, for a count-based exploration bonus
 * (Tang et al., "#Exploration") over any 64-bit key — pk_frame_keys' frame cell on any cartridge,
 * pk_cell_keys on Pokémon Red.  Every env of a range counts its key and gets the key's new count and
 * beta / sqrt(count) back, stream-ordered and without a host sync.  It needs nothing else: no
 * PK_F_REWARD, no bank, no archive.
 *
 * pk_counts_create (synchronous): once per handle, on any handle; cap_log2 in 10..30.  The table has
 * 2^cap_log2 entries of {key u64, count u64, sent u64} (24 bytes each, plus 4 bytes per env) and takes
 * limit = 3 * 2^(cap_log2 - 2) distinct keys: pk_counts_limit, 0 without a table.  On failure (second
 * call, bad cap_log2, limit < n_envs, out of memory) the handle is unchanged.  Every other counts call
 * on a handle without a table fails with a negative code and does nothing.  A handle that never
 * creates a table makes exactly the launches and allocations it made before.
 *
 * Placement: an entry's probe starts at the low cap_log2 bits of mix(key), mix splitmix64's finaliser
 * (pk_archive_explore above); probing is linear, to the next entry, and wraps from the last entry
 * to entry 0.  Where a key sits is not observable; the rule is stated so that a test can build keys
 * that share a probe sequence.
 *
 * pk_counts_update (stream-ordered, never a host sync, no allocation, two launches): keys_dev u64[n],
 * mask_dev u8[n] or NULL (= every env), counts_out_dev u64[n] or NULL, bonus_out_dev f64[n] or NULL,
 * full size and indexed by env; the range follows pk_step_range's rule.  The participants P are the
 * envs of the range whose mask byte is not 0 and whose key is not UINT64_MAX (reserved, as in the
 * archive: "no cell").  With `used` the distinct keys stored when the call starts, the call is open
 * when used + count <= limit — count the size of the range, not of P — and closed otherwise.
 *   - open: every key of P that is not stored is inserted with count 0, and used rises by their number;
 *   - closed: nothing is inserted; a participant whose key is not stored adds 1 to overflow and gets
 *     count 0 and bonus 0.0, the keys that are stored are counted as usual.
 * A call thus admits all of its new keys or none, whatever the order of its envs, and used never
 * exceeds limit.  With c0(k) the stored count of key k and m(k) the participants that hold k, the new
 * count is c(k) = c0(k) + m(k), and every participant e that holds k gets
 *   counts_out[e] = c(k),  bonus_out[e] = beta / sqrt((double)c(k))        IEEE f64, correctly rounded
 * The other envs of the range get 0 and 0.0; nothing outside the range is written.
 * PK_COUNTS_PEEK: the table, used and overflow stay as they are; the outputs are those of c0 (0 and 0.0
 * for a key that is not stored).
 *
 * pk_counts_add (stream-ordered, no allocation): the same rule over records, c(k) += rec.count.  rec_dev
 * is a device pk_crec[n_records], 16-byte aligned, n_records in 1..2^30.  A record with key UINT64_MAX
 * or count 0 is skipped.  The call is open when used + n_records <= limit; when closed, every record
 * whose key is not stored adds 1 to overflow.  PK_COUNTS_FOREIGN raises the key's sent word by the
 * same amount: counts that came from another handle are never sent on (pk_archive_merge's rule).
 *
 * pk_counts_pack (stream-ordered, one launch): one record per stored key whose packed count is not 0.
 * The packed count is the key's count, or with PK_COUNTS_DELTA count - sent, after which sent = count:
 * what this handle counted itself since its last delta pack.  The order of the records is
 * unspecified, their set is fixed.  rec_dev is a device pk_crec[max_records], 16-byte aligned;
 * *n_out_dev (device u32, required) receives the number written.  max_records < pk_counts_limit is
 * refused, so a pack is never cut short.
 *
 * pk_counts_read (synchronous): the distinct keys stored and the overflow count (not cleared by
 * reading); either pointer may be NULL.  pk_counts_clear (stream-ordered): the table is empty again,
 * used and overflow 0.
 *
 * Ordering: the table is one shared structure; the caller orders the calls that touch it, as for the
 * archive: calls over different ranges are allowed, but not concurrently.  Everything observable
 * — counts, bonuses, used, overflow, the set a pack writes — is the same from run to run.  Bad
 * arguments (no table, NULL keys_dev or rec_dev, a range past n, an env0 that is no multiple of 64,
 * n_records out of range, a misaligned rec_dev, unknown flag bits) are a negative code with
 * pk_last_error, never a fault, and write nothing. */
#define PK_COUNTS_PEEK 1u      /* pk_counts_update: read only */
#define PK_COUNTS_FOREIGN 1u   /* pk_counts_add: counts that came from another handle */
#define PK_COUNTS_DELTA 1u     /* pk_counts_pack: only what this handle counted itself since the last delta pack */
typedef struct pk_crec { uint64_t key, count; } pk_crec;      /* 16 bytes */
int pk_counts_create(pk_handle* h, uint32_t cap_log2);
uint64_t pk_counts_limit(const pk_handle* h);
int pk_counts_update(pk_handle* h, const uint64_t* keys_dev, const uint8_t* mask_dev, uint32_t env0, uint32_t count,
                     double beta, uint32_t flags, uint64_t* counts_out_dev, double* bonus_out_dev, void* stream);
int pk_counts_add(pk_handle* h, const pk_crec* rec_dev, uint32_t n_records, uint32_t flags, void* stream);
int pk_counts_pack(pk_handle* h, uint32_t flags, pk_crec* rec_dev, uint64_t max_records, uint32_t* n_out_dev,
                   void* stream);
int pk_counts_read(pk_handle* h, uint64_t* used, uint64_t* overflow);
int pk_counts_clear(pk_handle* h, void* stream);

/* Frame stack: a downscaled, k-deep frame history per env, kept on the device and updated in place
 * by one launch per step — the observation of a pixel policy on any cartridge (the reference's
 * screen[::2, ::2] and its 3-deep recent_frames, newest first).  It needs nothing else: no
 * PK_F_REWARD, no bank.
 *
 * Geometry: scale s is 1, 2 or 4, a plane is H x W = (144 / s) x (160 / s) bytes (scale 8 is left
 * out: an 18 x 20 plane is no multiple of 16 bytes).  depth D is 1..8 with PK_FSTACK_CHW, u8[n][D][H][W],
 * and 1, 2, 4 or 8 with PK_FSTACK_HWC, u8[n][H][W][D].  Plane 0 is always the newest.  The stack takes
 * n * D * H * W bytes: 23,040 per env at s = 2, D = 4, 1.5 GB at 65,536 envs.  HWC at s = 2, D = 4 has
 * the reference observation's shape (72, 80, 4); CHW at s = 4, D = 3 is its 3 x 36 x 40 screen stack.
 *
 * The plane p of a screen, for any byte values, in integers:
 *   PK_FSTACK_MEAN   p[y][x] = (sum over dy, dx < s of screen[s*y + dy][s*x + dx] + s*s/2) div (s*s)
 *   PK_FSTACK_PICK   p[y][x] = screen[s*y][s*x]
 * With s = 1 both are the screen.
 *
 * pk_fstack_create (synchronous): once per handle, on any handle; the stack starts as all zeros.  On
 * failure (second call, bad argument, out of memory) the handle is unchanged.  pk_fstack_depth and
 * pk_fstack_scale are 0 and pk_fstack_ptr is NULL without a stack, and pk_fstack_push then fails with
 * a negative code.  A handle that never creates one makes exactly the launches and allocations it
 * made before.  pk_fstack_ptr is a device pointer the handle owns, valid until pk_destroy.
 *
 * pk_fstack_push (one launch, stream-ordered, no host sync, no allocation): screen_dev NULL is the
 * handle's own screen (needs PK_F_RENDER, the call fails without it), otherwise a caller's device
 * u8[n][144][160], 16-byte aligned — pk_frame_keys' rules.  mask_dev is NULL or a full-size device
 * u8[n]; the range follows pk_step_range's rule.
 *   flags == 0: every env of the range takes part.  With mask[e] != 0 the env FILLS: all D planes
 *     become the new plane.  Otherwise (a NULL mask included) it PUSHES: plane k becomes the old
 *     plane k - 1 for k = D - 1 .. 1 and plane 0 the new plane.
 *   PK_FSTACK_FILL_ONLY: only the envs with mask[e] != 0 take part (a NULL mask: every env of the
 *     range), and they fill; the other envs keep every byte.
 * Nothing outside the rows of [env0, env0 + count) is written, so disjoint ranges may run
 * concurrently on different streams.  Bad arguments (no stack, unknown flag bits, a misaligned
 * screen pointer, a range past n, an env0 that is no multiple of 64) are a negative code with
 * pk_last_error, never a fault, and write nothing.
 *
 * A stack row is carried by generic episode parts when requested (PK_GEP_STACK: checkpoints,
 * resumes and the archive of a handle without PK_F_REWARD).  Otherwise it belongs to the env, not to
 * the episode or the machine: bank slots, checkpoints, the archive and the exchange payload do not
 * carry it and keep their formats, and the caller refills (PK_FSTACK_FILL_ONLY) an env whose
 * machine was replaced; VecEnv(frame_stack=D) does. */
#define PK_FSTACK_CHW 0u        /* u8[n][depth][H][W] */
#define PK_FSTACK_HWC 1u        /* u8[n][H][W][depth] */
#define PK_FSTACK_MEAN 0u
#define PK_FSTACK_PICK 1u
#define PK_FSTACK_FILL_ONLY 1u  /* pk_fstack_push flag */
int pk_fstack_create(pk_handle* h, uint32_t scale, uint32_t depth, uint32_t layout, uint32_t mode);
uint32_t pk_fstack_depth(const pk_handle* h);       /* 0 without a stack */
uint32_t pk_fstack_scale(const pk_handle* h);       /* 0 without a stack */
uint8_t* pk_fstack_ptr(pk_handle* h);               /* device pointer, owned by the handle; NULL without */
int pk_fstack_push(pk_handle* h, const uint8_t* screen_dev, const uint8_t* mask_dev, uint32_t flags,
                   uint32_t env0, uint32_t count, void* stream);

/* RAM probes: a reward, a done flag and a feature vector read from every env's RAM by a small program
 * given once per handle — the host-side mem_val / bit_count / BCD reads of a reward function, for a
 * whole range of envs in one launch and on any cartridge.  It needs nothing else: no PK_F_REWARD, no
 * bank.  Everything is exact in integers; only the reward is a double, with a stated rounding.
 *
 * A program is m probes, 1..64.  Probe j has `count` elements, 1..64; element k lies at the guest
 * addresses [addr + k * stride, addr + k * stride + len) (stride is ignored when count == 1), every
 * byte of it inside what pk_get_ram accepts — WRAM and its echo, 0xC000-0xFDFF, an element not
 * wrapping the echo mirror, or HRAM, 0xFF80-0xFFFE.  The value of an element, for any byte values:
 *   PK_PV_LE    len 1..3    little-endian unsigned
 *   PK_PV_BE    len 1..3    big-endian unsigned
 *   PK_PV_BCD   len 1..3    big-endian packed BCD: x = 0, then x = 10 * x + nibble over the 2 * len
 *                           nibbles, most significant first; a nibble above 9 counts as it is
 *   PK_PV_BITS  len 1..512  the number of set bits in the len bytes
 * The probe's value v is the PK_PR_SUM or the PK_PR_MAX of its elements; v < 2^30 by these bounds.
 *
 * Per env and probe the handle keeps one u32 word s, 0 after pk_probe_create; its layout is the
 * kernel's business.  The probe's contribution c to the reward, by op:
 *   PK_PO_NONE    a feature only: nothing is added, s is never written
 *   PK_PO_DELTA   c = weight * (double)((int64)v - (int64)s);               then s = v
 *   PK_PO_NEWMAX  c = v > s ? weight * (double)(v - s) : +0.0;              then s = max(s, v)
 *   PK_PO_CHANGE  c = v != s ? weight : +0.0;                               then s = v
 * The done term of a probe compares v with arg as unsigned numbers: PK_PC_NONE (never), EQ, NE, GE,
 * LE; an env's done is the OR over its probes.  The reward r of an env starts at +0.0 and takes the
 * contributions of the probes with op != PK_PO_NONE in ascending probe index; every product and every
 * sum is rounded once to IEEE f64 — no fused multiply-add — so r is the same bits as the same
 * statements in numpy (pokegym_amd/probes.py model()).
 *
 * pk_probe_create (synchronous): once per handle, on any handle; prog_host is a host array of m
 * pk_probe.  On failure — a second call, m outside 1..64, an unknown kind, reduce, op or cmp, a len
 * outside its kind's range, a count outside 1..64, a weight that is not finite, an element with a
 * byte outside the ranges above, out of memory — the handle is unchanged (a later correct call
 * succeeds).  pk_probe_count is m, 0 without a program.  A handle that never creates one makes
 * exactly the launches and allocations it made before.
 *
 * pk_probe_eval (one launch, stream-ordered, no host sync, no allocation): mask_dev is NULL or a
 * device u8[n], rew_dev f64[n], term_dev u8[n], feat_dev i32[n][m]; each of the three outputs may be
 * NULL; all are full size and indexed by env.  The range follows pk_step_range's rule.
 *   flags == 0: every env of the range takes part.  With mask[e] != 0 the env REBASES: s_j = v_j for
 *     every probe with op != PK_PO_NONE; its rew and term elements are not touched.  Otherwise (a
 *     NULL mask included) it EVALUATES: the states move as stated above, rew[e] = rew[e] + r (one
 *     more rounded sum) and term[e] |= done.
 *   PK_PROBE_REBASE_ONLY: only the envs with mask[e] != 0 take part (a NULL mask: every env of the
 *     range), and they rebase; the other envs keep every byte, of state and of outputs.
 *   PK_PROBE_SET (it only changes what an evaluating env does, so with REBASE_ONLY it does
 *     nothing): an evaluating env gets rew[e] = r and term[e] = done in the place of the sum and
 *     the OR.
 * Row e of feat_dev receives v_0 .. v_{m-1} for every env that takes part, rebasing or evaluating.
 * Nothing outside the elements of [env0, env0 + count) is written, so disjoint ranges may run
 * concurrently on different streams.  Bad arguments (no program, unknown flag bits, a range past n,
 * an env0 that is no multiple of 64) are a negative code with pk_last_error, never a fault, and write
 * nothing.
 *
 * The state is carried by generic episode parts when requested (PK_GEP_PROBES: checkpoints, resumes
 * and the archive of a handle without PK_F_REWARD; a resumed PK_PO_NEWMAX then keeps its maximum).
 * Otherwise it belongs to the env, as the frame stack does: bank slots, checkpoints, the archive and
 * the exchange payload do not carry it and keep their formats, and the caller rebases
 * (PK_PROBE_REBASE_ONLY) an env whose machine was replaced — a reset, a load, a resume — so a resumed
 * PK_PO_NEWMAX starts again from the current value; VecEnv(probes=...) does. */
#define PK_PV_LE 0u
#define PK_PV_BE 1u
#define PK_PV_BCD 2u
#define PK_PV_BITS 3u
#define PK_PR_SUM 0u
#define PK_PR_MAX 1u
#define PK_PO_NONE 0u
#define PK_PO_DELTA 1u
#define PK_PO_NEWMAX 2u
#define PK_PO_CHANGE 3u
#define PK_PC_NONE 0u
#define PK_PC_EQ 1u
#define PK_PC_NE 2u
#define PK_PC_GE 3u
#define PK_PC_LE 4u
#define PK_PROBE_REBASE_ONLY 1u   /* pk_probe_eval flags */
#define PK_PROBE_SET 2u
#define PK_PROBE_MAX 64u          /* probes of a program, and elements of a probe */
typedef struct pk_probe {          /* 24 bytes */
    uint16_t addr;                 /* guest address of element 0 */
    uint16_t len;                  /* bytes per element */
    uint16_t count;                /* elements, 1..64 */
    uint16_t stride;               /* bytes from one element to the next (ignored when count == 1) */
    uint8_t kind, reduce, op, cmp; /* PK_PV_*, PK_PR_*, PK_PO_*, PK_PC_* */
    uint32_t arg;                  /* the constant of cmp */
    double weight;                 /* finite */
} pk_probe;
int pk_probe_create(pk_handle* h, const pk_probe* prog_host, uint32_t m);
uint32_t pk_probe_count(const pk_handle* h);          /* 0 without a program */
int pk_probe_eval(pk_handle* h, const uint8_t* mask_dev, uint32_t flags, uint32_t env0, uint32_t count,
                  double* rew_dev, uint8_t* term_dev, int32_t* feat_dev, void* stream);

/* Tile view: the screen as 18 x 20 tile ids and object ids, computed on the device from the machine
 * state a step leaves — the symbolic observation Game Boy RL feeds a policy (the visible tile matrix
 * plus the sprite list), 360 or 720 small integers per env in the place of 23,040 grey bytes.  It
 * needs nothing else: no PK_F_RENDER (a headless handle has it), no PK_F_REWARD, no bank.
 *
 * The tile view of an env is THE FRAME THE PPU WOULD DRAW IF THE REGISTERS HELD AT THE END OF THE STEP
 * HAD HELD FOR THE WHOLE FRAME, sampled once per 8 x 8 screen cell: u16[n][P][18][20], plane 0 the
 * background / window, plane 1 (P = 2, with PK_TILES_OBJ) the objects; 0xFFFF means "nothing".  It
 * reads LCDC, SCY, SCX, WY, WX as the step left them, the VRAM image and the OAM image, all in
 * integers.  It is not the pixels where a game writes scroll or LCDC registers mid-frame, puts
 * more than ten objects on a line or toggles the window mid-frame (the window's line counter):
 * that is the price of not rasterising.
 *
 * Plane 0, cell (r, c), sample pixel (x, y) = (8c, 8r):
 *   LCDC.7 = 0 or LCDC.0 = 0      0xFFFF
 *   window cell                   when LCDC.5 is set, y >= WY, WX <= 166 and x + 7 >= WX: map row
 *                                 (y - WY) >> 3, map column (x + 7 - WX) >> 3, the map LCDC.6 selects
 *                                 (0x9C00 when set, else 0x9800)
 *   background cell               otherwise: map row ((y + SCY) & 255) >> 3, map column
 *                                 ((x + SCX) & 255) >> 3, the map LCDC.3 selects
 *   tile id                       with map byte t: t when LCDC.4 is set or t >= 128, else 256 + t — ids
 *                                 run 0..383 and id * 16 is the tile's offset in VRAM
 * Plane 1: all 0xFFFF when LCDC.7 = 0 or LCDC.1 = 0.  Otherwise OAM entry i = (Y, X, T, attr), i =
 * 0..39, sits at oy = Y - 16, ox = X - 8 and its home cell is r = (oy + 4) >> 3, c = (ox + 4) >> 3
 * (arithmetic shifts: the nearest cell; there is no ten-per-line limit).  An 8 x 8 object (LCDC.2 = 0)
 * puts T into (r, c).  An 8 x 16 object puts T & 0xFE into (r, c) and T | 1 into (r + 1, c), the two
 * values swapped when attr bit 6 (Y flip) is set.  A cell outside the 18 x 20 grid is dropped, each on
 * its own.  Where several objects claim a cell the smaller X wins, then the lower i (the DMG
 * priority rule).
 *
 * Mode: PK_TILES_ID stores the ids above.  PK_TILES_HASH with bits in 8..15 stores, in the place of
 * every id (of both planes; 0xFFFF stays), a hash of the tile's 16 data bytes — games reload tile
 * data, so an id is a slot and not a picture: with w0..w3 the little-endian dwords at VRAM offset
 * id * 16 (objects: T * 16 of the tile they show),
 *   h = mix((w0 | w1 << 32) ^ mix((w2 | w3 << 32) + 0x9E3779B97F4A7C15))
 * in 64-bit arithmetic, mix being splitmix64's finaliser (pk_archive_explore states it), and the stored
 * value is h & ((1 << bits) - 1).  Flips and palettes do not enter it.
 *
 * Key (optional): with v_i the i-th u16 of the env's view in output order, i = 0 .. P * 360 - 1,
 *   key = mix(salt ^ XOR_i mix(v_i + (i + 1) * 0x9E3779B97F4A7C15))
 * where salt = salt_dev[e], 0 without salt_dev.  The XOR makes the key independent of the order of
 * the reduction.  As in pk_frame_keys the reserved key 0xFFFF...F is never produced (it becomes
 * 0xFFFF...E), except that a salt of 0xFFFF...F ("no cell") gives the key 0xFFFF...F.
 *
 * pk_tiles_create (synchronous): once per handle, on any handle; mode is PK_TILES_ID (bits is
 * ignored) or PK_TILES_HASH (bits 8..15), flags 0 or PK_TILES_OBJ.  The view starts as all 0xFFFF.  On
 * failure (second call, unknown mode or flag bits, bits out of range, out of memory) the handle is
 * unchanged.  pk_tiles_planes is P, 0 without a view; pk_tiles_ptr a device pointer the handle owns,
 * valid until pk_destroy, NULL without a view.  A handle that never creates one makes exactly the
 * launches and allocations it made before.
 *
 * pk_tiles_eval (one launch, stream-ordered, no host sync, no allocation): the envs of the range
 * with mask_dev[e] != 0 (a NULL mask: every env of the range) get their rows of the view and, with
 * keys_dev, their keys; every other env keeps both.  mask_dev is a device u8[n], salt_dev and keys_dev
 * device u64[n], each may be NULL, all full size and indexed by env; salt_dev may be keys_dev.  The
 * range follows pk_step_range's rule.  The view is a pure function of the machine state: the
 * caller evaluates again after whatever replaces a machine (a reset, a load, a resume), and nothing
 * of it travels in bank slots.  Nothing outside the rows and keys of [env0, env0 + count) is written, so
 * disjoint ranges may run concurrently on different streams.  Bad arguments (no view, a range past
 * n, an env0 that is no multiple of 64, count 0) are a negative code with pk_last_error, never a
 * fault, and write nothing. */
#define PK_TILES_ID 0u
#define PK_TILES_HASH 1u
#define PK_TILES_OBJ 1u           /* pk_tiles_create flag: plane 1, the objects */
int pk_tiles_create(pk_handle* h, uint32_t mode, uint32_t bits, uint32_t flags);
uint32_t pk_tiles_planes(const pk_handle* h);         /* 0 without a view */
uint16_t* pk_tiles_ptr(pk_handle* h);                 /* device pointer, owned by the handle; NULL without */
int pk_tiles_eval(pk_handle* h, const uint8_t* mask_dev, const uint64_t* salt_dev, uint64_t* keys_dev,
                  uint32_t env0, uint32_t count, void* stream);

/* Emulated instructions executed by the last pk_step, summed over envs (synchronous). */
int pk_last_instr_count(pk_handle* h, uint64_t* out);

/* The K1 launch shape pk_step_range(h, env0, count, ...) takes (host-side, no GPU work):
 * out[0] = 1 for the small-LDS kernel, out[1] = envs per wave, out[2] = threads per workgroup,
 * out[3] = 1 for the wave-priority variant, out[4] = 1 for the every-bank-staged (ALL) instance.
 * Lets parity tests assert that they run the benchmarked launch. */
int pk_launch_shape(pk_handle* h, uint32_t env0, uint32_t count, uint32_t* out5);

/* Kernel timing with HIP events recorded on the step's stream around K1 (emulate), K2 (render)
 * and K4+K3 (reward + obs) of every pk_step while enabled.  pk_profile_read synchronises,
 * returns the summed milliseconds and the number of profiled steps since the last read, and
 * resets the sums. */
int pk_profile_enable(pk_handle* h, int on);
int pk_profile_read(pk_handle* h, double* emulate_ms, double* render_ms, double* reward_ms, uint64_t* steps);

#ifdef __cplusplus
}
#endif
#endif
