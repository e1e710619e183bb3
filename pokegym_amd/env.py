"""Gymnasium- and PufferLib-shaped surfaces over the batched MI355X env.step.

`Environment` is the drop-in for pokegym.environment.Environment (environment.py:436-1812): same
constructor arguments, reset(seed, options, max_episode_steps, reward_scale) -> (obs, info),
step(action) -> (obs, reward, terminated, truncated, info), close(); observation (72, 80, 4) u8,
Discrete(8) actions.  Where the reference raises inside step/reset, the same exception type is
raised here (the device reports it per env, include/pokegym_amd.h PK_ERR_*).

`VecEnv` is the PufferLib-style batch of N envs on ONE GPU (the intended way to use the device):
reset(seed) -> (obs, infos); step(actions) -> (obs, rewards, terminals, truncations, infos);
async_reset/send/recv; single_observation_space, single_action_space, num_envs.  Finished envs
are reset inside step (their returned obs is the first obs of the next episode), stream-ordered
with no host synchronisation; episode statistics are accumulated on the device and all-reduced
across ranks every `log_interval` steps (pokegym_amd.dist; with sub-batches the record is read one
env-step after the interval, from per-stream snapshots, so the pipeline never drains).  For several GPUs, run one process
per GPU and build each rank's shard with `make_sharded_vecenv`.
"""
from __future__ import annotations

import io
import os
import random
from pathlib import Path

import numpy as np
import torch
import torch.distributed as dist

from . import spaces
from .dist import EpisodeStats, InfoStats, env_rank, shard_range

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_STATE = os.path.join(HERE, "states", "Bulbasaur.state")  # environment.py:119-120


def _session_path(env_id: int) -> Path:
    """environment.py:130-140: experiments/{running experiment name}/sessions/{env_id}."""
    name = "default_exp_name"
    try:
        with open(os.path.join("experiments", "running_experiment.txt")) as f:
            name = f.read().strip() or name
    except OSError:
        pass
    return Path("experiments") / name / "sessions" / str(env_id)


def _read(path_or_bytes):
    if path_or_bytes is None or isinstance(path_or_bytes, (bytes, bytearray)):
        return path_or_bytes
    with open(path_or_bytes, "rb") as f:
        return f.read()


def _key_args(what: str, key, frame, render: bool, tiles: bool = False):
    """Validate a key choice ("ram", "frame", "frame+ram" or "tiles") and its (bw, bh, levels); what = the
    argument prefix, "archive" or "novelty"; tiles = the env has a tile view."""
    if key not in ("ram", "frame", "frame+ram", "tiles"):
        raise ValueError(f'{what}_key must be "ram", "frame", "frame+ram" or "tiles", not {key!r}')
    if key == "tiles" and not tiles:
        raise ValueError(f'{what}_key="tiles" is the tile view\'s key: the env needs tile_view=')
    try:
        bw, bh, levels = (int(v) for v in frame)
    except (TypeError, ValueError):
        raise ValueError(f"{what}_frame must be (bw, bh, levels)") from None
    if bw not in (8, 16, 32, 40, 80, 160) or bh not in (8, 16, 24, 48, 72, 144) or not 2 <= levels <= 256:
        raise ValueError(f"{what}_frame = (bw, bh, levels): bw a multiple of 8 that divides 160, bh one that "
                         "divides 144, levels in 2..256")
    if key not in ("ram", "tiles") and not render:
        raise ValueError(f'{what}_key="{key}" reads the screen: the emulator needs render=True')
    return key, (bw, bh, levels)


def _seen_cap_log2(max_episode_steps: int) -> int:
    """log2 of the seen-coordinate set's capacity for an episode length (pk_create /
    pk_set_episode_params: one entry per step at most, load factor <= 3/4, at least 1024)."""
    lg = 10
    while (1 << lg) * 3 < (int(max_episode_steps) + 2) * 4:
        lg += 1
    return lg


class SlotLedger:
    """What VecEnv keeps of an episode per bank slot: one column per carried value, device tensors.

    The columns' names are those of what an env carries (VecEnv._carried): "ret" and "length" (float64),
    "start" (int32, the pool slot the episode started from; -1 without a pool) and, only for generic
    episodes with probe_features, "feat" (int32 rows of `features` values).  `valid` mirrors the device's
    "holds an episode" flag.  One row past the last slot is a sink: it takes the writes of the slots
    the device rejects (negative or out of range) and is never valid."""

    WIRE = ("ret", "length", "valid", "start")      # column order of rows(): a wire format between ranks

    def __init__(self, n_slots: int, device, features: int = 0):
        self.sink = n_slots
        self.cols = {"ret": torch.zeros(n_slots + 1, dtype=torch.float64, device=device),
                     "length": torch.zeros(n_slots + 1, dtype=torch.float64, device=device),
                     "start": torch.full((n_slots + 1,), -1, dtype=torch.int32, device=device)}
        if features:
            self.cols["feat"] = torch.zeros((n_slots + 1, features), dtype=torch.int32, device=device)
        self.valid = torch.zeros(n_slots + 1, dtype=torch.bool, device=device)

    def _rows(self, slots: torch.Tensor) -> torch.Tensor:
        slots = slots.long()
        return torch.where((slots >= 0) & (slots < self.sink), slots, self.sink)

    def store(self, slots: torch.Tensor, values: dict, valid=True):
        """values[name][i] (and valid, or valid[i]) into slot slots[i]; a rejected slot stores nothing."""
        rows = self._rows(slots)
        for name, v in values.items():
            self.cols[name][rows] = v.to(self.cols[name].dtype)
        self.valid[rows] = valid
        self.valid[self.sink] = False

    def fetch(self, slots: torch.Tensor):
        """(ok, values): values[name][i] is slot slots[i]'s, ok[i] whether that slot holds an episode."""
        rows = self._rows(slots)
        return self.valid[rows], {name: col[rows] for name, col in self.cols.items()}

    def invalidate(self, slots: torch.Tensor | None = None):
        """The slots (None: every slot) hold no episode any more."""
        if slots is None:
            self.valid.zero_()
        else:
            self.valid[self._rows(slots)] = False

    def rows(self, slot0: int, count: int) -> torch.Tensor:
        """Slots [slot0, slot0 + count) as float64 (count, 4) rows in WIRE order, as the exchange sends them."""
        sl = slice(slot0, slot0 + count)
        return torch.stack([(self.valid if name == "valid" else self.cols[name])[sl].to(torch.float64)
                            for name in self.WIRE], dim=1)

    def place(self, slots: torch.Tensor, rows: torch.Tensor):
        """rows() rows back into slots[i]; the row of a rejected slot goes nowhere."""
        cols = dict(zip(self.WIRE, rows.unbind(1)))
        self.store(slots, {name: v for name, v in cols.items() if name != "valid"}, cols["valid"] != 0)


class Base:
    """pokegym.environment.Base (environment.py:89-434): the emulator surface without the reward
    stack — step(action) runs the action and returns (render(), 0, False, False, {}) (:404-406),
    reset() returns the current screen without touching the game (:228-230), plus the savestate,
    screenshot and video helpers Environment inherits.  As there, the template state is kept in
    initial_states but not loaded (make_env boots the ROM, :116-122), and render() keeps its own
    visited-tile memory per map (:157-160, :256-272), here on the device."""

    _next_id = 0

    def __init__(self, rom_path="pokemon_red.gb", state_path=None, headless=True, save_video=False, quiet=False,
                 device: int = 0, **kwargs):
        state = _read(state_path if state_path is not None else DEFAULT_STATE)
        self.emu = self._emulator(_read(rom_path), state, device)
        self.observation_space = spaces.observation_space()
        self.action_space = spaces.action_space()
        self.headless = headless
        self.initial_states = [io.BytesIO(state)]   # environment.py:119-122 (the template state)
        self.pokemon_center_save_states = []
        # video / screenshots (environment.py:123, :128, :140, :200-206, :1244-1249, :1340, :1616)
        self.save_video = save_video
        self.screenshot_counter = 0
        self.reset_count = 0
        self.env_id = Base._next_id
        Base._next_id += 1
        self.s_path = Path(kwargs["s_path"]) if "s_path" in kwargs else _session_path(self.env_id)
        self._recorder = None
        if save_video:
            from .video import FrameRecorder
            self._recorder = FrameRecorder(self.emu, [0])
        self.screen_memory = {}     # map -> (255, 255) u8 device tensor (environment.py:157-160)

    def _emulator(self, rom, state, device):
        # the ROM boots; the template state only goes into initial_states (environment.py:116-122)
        from .emulator import BatchedEmulator
        return BatchedEmulator(rom, 1, state=None, device=device, render=True)

    def video(self):
        """environment.py:408-410: the current (144, 160, 3) screen."""
        from .video import to_rgb
        return to_rgb(self.emu.screen[0].cpu().numpy())

    def add_video_frame(self):
        """environment.py:621-622 (the frame stays on the device until the episode is written)."""
        self._recorder.capture()

    def save_screenshot(self, event, map_n):
        """environment.py:200-206: screenshots/{counter}_{event}_{map_n}.jpeg."""
        from .video import save_screenshot
        self.screenshot_counter += 1
        return save_screenshot(self.emu.screen[0].cpu().numpy(), event, map_n, self.screenshot_counter)

    # -- savestates (environment.py:208-227): PyBoy v9 images of the device state --------------
    def save_state(self):
        """environment.py:208-213: append the current machine state (v9 savestate) to
        pokemon_center_save_states."""
        self.pokemon_center_save_states.append(io.BytesIO(self.emu.snapshot(0)))

    def load_pokemon_center_state(self):
        return self.pokemon_center_save_states[len(self.pokemon_center_save_states) - 1]

    def load_last_state(self):
        return self.initial_states[len(self.initial_states) - 1]

    def load_first_state(self):
        return self.initial_states[0]

    def load_random_state(self):
        return self.initial_states[random.randint(0, len(self.initial_states) - 1)]

    def load_pyboy_state(self, state):
        """pyboy_binding.py:59-69 load_pyboy_state: install a v9 savestate (bytes or file object)."""
        data = state.getvalue() if hasattr(state, "getvalue") else bytes(state)
        self.emu.load_env(0, data)

    def reset(self, seed=None, options=None):
        """environment.py:228-230: the current screen, the game untouched (seeding is not supported)."""
        return self.video(), {}

    def step(self, action):
        """environment.py:404-406: run the action (the same press / release schedule as
        Environment.step, pyboy_binding.py:71-91), then (render(), 0, False, False, {})."""
        a = torch.tensor([int(action)], dtype=torch.uint8, device=self.emu.device)
        self.emu.step(a)
        return self.render(), 0, False, False, {}

    def render(self):
        """environment.py:256-272 (+ get_fixed_window :233-254): mark the player's tile in this
        map's memory, then the screen at half resolution (3 channels) beside the (72, 80) window of
        that memory centred on the player, zero-padded past the 255 x 255 edge."""
        pos = self.emu.peek(0, 0xD35E, 5)               # ram_map.position: D35E map, D361 y, D362 x
        r, c, m = pos[3], pos[4], min(pos[0], 247)
        mm = self.screen_memory.get(m)
        if mm is None:
            mm = self.screen_memory[m] = torch.zeros((255, 255), dtype=torch.uint8, device=self.emu.device)
        if r <= 254 and c <= 254:
            mm[r, c] = 255
        win = torch.zeros((72, 80), dtype=torch.uint8, device=self.emu.device)
        y0, y1, x0, x1 = max(0, r - 36), min(255, r + 36), max(0, c - 40), min(255, c + 40)
        if y0 < y1 and x0 < x1:
            win[y0 - r + 36:y1 - r + 36, x0 - c + 40:x1 - c + 40] = mm[y0:y1, x0:x1]
        half = self.emu.screen[0, ::2, ::2]
        return torch.stack((half, half, half, win), dim=2).cpu().numpy()

    def close(self):
        self.emu.close()


class Environment(Base):
    """One env (a single emulator lane) with pokegym's reward stack (environment.py:436-1812).
    Functionally the reference env; for throughput use VecEnv, which steps thousands of envs per
    kernel launch."""

    def __init__(self, rom_path="pokemon_red.gb", state_path=None, headless=True, save_video=False, quiet=False,
                 verbose=False, device: int = 0, max_episode_steps: int = 20480, reward_scale: float = 4.0, **kwargs):
        self.max_episode_steps, self.reward_scale = max_episode_steps, reward_scale
        self._default_episode = (int(max_episode_steps), float(reward_scale))   # reset()'s defaults
        super().__init__(rom_path, state_path, headless, save_video, quiet, device=device, **kwargs)
        self.screen_memory = None   # the reward stack's observation keeps it on the device (K3)

    def _emulator(self, rom, state, device):
        from .emulator import BatchedEmulator
        return BatchedEmulator(rom, 1, state=state, device=device, render=True, reward=True,
                               max_episode_steps=self.max_episode_steps, reward_scale=self.reward_scale, heatmap=True)

    def reset(self, seed=None, options=None, max_episode_steps=None, reward_scale=None):
        """environment.py:1233-1334 (seeding is not supported, as in the reference).  As there, every
        reset sets max_episode_steps / reward_scale from its arguments (:1258-1259): an argument left
        out takes its default — the constructor's value, 20480 / 4.0 unless given (the reference's
        reset defaults) — so one reset(max_episode_steps=X) does not stick to later resets."""
        mes = self._default_episode[0] if max_episode_steps is None else int(max_episode_steps)
        rsc = self._default_episode[1] if reward_scale is None else float(reward_scale)
        if (mes, rsc) != (self.max_episode_steps, self.reward_scale):
            self.emu.set_episode_params(mes, rsc)
            self.max_episode_steps, self.reward_scale = mes, rsc
        obs = self.emu.reset()
        self.emu.raise_if_failed(0)
        if self.save_video:   # a new episode file: {s_path}/reset_{k} (environment.py:1244-1249)
            self._recorder.clear()
            self._video_file = self.s_path / f"reset_{self.reset_count}"
        self.reset_count += 1
        return obs[0].cpu().numpy(), {}

    def step(self, action, fast_video=True):
        """environment.py:1336-1812; info is {} except at done / every 10000th step (:1621), where it
        holds the numeric scalars of the reference's "stats" and "reward" dicts (pokegym_amd/info.py)."""
        a = torch.tensor([int(action)], dtype=torch.uint8, device=self.emu.device)
        obs, rew, term, trunc = self.emu.step(a)
        if self.save_video:
            self.add_video_frame()
        self.emu.raise_if_failed(0)
        done = bool(term[0].item())
        if self.save_video and done:    # environment.py:1616-1617: the episode's video is closed
            self.last_video = self._recorder.write(self._video_file)
            self._recorder.clear()
        info = self.emu.info_dicts([0]).get(0, {})
        if info:   # "pokemon_exploration_map": self.counts_map (float64 in the reference)
            info["pokemon_exploration_map"] = self.emu.heatmap[0].cpu().numpy().astype(np.float64)
            info["stats"]["pokemon_exploration_map"] = info["pokemon_exploration_map"]
        return obs[0].cpu().numpy(), float(rew[0].item()), done, done, info

    def render(self):
        """Base.render's observation as the reward stack's K3 built it for the last step / reset."""
        return self.emu.obs[0].cpu().numpy()


class VecEnv:
    """N envs on one GPU with PufferLib-style batch semantics (device tensors in and out).

    batch_size < num_envs splits the envs into num_envs / batch_size sub-batches (the reference
    trains 72 envs 24 at a time, README.md:116-118): recv() returns the next sub-batch whose step
    has finished, send(actions) steps the sub-batch the last recv() returned on its own HIP stream
    (pk_step_range) and returns immediately, so the policy works on one sub-batch while the GPU
    steps the others.  batch_size must divide num_envs; a sub-batch starts on a 64-env image group
    (pk_step_range), so a batch_size that is not a multiple of 64 (the reference's 24) is laid out
    in 64-aligned slots whose padding envs are never stepped.  step(actions) steps all envs at once.
    Sub-batches overlap on the GPU while the HIP runtime has a hardware queue per stream
    (GPU_MAX_HW_QUEUES, 4 by default: the default stream plus up to 3 sub-batches; beyond that
    streams share queues and their launches serialise)."""

    def __init__(self, num_envs: int, rom_path=None, state_path=None, rom: bytes | None = None, state: bytes | None = None,
                 device: int | None = None, max_episode_steps: int = 20480, reward_scale: float = 4.0,
                 reload_on_reset: bool = False, env_offset: int = 0, log_interval: int = 128, emulator=None,
                 heatmap: bool = False, reward: bool = True, power_on: bool = False, batch_size: int | None = None,
                 state_pool=None, pool_seed: int = 0, bank_slots: int = 0, bank_episodes: bool | str = False,
                 fork_slots: int = 0, archive_cells: int = 0, archive_seed: int = 0, archive_shift: int = 0,
                 record_trajectories: bool = False, archive_exchange: bool = False, archive_key: str = "ram",
                 archive_frame=(16, 16, 8), novelty_log2: int = 0, novelty_beta: float = 1.0, novelty_key: str = "frame",
                 novelty_frame=(16, 16, 8), frame_stack: int = 0, stack_scale: int = 2, stack_layout: str = "chw",
                 stack_mode: str = "mean", probes=None, probe_features: bool = False, tile_view: str | None = None,
                 tile_bits: int = 12, tile_objects: bool = True):
        """reward=False: the screen-obs env of configs[3] — obs is the (144, 160) u8 screen; without
        probes= or novelty_log2= the rewards are 0 and episodes end at max_episode_steps.
        power_on=True starts (and resets) every env from the cartridge's power-on state instead of
        a savestate.

        state_pool (a list of v9 savestates, bytes or paths) puts the states into a device savestate
        bank; every reset, the auto-resets included, then starts each env from a slot drawn on the
        device (a torch.Generator seeded with pool_seed) — the reference's get_random_state /
        load_random_state (environment.py:51, :116, :219-227) for a whole batch.  `start_slots` is
        the slot every env last started from.  bank_slots adds that many free slots after the
        pool's, for save_to_bank / load_from_bank.  With neither, no bank exists and every call is
        the one made without this feature.

        bank_episodes=True (needs reward=True) lets the slots carry whole episodes: checkpoint_to_bank
        / resume_from_bank move the machine state together with the episode's step counter and
        reward bookkeeping, so a resumed env continues exactly as the saved one would have, and
        this class's per-env episode return / length and start slot travel with it.  fork_slots
        reserves that many scratch slots after the pool's and the user's for fork(): the number of
        distinct source envs one fork() call can copy.

        bank_episodes="generic" (needs reward=False) is the same on any cartridge: the slots carry generic
        episode parts (pk_bank_enable_generic_episodes) — the raw lane registers with the step counter,
        and whatever of probes= and frame_stack= the env has, the probe state words and the stack rows —
        so checkpoint_to_bank, resume_from_bank, fork, fork_slots, archive_cells (archive_key="frame";
        "ram" and "frame+ram" stay legal but read Pokémon Red's addresses) and record_trajectories work
        as for reward envs, with the frame key and the probe return.  A resumed env keeps the
        checkpoint's frames and probe state: resume_from_bank, fork and archive_explore neither refill
        nor rebase, a resumed "newmax" keeps its maximum, and with probe_features the feature rows
        travel per slot like the episode return, so probe_values shows the checkpoint's values.
        archive_exchange=True raises: the exchange payload has no format for generic parts.

        archive_cells=K (needs bank_episodes=True) adds K more slots after those and an exploration
        archive over them (pk_archive_*): archive_update() keeps the best episode per cell key,
        archive_explore(mask) resumes envs from cells drawn by visit count with archive_seed;
        archive_shift is cell_keys()'s coordinate shift.  archive_key chooses what a cell is: "ram" (the
        default) is pk_cell_keys' map | x | y | badges of Pokémon Red's WRAM; "frame" is Go-Explore's
        downscaled frame (pk_frame_keys), which any cartridge has and which tells a menu, a battle or a
        dialogue from the map under it; "frame+ram" is both, the RAM key mixed into the frame key as its
        salt.  archive_frame = (bw, bh, levels) is the frame cell's block size and level count;
        frame_cells() returns the cell image itself.  Both are calls of the training loop between
        steps: the auto-reset path does not explore, and the archive is not driven per sub-batch
        on the sub-batch streams.  archive_exchange=True (needs archive_cells) lets the archive leave
        the handle: archive_export() / archive_import() move its cells — records, whole slots and this
        class's per-slot episode return / length / start slot — as host arrays, and archive_sync()
        exchanges what the archives of a torch.distributed group learned since the last call.

        record_trajectories=True records every env's actions since its last reset on the device
        (pk_traj_enable): trajectory(env), and with bank_episodes slot_trajectory(slot) and
        archive_trajectory(cell), return the action list that reaches a state and the slot it starts
        from — a demonstration, and with BatchedEmulator.replay() the way to rebuild a slot or a
        whole archive after a restart.  Checkpoints, resumes, forks and the archive carry the lists
        along.  Without it nothing is allocated or launched.

        novelty_log2=L (10..30; 0 = off) adds a count-based exploration bonus on any cartridge, with or
        without the reward stack: a device table of 2**L entries (pk_counts_*) counts the key of the
        frame every step ends on — the last frame of an episode counts, the frame an auto-reset
        restarts from never does — and the returned rewards are the extrinsic reward plus
        novelty_beta / sqrt(visits of the key, this one included); with reward=False they are the bonus
        alone.  The episode statistics keep the extrinsic return.  novelty_key and novelty_frame
        choose the key as archive_key and archive_frame do (the "ram" key uses archive_shift).  Each
        sub-batch takes its keys on its own stream right after its step; the table, one shared
        structure, is updated where calls are in one order: inside step() in batch order, and in the
        recv() that returns a sub-batch.  novelty_keys / novelty_counts / novelty_bonus are the last
        values per env; counts_sync() adds up the tables of a torch.distributed group.

        frame_stack=D (1..8; 0 = off; needs a rendering emulator) makes the observation a frame stack kept
        on the device (pk_fstack_*): the last D frames of every env, newest first, downscaled by
        stack_scale (1, 2, 4; stack_mode "mean" averages a block, "pick" takes its top left pixel, the
        reference's [::2, ::2]) — uint8 (D, 144 / s, 160 / s) for stack_layout "chw", (144 / s, 160 / s, D)
        for "hwc" (D = 1, 2, 4, 8; D = 4 at scale 2 is the reference observation's shape) — with or
        without the reward stack, on any cartridge.  reset(), step(), recv() and async_reset() return it
        in the place of the composite observation or the screen.  Each sub-batch pushes the frame its
        step ended on, on its own stream and in one launch; an env that finished returns D copies of
        the first frame of its next episode.  reset() fills every env, and load_from_bank,
        resume_from_bank, fork, archive_explore and load_state refill the envs whose machine they
        replaced (load_from_bank: every env it names with a slot of the bank).  With 0 nothing is
        allocated or launched.

        probes=program (a list of probes.Probe records, e.g. probes.pkbench_program(); None = off) reads a
        reward and a termination condition from every env's RAM (pk_probe_*), on any cartridge: with
        reward=False they are the env's reward and the only way an episode ends before
        max_episode_steps, with reward=True they are added on top of the reward stack's.  Right after
        each sub-batch's step, on its stream, one launch adds the program's reward into the emulator's
        reward array and ORs its done flag into the terminal array, so the returned rewards and
        terminals, the episode statistics and the auto-reset all see them; a second launch after the
        auto-reset rebases the envs that were reset, so their next step is measured from the reset
        state.  reset() rebases every env, and load_from_bank, resume_from_bank, fork, archive_explore
        and load_state rebase the envs whose machine they replaced, at the sites and with the masks of
        the frame stack's refill: without bank_episodes="generic" the probe state does not travel through
        the bank, a resumed "newmax" starts again from the current value.  probe_features=True also keeps the probe values:
        probe_values is int32 (num_envs, m), the values every env's last step ended on (probe_space).
        With None nothing is allocated or launched.

        tile_view="id" or "hash" (None = off) keeps the symbolic observation of every env on the device
        (pk_tiles_*): the screen as 18 x 20 background / window tile ids and, with tile_objects, a second
        plane of object tiles — or, with "hash", tile_bits-bit (8..15) hashes of the tiles' data, which
        survive a game's reloading of tile data — int16 (P, 18, 20), -1 = nothing (tile_space).  It is
        computed from the registers, VRAM and OAM a step leaves, never from pixels, so it works with a
        headless emulator (render=False), and it is not the pixels where a game writes scroll or LCDC
        mid-frame.  tile_obs() returns it.  Each sub-batch evaluates once per step, on its own stream and
        in one launch, after the auto-reset (a finished env shows the first state of its next episode);
        reset(), load_from_bank, resume_from_bank, fork, archive_explore and load_state evaluate the
        envs whose machine they replaced.  archive_key="tiles" and novelty_key="tiles" use the view's
        64-bit key: two envs are in one cell exactly when their views are equal.  With None nothing is
        allocated or launched."""
        self.batch_size = batch_size or num_envs
        self.num_batches, rest = divmod(num_envs, self.batch_size)
        if rest:
            raise ValueError("batch_size must divide num_envs")
        # slot of a sub-batch in the emulator: batch_size rounded up to a 64-env group
        self.slot = (self.batch_size if self.num_batches == 1 or self.batch_size % 64 == 0
                     else -(-self.batch_size // 64) * 64)
        n_phys = self.num_batches * self.slot
        if emulator is None:
            from .emulator import BatchedEmulator
            rom = rom if rom is not None else _read(rom_path or "pokemon_red.gb")
            if power_on:
                state = None
            else:
                state = state if state is not None else _read(state_path if state_path is not None else DEFAULT_STATE)
            emulator = BatchedEmulator(rom, n_phys, state=state, device=0 if device is None else device, render=True,
                                       reward=reward, max_episode_steps=max_episode_steps, reward_scale=reward_scale,
                                       reload_on_reset=reload_on_reset, heatmap=heatmap)
        if getattr(emulator, "n", n_phys) != n_phys:
            raise ValueError(f"the emulator must hold {n_phys} envs ({self.num_batches} sub-batch slots of {self.slot})")
        self.emu = emulator
        self.device = emulator.device
        self.num_envs = self.num_agents = num_envs
        # emulator index of every env (only differs from the env index when slots are padded)
        self._padded = n_phys != num_envs
        self._phys = self.phys(torch.arange(num_envs)).to(self.device) if self._padded else None
        self.single_observation_space = (spaces.observation_space() if getattr(emulator, "reward", True)
                                         else spaces.screen_space())
        self.frame_stack = 0 if frame_stack is None else frame_stack
        self.stack_scale, self.stack_layout, self.stack_mode = stack_scale, stack_layout, stack_mode
        if self.frame_stack != 0:
            self.single_observation_space = spaces.stack_space(stack_scale, frame_stack, stack_layout)
            if stack_mode not in ("mean", "pick"):
                raise ValueError("stack_mode must be 'mean' or 'pick'")
            if not getattr(emulator, "render", True):
                raise ValueError("frame_stack needs an emulator that renders (render=True)")
            self.emu.stack_create(stack_scale, frame_stack, stack_layout, stack_mode)
        # RAM probes (pk_probe_*): nothing is allocated or called with probes=None
        self.probes = None if probes is None else list(probes)
        self._probe_feat = None
        self.probe_space = None
        if self.probes is None:
            if probe_features:
                raise ValueError("probe_features=True needs probes=")
        else:
            self.emu.probes_create(self.probes)
            self.probe_space = spaces.probe_space(len(self.probes))
            if probe_features:
                self._probe_feat = torch.zeros((n_phys, len(self.probes)), dtype=torch.int32, device=self.device)
        # tile view (pk_tiles_*): nothing is allocated or called with tile_view=None
        self.tile_view = tile_view
        self.tile_space = None
        if tile_view is not None:
            if tile_view not in ("id", "hash"):
                raise ValueError(f'tile_view must be "id", "hash" or None, not {tile_view!r}')
            if tile_view == "hash" and not 8 <= int(tile_bits) <= 15:
                raise ValueError("tile_bits must be 8..15")
            self.emu.tiles_create(tile_view, tile_bits, bool(tile_objects))
            self.tile_space = spaces.tile_space(self.emu.tile_planes)
        self.single_action_space = spaces.action_space()
        self.env_ids = torch.arange(env_offset, env_offset + num_envs, device=self.device)
        self.masks = torch.ones(num_envs, dtype=torch.bool, device=self.device)
        self.stats = EpisodeStats(num_envs, self.device, self.num_batches)
        self.info_stats = (InfoStats(self.device, self.num_batches) if getattr(emulator, "info", None) is not None
                           else None)
        self.log_interval = log_interval
        self.t = 0
        self._pending = None
        # first PK_ERR_* code of every env since the last check: the device clears an env's error
        # word when the env auto-resets, so the codes are kept here (no host sync) and raised at
        # the next logging interval — an exception between two checks is not lost
        errs = getattr(emulator, "errors", None)
        self.sticky_errors = torch.zeros_like(errs) if errs is not None else None
        # sub-batch pipeline (batch_size < num_envs): one stream + completion event per sub-batch,
        # FIFO of finished ones
        self._streams = [torch.cuda.Stream(self.device) for _ in range(self.num_batches)] if self.num_batches > 1 else []
        self._events = [torch.cuda.Event() for _ in range(self.num_batches)] if self.num_batches > 1 else []
        self._ready: list[int] = []
        self._current: int | None = None
        self._batch_steps = 0
        self.logs_fired = 0        # logging intervals that fired (error check + all-reduce issued)
        # deferred interval read (sub-batch pipeline): the interval's rows and error codes are
        # snapshotted on each sub-batch stream where it fires, and read by the host num_batches
        # recv()s later, when the last of those streams' steps is the one being received
        self._log_wait = 0
        self._snap_events = [torch.cuda.Event() for _ in range(self.num_batches)] if self.num_batches > 1 else []
        self._snap_err = torch.zeros_like(self.sticky_errors) if self.sticky_errors is not None else None
        # savestate bank: the pool's states in slots [0, pool_size), bank_slots free ones after them
        self.pool_size = 0
        self._slots = self._pool_gen = None
        self.record_trajectories = bool(record_trajectories)
        if self.record_trajectories:
            self.emu.traj_enable()
        self.fork_slots = int(fork_slots)
        self._cap_lg = _seen_cap_log2(getattr(emulator, "max_episode_steps", 20480))
        self._fork0 = 0             # first scratch slot of fork()
        self._ledger = None         # SlotLedger with bank_episodes
        self._generic = isinstance(bank_episodes, str)
        if self._generic:
            if bank_episodes != "generic":
                raise ValueError(f'bank_episodes must be True, False or "generic", not {bank_episodes!r}')
            if getattr(emulator, "reward", False):
                raise ValueError('bank_episodes="generic" is for emulators without the reward stack (reward=False)')
            if archive_exchange:
                raise ValueError('archive_exchange needs bank_episodes=True: generic episode parts have no exchange payload')
        elif bank_episodes and not getattr(emulator, "reward", False):
            raise ValueError("bank_episodes=True needs the reward stack (reward=True)")
        if self.fork_slots and not bank_episodes:
            raise ValueError("fork_slots needs bank_episodes=True")
        self.archive_cells, self.archive_shift = int(archive_cells), int(archive_shift)
        self.archive_key, self.archive_frame = _key_args("archive", archive_key, archive_frame,
                                                         getattr(emulator, "render", True), tile_view is not None)
        # count-based novelty bonus (pk_counts_*): nothing is allocated or called with novelty_log2 = 0
        self.novelty_log2, self.novelty_beta = int(novelty_log2), float(novelty_beta)
        self.novelty_key, self.novelty_frame = _key_args("novelty", novelty_key, novelty_frame,
                                                         not self.novelty_log2 or getattr(emulator, "render", True),
                                                         tile_view is not None)
        self._nov_keys = self._nov_counts = self._nov_bonus = None
        # per sub-batch of the pipeline: 0 = nothing owed, 1 = sent, its keys not counted yet (recv()
        # counts them), 2 = counted by a flush, recv() still owes its bonus to the returned rewards
        self._nov_due = [0] * self.num_batches
        if self.novelty_log2:
            self.emu.counts_create(self.novelty_log2)
            # emulator order; padding envs keep key -1 ("no key") and never count
            self._nov_keys = torch.full((n_phys,), -1, dtype=torch.int64, device=self.device)
            self._nov_counts = torch.zeros(n_phys, dtype=torch.int64, device=self.device)
            self._nov_bonus = torch.zeros(n_phys, dtype=torch.float64, device=self.device)
        self._arch0 = 0             # first slot of the archive's cells
        self._arch_out = None
        self.archive_exchange = bool(archive_exchange)
        if self.archive_cells and not bank_episodes:
            raise ValueError("archive_cells needs bank_episodes=True")
        if self.archive_exchange and not self.archive_cells:
            raise ValueError("archive_exchange needs archive_cells")
        if state_pool is not None or bank_slots or self.fork_slots or self.archive_cells:
            pool = [st if isinstance(st, (bytes, bytearray)) else _read(st) for st in (state_pool or [])]
            if state_pool is not None and not pool:
                raise ValueError("state_pool is empty")
            self._fork0 = len(pool) + int(bank_slots)
            self._arch0 = self._fork0 + self.fork_slots
            self.emu.bank_create(self._arch0 + self.archive_cells)
            for k, st in enumerate(pool):
                self.emu.bank_put(k, st)
            self.pool_size = len(pool)
            if pool:
                self._pool_gen = torch.Generator(device=self.device)
                self._pool_gen.manual_seed(int(pool_seed))
                # slot each emulator env last started from; padding envs keep -1 (the template)
                self._slots = torch.full((n_phys,), -1, dtype=torch.int32, device=self.device)
            if bank_episodes:
                # what this class keeps per env of an episode, per slot: taken at a checkpoint,
                # restored at a resume (device tensors, no host copy)
                if self._generic:   # the parts of what this env has; both were created above
                    self.emu.bank_enable_generic_episodes(probes=self.probes is not None, stack=bool(self.frame_stack))
                else:
                    self.emu.bank_enable_episodes()
                # (generic episodes with probe_features: the feature row travels per slot too)
                self._ledger = SlotLedger(self._arch0 + self.archive_cells, self.device,
                                          len(self.probes) if self._generic and self._probe_feat is not None else 0)
                if self.archive_cells:
                    self.emu.archive_create(self._arch0, self.archive_cells, archive_seed)
                    self._arch_out = torch.full((n_phys,), -1, dtype=torch.int32, device=self.device)
                    if self.archive_exchange:
                        self.emu.archive_exchange_enable()
        elif bank_episodes:
            raise ValueError("bank_episodes=True needs a bank: state_pool, bank_slots or fork_slots")

    def _draw_slots(self, psl: slice, done: torch.Tensor | None = None):
        """Draw a pool slot for the envs of emulator range psl (those with done[e] != 0) on the
        current stream; the others keep the slot they started from."""
        draw = torch.randint(0, self.pool_size, (psl.stop - psl.start,), generator=self._pool_gen,
                             device=self.device, dtype=torch.int32)
        cur = self._slots[psl]
        if done is None:
            cur.copy_(draw)
        else:
            torch.where(done != 0, draw, cur, out=cur)

    @property
    def start_slots(self) -> torch.Tensor:
        """Pool slot every env last started an episode from (int32, env order)."""
        if self._slots is None:
            raise RuntimeError("VecEnv(state_pool=...) draws start slots")
        return self._logical(self._slots).clone()

    def _bank_map(self, envs, slots) -> torch.Tensor:
        """Full-size slot_of_env (emulator order) naming slots[i] for env envs[i], -1 elsewhere."""
        if not self.emu.bank_slots:
            raise RuntimeError("VecEnv(state_pool=... or bank_slots=...) makes the bank")
        envs = torch.as_tensor(envs, device=self.device).reshape(-1).long()
        slots = torch.as_tensor(slots, device=self.device).reshape(-1).to(torch.int32)
        if envs.numel() != slots.numel():
            raise ValueError("envs and slots must have the same length")
        out = torch.full((self.emu.n,), -1, dtype=torch.int32, device=self.device)
        out[self.phys(envs)] = slots
        return out

    def save_to_bank(self, envs, slots, check: bool = True):
        """Save env envs[i] into bank slot slots[i] (host lists or device tensors, env indices as
        everywhere in this class) on the current stream, after it has joined the sub-batch streams:
        a pipeline join — steps in flight finish first — not a host sync.  check=True rejects a
        slot named twice (the slot would hold a mixture), which reads the slots back and so does
        sync the host; pass check=False inside a training loop."""
        if check:
            s = torch.as_tensor(slots).reshape(-1)
            if torch.unique(s).numel() != s.numel():
                raise ValueError("save_to_bank: a slot is named twice")
        self._join_streams()
        self.emu.bank_save(self._bank_map(envs, slots))
        if self._ledger is not None:        # a plain save leaves the slot without an episode
            self._ledger.invalidate(torch.as_tensor(slots, device=self.device).reshape(-1))

    def load_from_bank(self, envs, slots):
        """Load bank slot slots[i] into env envs[i] (pk_bank_load: machine state only, the episode's
        step counter and reward bookkeeping survive) on the current stream, after a pipeline join
        like save_to_bank's.  An empty or out-of-range slot leaves its env alone and counts in
        emu.bank_rejects()."""
        self._join_streams()
        m = self._bank_map(envs, slots)
        self.emu.bank_load(m)
        if self.frame_stack or self.probes is not None or self.tile_view:
            self._machines_replaced(((m >= 0) & (m < self.emu.bank_slots)).to(torch.uint8))

    def _machines_replaced(self, mask: torch.Tensor, carried: bool = False):
        """The envs with mask[e] != 0 (uint8, emulator order) run another machine from here on: their
        frame stacks start over and their probes are rebased (not with carried: generic episode parts
        brought both along), and their tile views are evaluated again, on the current stream."""
        if self.frame_stack and not carried:
            self.emu.stack_push(mask, fill_only=True)
        if self.probes is not None and not carried:
            self.emu.probes_eval(mask, rebase_only=True, features=self._probe_feat)
        if self.tile_view:
            self.emu.tiles_eval(mask)

    def _carried(self) -> dict:
        """Everything of an episode that this class keeps per env and that travels through a bank slot:
        SlotLedger column -> (tensor, whether it is in emulator order); the others are in env order."""
        c = {"ret": (self.stats.ep_return, False), "length": (self.stats.ep_length, False)}
        if self._slots is not None:
            c["start"] = (self._slots, True)
        if "feat" in self._ledger.cols:
            c["feat"] = (self._probe_feat, True)
        return c

    def _gather(self, envs: torch.Tensor | None = None) -> dict:
        """What the envs (None: every env, in env order) carry, for SlotLedger.store."""
        if envs is None:
            return {name: self._logical(t) if emu_order else t for name, (t, emu_order) in self._carried().items()}
        return {name: t[self.phys(envs) if emu_order else envs] for name, (t, emu_order) in self._carried().items()}

    def _scatter(self, values: dict, ok: torch.Tensor, envs: torch.Tensor | None = None):
        """The reverse: envs[i] (None: env i) takes values[name][i] where ok[i]; the others keep theirs."""
        for name, (t, emu_order) in self._carried().items():
            take = ok if t.dim() == 1 else ok[:, None]
            if envs is not None:
                idx = self.phys(envs) if emu_order else envs
                t[idx] = torch.where(take, values[name], t[idx])
            elif emu_order:
                self._set_physical(t, torch.where(take, values[name], self._logical(t)))
            else:
                t.copy_(torch.where(take, values[name], t))

    def _episode_args(self, envs, slots):
        self._require("episodes")
        envs = torch.as_tensor(envs, device=self.device).reshape(-1).long()
        slots = torch.as_tensor(slots, device=self.device).reshape(-1).long()
        if envs.numel() != slots.numel():
            raise ValueError("envs and slots must have the same length")
        return envs, slots

    def checkpoint_to_bank(self, envs, slots, check: bool = True):
        """Checkpoint the episode of env envs[i] into bank slot slots[i] (pk_bank_checkpoint): the
        machine state as save_to_bank stores it, the episode's step counter and reward bookkeeping,
        and this class's episode return / length and start slot of the env.  On the current stream
        after a pipeline join, like save_to_bank; check=True rejects a slot named twice (host sync)."""
        envs, slots = self._episode_args(envs, slots)
        if check and torch.unique(slots).numel() != slots.numel():
            raise ValueError("checkpoint_to_bank: a slot is named twice")
        self._join_streams()
        self.emu.bank_checkpoint(self._bank_map(envs, slots))
        self._ledger.store(slots, self._gather(envs))

    def resume_from_bank(self, envs, slots):
        """Env envs[i] continues the episode checkpointed in slot slots[i] (pk_bank_resume): fed the
        same actions it returns what the checkpointed env returned, its observation row shows the
        resumed state at once, and its episode return / length and start slot are the checkpoint's.
        Many envs may name one slot.  On the current stream after a pipeline join.  A slot that is
        empty, out of range or holds no episode (save_to_bank, the pool) leaves its env alone and
        counts in emu.bank_rejects(); sticky_errors stay with the env."""
        envs, slots = self._episode_args(envs, slots)
        self._join_streams()
        self.emu.bank_resume(self._bank_map(envs, slots))
        ok, values = self._ledger.fetch(slots)      # ok: the envs the device does not reject
        self._scatter(values, ok, envs)
        # generic: stack rows and probe words came with the slot (and the feature rows with the ledger:
        # an evaluation would pay reward), so no refill and no rebase; else the resumed envs start a
        # history of their own
        if self.tile_view or (not self._generic and (self.frame_stack or self.probes is not None)):
            m = torch.zeros(self.emu.n, dtype=torch.uint8, device=self.device)
            m[self.phys(envs)] = ok.to(torch.uint8)
            self._machines_replaced(m, carried=self._generic)

    def fork(self, dst_envs, src_envs, check: bool = True):
        """Copy the running episode of env src_envs[i] over env dst_envs[i]: every distinct source
        is checkpointed into one of the fork_slots scratch slots and the destinations resume from
        those, on the current stream after a pipeline join.  The arguments are host lists (or
        tensors, read back).  A destination named twice, or more distinct sources than fork_slots,
        raises; check=True also rejects a destination that is a source of the same call."""
        dst = [int(e) for e in torch.as_tensor(dst_envs).reshape(-1).tolist()]
        src = [int(e) for e in torch.as_tensor(src_envs).reshape(-1).tolist()]
        self._require("fork")
        if len(dst) != len(src):
            raise ValueError("fork: dst_envs and src_envs must have the same length")
        if any(not 0 <= e < self.num_envs for e in dst + src):
            raise ValueError("fork: env index out of range")
        if len(set(dst)) != len(dst):
            raise ValueError("fork: a destination is named twice")
        if check and set(dst) & set(src):
            raise ValueError("fork: a destination is also a source")
        uniq = sorted(set(src))
        if len(uniq) > self.fork_slots:
            raise ValueError(f"fork: {len(uniq)} distinct sources, {self.fork_slots} scratch slots (fork_slots)")
        if not dst:
            return
        slot_of = {e: self._fork0 + k for k, e in enumerate(uniq)}
        self.checkpoint_to_bank(uniq, [slot_of[e] for e in uniq], check=False)
        self.resume_from_bank(dst, [slot_of[e] for e in src])

    def _physical(self, values: torch.Tensor, fill, dtype) -> torch.Tensor:
        """A per-env tensor (env order) as a full-size emulator-order one, padding envs = fill."""
        values = torch.as_tensor(values, device=self.device).reshape(-1).to(dtype)
        if values.numel() != self.num_envs:
            raise ValueError("a per-env argument must have num_envs elements")
        if not self._padded:
            return values.contiguous()
        out = torch.full((self.emu.n,), fill, dtype=dtype, device=self.device)
        out[self._phys] = values
        return out

    def _set_physical(self, buf: torch.Tensor, values: torch.Tensor):
        """The reverse of _logical: a per-env tensor (env order) into the envs' rows of an emulator-order one."""
        if self._padded:
            buf[self._phys] = values
        else:
            buf.copy_(values)

    def _take_keys(self, kind: str, frame, out: torch.Tensor | None = None, env0: int = 0, count: int | None = None):
        """The keys of kind "ram", "frame" (frame = (bw, bh, levels)) or "frame+ram" — the second salted
        with the first — of emulator envs [env0, env0 + count) into out (None: a new tensor), on the
        current stream."""
        if kind == "tiles":
            if out is None:
                out = torch.zeros(self.emu.n, dtype=torch.int64, device=self.device)
            self.emu.tiles_eval(keys=out, env0=env0, count=count)
            return out
        salt = None
        if kind != "frame":
            salt = self.emu.cell_keys(self.archive_shift, out=out, env0=env0, count=count)
            if kind == "ram":
                return salt
        return self.emu.frame_keys(*frame, salt=salt, out=out if salt is None else salt, env0=env0, count=count)

    def _cell_keys(self) -> torch.Tensor:
        """The keys archive_key names, in emulator order."""
        return self._take_keys(self.archive_key, self.archive_frame)

    def cell_keys(self) -> torch.Tensor:
        """The cell key of every env (int64, env order) as archive_key has it: pk_cell_keys with
        archive_shift, pk_frame_keys with archive_frame, or the second salted with the first."""
        return self._logical(self._cell_keys())

    def frame_cells(self) -> torch.Tensor:
        """The frame cell image of every env, uint8 (num_envs, C) in env order: the screen in blocks of
        archive_frame's size, each quantised to its levels (pk_frame_keys' cells_dev) — a small global
        observation, and what the "frame" keys are made of.  On the current stream after a pipeline join."""
        self._join_streams()
        bw, bh, levels = self.archive_frame
        cells = torch.zeros((self.emu.n, self.emu.frame_cells(bw, bh)), dtype=torch.uint8, device=self.device)
        self.emu.frame_keys(bw, bh, levels, cells=cells)
        return self._logical(cells)

    def archive_update(self, scores=None, keys=None, mask=None) -> torch.Tensor:
        """Enter every env (those with mask[e] != 0) into the archive: scores default to the running
        episode return (stats.ep_return), keys to cell_keys(); per-env tensors in env order.  Each
        cell's new best episode is checkpointed into the cell's slot together with this class's
        episode return / length and start slot.  On the current stream after a pipeline join, like
        checkpoint_to_bank; no host sync.  Returns the slot each env won (int32, env order, -1 else)."""
        self._require("archive")
        self._join_streams()
        scores = self._physical(self.stats.ep_return if scores is None else scores, float("nan"), torch.float64)
        keys = self._cell_keys() if keys is None else self._physical(keys, -1, torch.int64)
        # padding envs never take part: their mask byte is 0
        mask = self._physical(torch.ones(self.num_envs, dtype=torch.uint8, device=self.device) if mask is None
                              else torch.as_tensor(mask, device=self.device) != 0, 0, torch.uint8)
        self.emu.archive_update(keys, scores, mask, out=self._arch_out)
        won = self._logical(self._arch_out).long()
        self._ledger.store(won, self._gather())
        return won.to(torch.int32)

    def archive_explore(self, mask) -> torch.Tensor:
        """Every env with mask[e] != 0 draws a cell (weight 1 / sqrt(visits + picks + 1)) and continues
        the episode kept there, as resume_from_bank does it; no host sync.  Returns the slot each
        env resumed from (int32, env order, -1 for the others and for rejects)."""
        self._require("archive")
        self._join_streams()
        mask = self._physical(torch.as_tensor(mask, device=self.device) != 0, 0, torch.uint8)
        self.emu.archive_explore(mask, out=self._arch_out)
        # the envs that resumed: the device's own answer, rejects excluded (generic parts carry both)
        if self.tile_view or ((self.frame_stack or self.probes is not None) and not self._generic):
            self._machines_replaced((self._arch_out >= 0).to(torch.uint8), carried=self._generic)
        drawn = self._logical(self._arch_out).long()
        ok, values = self._ledger.fetch(drawn)      # ok: drawn >= 0 and the slot holds an episode
        self._scatter(values, ok)
        return drawn.to(torch.int32)

    _REQUIRES = {   # feature -> (the attribute that is None, False or 0 without it, what to say then)
        "episodes": ("_ledger", "VecEnv(bank_episodes=True) keeps episode checkpoints"),
        "fork": ("_ledger", "VecEnv(bank_episodes=True, fork_slots=...) forks envs"),
        "archive": ("archive_cells", "VecEnv(archive_cells=...) keeps the archive"),
        "exchange": ("archive_exchange", "VecEnv(archive_cells=..., archive_exchange=True) exchanges archive cells"),
        "trajectories": ("record_trajectories", "VecEnv(record_trajectories=True) records trajectories"),
        "novelty": ("novelty_log2", "VecEnv(novelty_log2=...) counts visits"),
    }

    def _require(self, feature: str):
        """Raise unless the constructor was given what `feature` needs."""
        attr, text = self._REQUIRES[feature]
        if not getattr(self, attr):
            raise RuntimeError(text)

    def _exchange(self):
        self._require("exchange")
        self._join_streams()

    def _cell_rows(self) -> torch.Tensor:
        """What this class keeps per slot, for the cells' slots: SlotLedger.rows — row c travels with
        record c of a pack."""
        return self._ledger.rows(self._arch0, self.archive_cells)

    def _place_rows(self, cell_out: torch.Tensor, rows: torch.Tensor):
        """Row i goes to the slot of cell cell_out[i]; the rows of records that won nothing go nowhere."""
        won = cell_out.long()
        self._ledger.place(torch.where(won >= 0, won + self._arch0, -1), rows)

    def archive_export(self) -> dict:
        """The whole archive as host arrays (a full pack, which changes nothing; synchronises):
        "records" uint8 (archive_cells, 48) in cell order, "payloads" uint8 (cells in use,
        emu.archive_payload_bytes), and this class's rows "ck_return", "ck_length", "ck_valid",
        "ck_slots" per cell.  np.savez(path, **d) keeps it across a restart."""
        self._exchange()
        records, payloads, n = self.emu.archive_pack()
        rows = self._cell_rows().cpu().numpy()
        return {"records": records.cpu().numpy(), "payloads": payloads[:int(n)].cpu().numpy(),
                "ck_return": rows[:, 0].copy(), "ck_length": rows[:, 1].copy(), "ck_valid": rows[:, 2] != 0,
                "ck_slots": rows[:, 3].astype(np.int32)}

    def archive_import(self, d) -> torch.Tensor:
        """Merge an archive_export() dict (of this or another VecEnv with the same geometry) into the
        archive (emu.archive_merge): a cell takes an imported record when it is new or strictly
        better, with its slot and its episode return / length / start slot.  Start slots name the
        exporter's state pool: use the same pool.  Returns the cell each record won (int32, -1 else)."""
        self._exchange()
        dev = self.device
        records = torch.from_numpy(np.ascontiguousarray(d["records"], np.uint8)).to(dev)
        payloads = torch.from_numpy(np.ascontiguousarray(d["payloads"], np.uint8)).to(dev)
        rows = torch.from_numpy(np.stack([np.asarray(d["ck_return"], np.float64), np.asarray(d["ck_length"], np.float64),
                                          np.asarray(d["ck_valid"], np.float64), np.asarray(d["ck_slots"], np.float64)],
                                         axis=1)).to(dev)
        if rows.shape[0] != records.shape[0]:
            raise ValueError("archive_import: one statistics row per record")
        out = self.emu.archive_merge(records, payloads)
        self._place_rows(out, rows)
        return out

    def archive_sync(self, group=None, max_payloads: int | None = None):
        """Exchange with the other ranks of a torch.distributed group what the archives learned since
        the last call: a delta pack (this rank's own new visits and picks, and at most max_payloads
        of the cells whose record it replaced; default: all cells — the rest goes with the next
        call), an all_gather of records, payload rows and statistics rows, then a merge of every
        other rank's buffers in ascending rank order.  Counts that came from other ranks are never
        sent on.  A collective: every rank calls it, with the same max_payloads.  World size 1 (or no
        process group) is a no-op.  On the current stream after a pipeline join."""
        import torch.distributed as dist
        from .dist import archive_all_gather
        self._require("exchange")
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            return
        self._join_streams()
        max_payloads = self.archive_cells if max_payloads is None else int(max_payloads)
        records, payloads, _ = self.emu.archive_pack(delta=True, max_payloads=max_payloads)
        recs, pays, rows = archive_all_gather(records, payloads, self._cell_rows(), group)
        me = dist.get_rank(group)
        for r in range(len(recs)):
            if r != me:
                self._place_rows(self.emu.archive_merge(recs[r], pays[r]), rows[r])

    def archive_state(self) -> dict:
        """The archive as host arrays (emu.archive_read; synchronous)."""
        self._require("archive")
        return self.emu.archive_read()

    @staticmethod
    def _trajectory(d: dict, i: int) -> dict:
        """Row i of a trajectories() result as host values (synchronises)."""
        n = int(d["length"][i])
        return {"origin": int(d["origin"][i]), "actions": d["actions"][i, :n].cpu().numpy().copy(),
                "replayable": int(d["flags"][i]) == 0}

    def trajectory(self, env: int) -> dict:
        """How env got where it is: {"origin": the bank slot its episode started from (-1 = the
        template state), "actions": uint8 array of every action since, "replayable": whether resetting
        from origin and stepping through actions rebuilds the env exactly (False after load_state,
        load_from_bank, a RAM write, a reset that kept the machine, or a step past the capacity)}.
        Needs record_trajectories=True; waits for the sub-batch streams and syncs the host."""
        self._require("trajectories")
        self._join_streams()
        p = self.phys(int(env))
        g0 = p // 64 * 64
        return self._trajectory(self.emu.trajectories(g0, min(64, self.emu.n - g0)), p - g0)

    def slot_trajectory(self, slot: int) -> dict:
        """trajectory() of the episode checkpointed in a bank slot; a slot that holds no episode is
        origin -1, no actions, not replayable."""
        self._require("trajectories")
        self._join_streams()
        return self._trajectory(self.emu.bank_trajectories(int(slot), 1), 0)

    def archive_trajectory(self, cell: int) -> dict:
        """trajectory() of the best episode the archive keeps for a cell."""
        self._require("archive")
        if not 0 <= int(cell) < self.archive_cells:
            raise ValueError("archive_trajectory: no such cell")
        return self.slot_trajectory(self._arch0 + int(cell))

    def _range(self, b: int) -> slice:
        return slice(b * self.batch_size, (b + 1) * self.batch_size)

    def _prange(self, b: int) -> slice:
        """Emulator envs of sub-batch b."""
        return slice(b * self.slot, b * self.slot + self.batch_size)

    def phys(self, env):
        """Emulator index of env: sub-batch b lives in emulator envs [b * slot, b * slot + batch_size).
        An int, or a tensor of env indices; the one place with this arithmetic (_env_of is its inverse)."""
        return (env // self.batch_size) * self.slot + env % self.batch_size

    def _env_of(self, phys: int) -> int:
        """The env at emulator index phys (not a padding env's)."""
        return (phys // self.slot) * self.batch_size + phys % self.slot

    def _obs_buffer(self) -> torch.Tensor:
        """What the envs observe, in emulator order: the frame stack, the composite observation or the screen."""
        if self.frame_stack:
            return self.emu.stack
        return self.emu.obs if self.emu.reward else self.emu.screen

    def _logical(self, obs: torch.Tensor) -> torch.Tensor:
        return obs.index_select(0, self._phys) if self._padded else obs

    def _join_streams(self):
        """The current stream waits for every sub-batch stream (steps still in flight)."""
        if self._streams:
            cur = torch.cuda.current_stream(self.device)
            for st in self._streams:
                cur.wait_stream(st)

    def reset(self, seed=None, max_episode_steps=None, reward_scale=None):
        """Reset every env; max_episode_steps / reward_scale (Environment.reset's arguments,
        environment.py:1233) apply to all envs from here on, None keeps the current values.  Unlike
        the single Environment (where each reset() restores 20480 / 4.0, as the reference does), they
        are the VecEnv's configuration: its device auto-resets keep them."""
        self._join_streams()
        if max_episode_steps is not None or reward_scale is not None:
            mes = max_episode_steps if max_episode_steps is not None else getattr(self.emu, "max_episode_steps", 20480)
            rsc = reward_scale if reward_scale is not None else getattr(self.emu, "reward_scale", 4.0)
            grows = _seen_cap_log2(mes) > self._cap_lg      # the seen set never shrinks
            self._cap_lg = max(self._cap_lg, _seen_cap_log2(mes))
            self.emu.set_episode_params(mes, rsc)
            if grows and self._ledger is not None and not self._generic:   # the device emptied every slot's episode part
                self._ledger.invalidate()
        if self._slots is None:
            obs = self._logical(self.emu.reset())
        else:
            for b in range(self.num_batches):
                self._draw_slots(self._prange(b))
            obs = self._logical(self.emu.reset_from(self._slots))
        if self.frame_stack:
            obs = self._logical(self.emu.stack_push(fill_only=True))
        if self.probes is not None:
            self.emu.probes_eval(rebase_only=True, features=self._probe_feat)
        if self.tile_view:
            self.emu.tiles_eval()
        self.t = 0
        self._log_wait = 0
        if self.sticky_errors is not None:
            self.sticky_errors.zero_()
        return obs, []

    def raise_if_failed(self, codes: torch.Tensor | None = None):
        """Raise the reference's exception for the first env that hit one since the last check
        (codes: the sticky error codes, or a snapshot of them)."""
        codes = self.sticky_errors if codes is None else codes
        if codes is None:
            return
        bad = torch.nonzero(codes).flatten()
        if bad.numel():
            from ._native import ERR_EXCEPTIONS
            p = int(bad[0])
            code = int(codes[p])
            codes.zero_()
            raise ERR_EXCEPTIONS.get(code, RuntimeError)(
                f"env {self._env_of(p)}: reference reward stack raises here (PK_ERR {code}); {bad.numel()} env(s) failed")

    def _novelty_take(self, psl: slice):
        """The keys of emulator envs psl into _nov_keys, on the current stream; no table is touched."""
        self._take_keys(self.novelty_key, self.novelty_frame, self._nov_keys, psl.start, psl.stop - psl.start)

    def _novelty_count(self, psl: slice) -> torch.Tensor:
        """Count the keys taken for emulator envs psl (one table update, on the current stream);
        returns their bonus."""
        self.emu.counts_update(self._nov_keys, None, psl.start, psl.stop - psl.start, self.novelty_beta, False,
                               self._nov_counts, self._nov_bonus)
        return self._nov_bonus[psl]

    def _novelty_flush(self):
        """Count the sub-batches that were sent and not received yet, in batch order (the streams are
        joined).  Their bonus stays in _nov_bonus, which only the sub-batch's next count overwrites;
        the recv() that returns such a sub-batch adds it to the rewards."""
        for b, due in enumerate(self._nov_due):
            if due == 1:
                self._nov_due[b] = 2
                self._novelty_count(self._prange(b))

    def _novelty_last(self, t):
        self._require("novelty")
        self._join_streams()
        return self._logical(t).clone()

    @property
    def novelty_keys(self) -> torch.Tensor:
        """The key every env's last step ended on (int64, env order; -1 before the first step)."""
        return self._novelty_last(self._nov_keys)

    @property
    def novelty_counts(self) -> torch.Tensor:
        """The visits of that key when the step was counted, itself included (int64, env order)."""
        return self._novelty_last(self._nov_counts)

    @property
    def novelty_bonus(self) -> torch.Tensor:
        """novelty_beta / sqrt(novelty_counts): the part of the last returned reward that is the bonus."""
        return self._novelty_last(self._nov_bonus)

    def counts_sync(self, group=None):
        """Add up the visit counts of the ranks of a torch.distributed group: a delta pack (what this
        rank counted itself since the last call), an all_gather of the records, then every other
        rank's records added in ascending rank order, as counts that are never sent on.  A
        collective: every rank calls it.  World size 1 (or no process group) is a no-op.  On the
        current stream after a pipeline join; reads the ranks' record counts back (a host sync).
        In a recv() / send() loop the sub-batches that are sent and not received yet are counted
        here, so that they travel with this call; their recv() returns the bonus all the same."""
        from .dist import counts_all_gather
        self._require("novelty")
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            return
        self._join_streams()
        self._novelty_flush()
        records, n = self.emu.counts_pack_raw(delta=True)
        me = dist.get_rank(group)
        for r, rec in enumerate(counts_all_gather(records, n, group)):
            if r != me:
                self.emu.counts_add(rec, foreign=True)

    def _step_range(self, b: int, actions: torch.Tensor, count_now: bool = False):
        """Step sub-batch b (envs _range(b)) on the current stream, then book-keep and auto-reset.
        With the novelty bonus the step's keys are taken here; count_now also counts them (step():
        one stream, batch order), else recv() does."""
        sl, psl = self._range(b), self._prange(b)
        if self.num_batches == 1:
            obs, rew, term, trunc = self.emu.step(actions)
        else:
            obs, rew, term, trunc = self.emu.step_range(psl.start, actions)
        if self.probes is not None:     # rew and term are views of the arrays this adds and ORs into
            self.emu.probes_eval(rewards=self.emu.rewards, terminals=self.emu.terminals, features=self._probe_feat,
                                 env0=psl.start, count=self.batch_size)
        self.stats.update(rew, term, batch=b, envs=sl)
        if self.info_stats is not None:
            self.info_stats.update(self.emu.info[:, psl], self.emu.info_flag[psl], batch=b)
        if self.sticky_errors is not None:
            se = self.sticky_errors[psl]
            torch.where(se != 0, se, self.emu.errors[psl], out=se)
        rewards = rew.clone()
        if self.novelty_log2:       # the frame the step ended on, before an auto-reset replaces it
            self._novelty_take(psl)
            if count_now:
                rewards += self._novelty_count(psl)
                self._nov_due[b] = 0
            else:
                self._nov_due[b] = 1
        terminals = term.to(torch.bool)
        truncations = trunc.to(torch.bool)
        # auto-reset the finished envs (no host sync); their obs is the first obs of the next episode
        if self._slots is not None:
            self._draw_slots(psl, term)
            if self.num_batches == 1:
                self.emu.reset_from(self._slots, term)
            else:
                self.emu.reset_range_from(psl.start, self.batch_size, self._slots, self.emu.terminals)
        elif self.num_batches == 1:
            self.emu.reset(term)
        else:
            self.emu.reset_range(psl.start, self.batch_size, self.emu.terminals)
        if self.probes is not None:  # the finished envs are measured from their reset state; the features stay the step's
            self.emu.probes_eval(self.emu.terminals, rebase_only=True, env0=psl.start, count=self.batch_size)
        if self.frame_stack:        # one launch: the finished envs fill from their reset frame, the others push
            obs = self.emu.stack_push(self.emu.terminals, env0=psl.start, count=self.batch_size)[psl]
        if self.tile_view:          # one launch: the state the step ended on, or the reset state of a finished env
            self.emu.tiles_eval(env0=psl.start, count=self.batch_size)
        return obs, rewards, terminals, truncations

    def _log(self, deferred: bool = False):
        infos = []
        if not (self.log_interval and self._batch_steps % (self.log_interval * self.num_batches) == 0):
            return infos
        if deferred and self._streams:
            # the sub-batch pipeline: no host sync here (it would drain every stream's queue).  Each
            # stream, after its latest step, moves its statistics rows and error codes into the
            # snapshot and restarts them; recv() reads the snapshot once the step it waits for is
            # the last of these (_read_logs)
            for b, st in enumerate(self._streams):
                with torch.cuda.stream(st):
                    self.stats.snapshot(b)
                    if self.info_stats is not None:
                        self.info_stats.snapshot(b)
                    if self.sticky_errors is not None:
                        psl = self._prange(b)
                        self._snap_err[psl].copy_(self.sticky_errors[psl])
                        self.sticky_errors[psl].zero_()
                    self._snap_events[b].record(st)
            self.logs_fired += 1
            self._log_wait = self.num_batches
            return infos
        # the sticky error codes and the statistics rows are written by the sub-batch streams:
        # wait for every one of them before reading and clearing (the next send() orders its
        # stream after these reads again through st.wait_stream(current))
        self._join_streams()
        self.raise_if_failed()
        self.logs_fired += 1
        infos = [self.stats.allreduce()]
        if self.info_stats is not None:
            infos[0].update(self.info_stats.allreduce())
        return infos

    def _read_logs(self):
        """The deferred interval's record: wait (host) for the snapshot, raise its first error code,
        all-reduce its rows."""
        cur = torch.cuda.current_stream(self.device)
        for e in self._snap_events:
            cur.wait_event(e)
        self.raise_if_failed(self._snap_err)
        infos = [self.stats.allreduce(snapshot=True)]
        if self.info_stats is not None:
            infos[0].update(self.info_stats.allreduce(snapshot=True))
        return infos

    def step(self, actions):
        """Step every env (all sub-batches) with actions of shape (num_envs,)."""
        if isinstance(actions, np.ndarray):
            actions = torch.from_numpy(actions)
        a = actions.to(device=self.device, dtype=torch.uint8).contiguous()
        self._join_streams()
        # an interval that fired on a send() and has not been read by a recv() yet
        pending = []
        if self._log_wait:
            self._log_wait = 0
            pending = self._read_logs()
        if self.novelty_log2:
            self._novelty_flush()
        if self.num_batches == 1:
            obs, rewards, terminals, truncations = self._step_range(0, a, True)
        else:
            outs = [self._step_range(b, a[self._range(b)], True) for b in range(self.num_batches)]
            obs = self._logical(self._obs_buffer())
            rewards = torch.cat([o[1] for o in outs])
            terminals = torch.cat([o[2] for o in outs])
            truncations = torch.cat([o[3] for o in outs])
        self.t += 1
        self._batch_steps += self.num_batches
        return obs, rewards, terminals, truncations, pending + self._log()

    def save_state(self, env: int) -> bytes:
        """PyBoy v9 savestate of one env (pk_snapshot; environment.py:208-213 per env)."""
        return self.emu.snapshot(self.phys(env))

    def load_state(self, env: int, state: bytes):
        """Install a v9 savestate into one env (pk_load_env; pyboy_binding.py:59-69)."""
        self.emu.load_env(self.phys(env), state)
        if self.frame_stack or self.probes is not None or self.tile_view:
            self._join_streams()
            m = torch.zeros(self.emu.n, dtype=torch.uint8, device=self.device)
            m[self.phys(env)] = 1
            self._machines_replaced(m)

    @property
    def probe_values(self) -> torch.Tensor:
        """The probe values every env's last step ended on, or its last reset or rebase produced (int32
        (num_envs, m), env order); needs probes= and probe_features=True."""
        if self._probe_feat is None:
            raise RuntimeError("VecEnv(probes=..., probe_features=True) keeps the probe values")
        self._join_streams()
        return self._logical(self._probe_feat).clone()

    def tile_obs(self) -> torch.Tensor:
        """The tile view, int16 (P, 18, 20) per env, -1 = nothing; needs tile_view=.  Between a recv() and
        its send() of the sub-batch pipeline: the rows of the sub-batch recv() returned, a view of the
        emulator's buffer that the sub-batch's next step overwrites (no copy, no wait beyond recv()'s).
        Otherwise every env's rows in env order, after a pipeline join."""
        if not self.tile_view:
            raise RuntimeError('VecEnv(tile_view="id" or "hash") keeps the tile view')
        if self.num_batches > 1 and self._current is not None:
            return self.emu.tiles[self._prange(self._current)]
        self._join_streams()
        return self._logical(self.emu.tiles)

    def video_recorder(self, envs, capacity: int = 1024):
        """A FrameRecorder (pokegym_amd/video.py) of the given envs' screens: call .capture() after
        each step, .write(path, k) at an episode's end (the reference's save_video per env)."""
        from .video import FrameRecorder
        return FrameRecorder(self.emu, [self.phys(int(e)) for e in envs], capacity)

    def exploration_map(self, group=None) -> torch.Tensor:
        """Sum of every env's counts_map over all ranks (int64 (444, 436), RCCL all-reduce) — the
        aggregate of the reference's per-env info["pokemon_exploration_map"]; needs heatmap=True."""
        hm = getattr(self.emu, "heatmap", None)
        if hm is None:
            raise RuntimeError("VecEnv(heatmap=True) keeps the per-env counts_map")
        out = hm.sum(dim=0, dtype=torch.int64)
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            dist.all_reduce(out, op=dist.ReduceOp.SUM, group=group)
        return out

    # PufferLib async API: async_reset, then repeatedly recv() -> policy -> send(actions)
    def async_reset(self, seed=None):
        obs, infos = self.reset(seed)
        if self.num_batches == 1:   # one batch: send() steps synchronously on the current stream
            z = torch.zeros(self.num_envs, device=self.device)
            f = torch.zeros(self.num_envs, dtype=torch.bool, device=self.device)
            self._pending = (obs, z, f, f, infos)
            return
        cur = torch.cuda.current_stream(self.device)
        z = torch.zeros(self.num_envs, dtype=torch.float64, device=self.device)
        f = torch.zeros(self.num_envs, dtype=torch.bool, device=self.device)
        self._pending = [(z[self._range(b)], f[self._range(b)], f[self._range(b)]) for b in range(self.num_batches)]
        for b in range(self.num_batches):
            self._events[b].record(cur)
        self._ready = list(range(self.num_batches))
        self._current = None
        self._nov_due = [0] * self.num_batches

    def recv(self):
        """The next finished sub-batch: (obs, rewards, terminals, truncations, infos, env_ids, masks),
        device tensors over its batch_size envs; the current stream waits for its step (no host sync).
        The num_batches-th recv() after a logging interval fired reads that interval's snapshot (a
        host wait for the streams' steps of the interval — the last of which is the one received
        here): it raises the first reference exception an env hit, else returns the all-reduced
        record in infos."""
        if self.num_batches == 1:
            obs, rew, term, trunc, infos = self._pending
            return obs, rew, term, trunc, infos, self.env_ids, self.masks
        if self._current is not None:
            raise RuntimeError("recv() called twice without send()")
        if not self._ready:
            raise RuntimeError("recv() before async_reset()")
        logged = []
        if self._log_wait:
            self._log_wait -= 1
            if self._log_wait == 0:
                logged = self._read_logs()
        b = self._ready.pop(0)
        torch.cuda.current_stream(self.device).wait_event(self._events[b])
        self._current = b
        sl = self._range(b)
        rew, term, trunc = self._pending[b]
        if self._nov_due[b]:        # the table is updated here, on the consumer's stream, in recv() order
            psl = self._prange(b)   # (a counts_sync() in between has counted the sub-batch already)
            rew = rew + (self._novelty_count(psl) if self._nov_due[b] == 1 else self._nov_bonus[psl])
            self._nov_due[b] = 0
        obs = self._obs_buffer()
        infos, self._pending_infos = getattr(self, "_pending_infos", []) + logged, []
        return obs[self._prange(b)], rew, term, trunc, infos, self.env_ids[sl], self.masks[sl]

    def current_envs(self) -> slice:
        """Local env range of the sub-batch the last recv() returned (host-side, no sync)."""
        return self._range(self._current) if self.num_batches > 1 else slice(0, self.num_envs)

    def send(self, actions):
        """Step the sub-batch the last recv() returned, with actions (batch_size,), on its own stream."""
        if self.num_batches == 1:
            self._pending = self.step(actions)
            return
        b = self._current
        if b is None:
            raise RuntimeError("send() without a preceding recv()")
        if isinstance(actions, np.ndarray):
            actions = torch.from_numpy(actions)
        cur = torch.cuda.current_stream(self.device)
        a = actions.to(device=self.device, dtype=torch.uint8).contiguous()
        st = self._streams[b]
        st.wait_stream(cur)                       # the policy's actions (and its reads of obs)
        with torch.cuda.stream(st):
            a.record_stream(st)
            _, rew, term, trunc = self._step_range(b, a)
            self._events[b].record(st)
        self._pending[b] = (rew, term, trunc)
        self._batch_steps += 1
        if self._batch_steps % self.num_batches == 0:
            self.t += 1
        logged = self._log(deferred=True)
        if logged:
            self._pending_infos = logged
        self._ready.append(b)
        self._current = None

    def close(self):
        if self._streams:
            torch.cuda.synchronize(self.device)
        self.emu.close()


def make_sharded_vecenv(num_envs_total: int, **kwargs) -> VecEnv:
    """This rank's shard (contiguous env ids) of a num_envs_total batch; one process per GPU."""
    rank, world, local = env_rank()
    start, end = shard_range(num_envs_total, world, rank)
    kwargs.setdefault("device", local)
    return VecEnv(end - start, env_offset=start, **kwargs)
