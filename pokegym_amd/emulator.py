"""BatchedEmulator — N Game Boys on one MI355X behind the C ABI (include/pokegym_amd.h).

This is the device-side replacement of pokegym's per-process PyBoy instance
(pokegym/pyboy_binding.py:42-91): one call to `step(actions)` advances every env by one
env-step (press, 24 frames, release before frame 8, rasterise frame 24) inside one HIP launch.
With `reward=True` the same call also runs pokegym's reward stack and builds the (72, 80, 4)
observation (environment.py:1338-1612, :256-274) on the device.  Device buffers are
PyTorch-ROCm tensors; the kernels run on the caller's current HIP stream.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _native
from .info import NFIELDS, event_dicts, info_dict
from .spaces import stack_shape
from ._native import (COLS, ERR_EXCEPTIONS, OBS_SHAPE, PK_F_RELOAD_ON_RESET, PK_F_RENDER, PK_F_REWARD, ROWS,
                      STATE_V9_BYTES, check)


class _CudaArray:
    """__cuda_array_interface__ shim to wrap a handle-owned device buffer without a copy."""

    def __init__(self, ptr: int, shape, typestr: str):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr,
                                         "data": (ptr, False), "version": 2, "strides": None}


class _HostArray:
    """__array_interface__ shim: the same for a handle whose buffers are host memory (device cpu)."""

    def __init__(self, ptr: int, shape, typestr: str):
        self.__array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "version": 3}


def _u8p(buf: bytes | bytearray | np.ndarray):
    a = np.frombuffer(bytes(buf), dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


class BatchedEmulator:
    def __init__(self, rom: bytes, n_envs: int, state: bytes | None = None, device: int = 0,
                 frame_skip: int = 24, release_frame: int = 8, render: bool = True,
                 max_episode_steps: int = 20480, reward: bool = False, reload_on_reset: bool = False,
                 reward_scale: float = 4.0, heatmap: bool = False):
        self._L, self.device, on_device = self._backend(device)
        self.n = int(n_envs)
        self._rom, rom_p = _u8p(rom)
        cfg = _native.PkConfig()
        cfg.n_envs = self.n
        cfg.device = device
        cfg.rom = rom_p
        cfg.rom_len = len(self._rom)
        if state is not None:
            self._state, st_p = _u8p(state)
            cfg.state = st_p
            cfg.state_len = len(self._state)
        cfg.frame_skip = frame_skip
        cfg.release_frame = release_frame
        cfg.flags = ((PK_F_RENDER if render else 0) | (PK_F_REWARD if reward else 0)
                     | (PK_F_RELOAD_ON_RESET if reload_on_reset else 0)
                     | (_native.PK_F_HEATMAP if (heatmap and reward) else 0))
        cfg.max_episode_steps = max_episode_steps
        cfg.reward_scale = reward_scale
        h = ctypes.c_void_p()
        with on_device:
            check(self._L.pk_create(ctypes.byref(cfg), ctypes.byref(h)), "pk_create")
        self._h = h
        self.render = render
        self.reward = reward
        self.max_episode_steps, self.reward_scale = int(max_episode_steps), float(reward_scale)
        L, n = self._L, self.n
        self.screen = self._view(L.pk_screen_ptr(h), (n, ROWS, COLS), "|u1")
        self.obs = None
        self.errors = None
        self.heatmap = None     # int32 (n, 444, 436) with heatmap=True
        self.info_bits = None
        self.info = None        # f64 (PK_INFO_NFIELDS, n) view, field-major (pokegym_amd/info.py FIELDS)
        self.info_flag = None   # u8 (n,): 1 where the last step built the reference's info dict
        if reward:
            self.obs = self._view(L.pk_obs_ptr(h), (n,) + OBS_SHAPE, "|u1")
            self.errors = self._view(L.pk_error_ptr(h), (n,), "<i4")
            stride = int(L.pk_info_stride(h))
            self.info = self._view(L.pk_info_ptr(h), (NFIELDS, stride), "<f8")[:, :n]
            # event-monitor bits (int32 words; pokegym_amd/info.py event_dicts)
            self.info_bits = self._view(L.pk_info_bits_ptr(h), (5, stride), "<i4")[:, :n]
            self.info_flag = self._view(L.pk_info_flag_ptr(h), (n,), "|u1")
            hp = L.pk_heatmap_ptr(h)
            if hp:   # int32 (n, 444, 436) counts_map of every env (environment.py:448, :648-679)
                self.heatmap = self._view(hp, (n,) + _native.HEAT_SHAPE, "<i4")
        self.rewards = torch.zeros(self.n, dtype=torch.float64, device=self.device)
        self.terminals = torch.zeros(self.n, dtype=torch.uint8, device=self.device)
        self.truncations = torch.zeros(self.n, dtype=torch.uint8, device=self.device)
        self.actions = torch.full((self.n,), 8, dtype=torch.uint8, device=self.device)  # sub-batch staging

    def _backend(self, device: int):
        """What depends on where the handle's buffers live: the loaded library, the torch device, and the
        context pk_create runs in.  The product has one backend: a ROCm GPU."""
        L = _native.load()
        if not torch.cuda.is_available():
            raise _native.PkError("no ROCm GPU visible: the HIP path has no CPU fallback")
        dev = torch.device("cuda", device)
        return L, dev, torch.cuda.device(dev)

    def _view(self, ptr: int, shape, typestr: str) -> torch.Tensor:
        """A tensor over a handle-owned buffer on the handle's device, without a copy."""
        if self.device.type == "cpu":
            return torch.from_numpy(np.asarray(_HostArray(ptr, shape, typestr)))
        return torch.as_tensor(_CudaArray(ptr, shape, typestr), device=self.device)

    # -- stream helpers -----------------------------------------------------------------
    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # -- hot path -----------------------------------------------------------------------
    def step(self, actions: torch.Tensor):
        """actions: uint8[n] on this device.  Returns (obs, rewards, terminals, truncations) where
        obs is the (n, 72, 80, 4) observation with reward=True, else the (n, 144, 160) screen."""
        if actions.dtype != torch.uint8 or actions.device != self.device or actions.numel() != self.n:
            raise ValueError("actions must be a uint8 tensor of n_envs elements on the emulator's device")
        actions = actions.contiguous()
        check(self._L.pk_step(self._h, ctypes.c_void_p(actions.data_ptr()), None,
                              ctypes.c_void_p(self.rewards.data_ptr()),
                              ctypes.c_void_p(self.terminals.data_ptr()),
                              ctypes.c_void_p(self.truncations.data_ptr()), self._stream()), "pk_step")
        return (self.obs if self.reward else self.screen), self.rewards, self.terminals, self.truncations

    def step_range(self, env0: int, actions: torch.Tensor):
        """One env-step of the sub-batch [env0, env0 + len(actions)) only (pk_step_range), on the
        current stream: env0 is a multiple of 64, the end anywhere up to n.  Returns views of
        the sub-batch's (obs, rewards, terminals, truncations)."""
        count = actions.numel()
        sl = slice(env0, env0 + count)
        self.actions[sl].copy_(actions.reshape(-1))
        check(self._L.pk_step_range(self._h, env0, count, ctypes.c_void_p(self.actions.data_ptr()),
                                    ctypes.c_void_p(self.rewards.data_ptr()), ctypes.c_void_p(self.terminals.data_ptr()),
                                    ctypes.c_void_p(self.truncations.data_ptr()), self._stream()), "pk_step_range")
        obs = self.obs if self.reward else self.screen
        return obs[sl], self.rewards[sl], self.terminals[sl], self.truncations[sl]

    def reset_range(self, env0: int, count: int, mask: torch.Tensor | None = None):
        """Reset the envs of [env0, env0 + count) — all of them, or those with mask[e] != 0 where
        mask is a FULL-size (n) device u8 tensor (e.g. `terminals`; only the range is read) —
        pk_reset_range on the current stream."""
        mp = None
        if mask is not None:
            if mask.dtype != torch.uint8 or mask.device != self.device or mask.numel() != self.n or not mask.is_contiguous():
                raise ValueError("reset_range mask must be a contiguous uint8 tensor of n_envs elements on the device")
            mp = ctypes.c_void_p(mask.data_ptr())
        check(self._L.pk_reset_range(self._h, env0, count, mp, self._stream()), "pk_reset_range")
        obs = self.obs if self.reward else self.screen
        return obs[env0:env0 + count]

    def reset(self, mask: torch.Tensor | None = None):
        """Reset all envs (mask None) or those with mask[e] != 0 (device tensor).  Returns the obs."""
        mp = None
        if mask is not None:
            mask = mask.to(device=self.device, dtype=torch.uint8).contiguous()
            mp = ctypes.c_void_p(mask.data_ptr())
        check(self._L.pk_reset(self._h, mp, self._stream()), "pk_reset")
        return self.obs if self.reward else self.screen

    # -- savestate bank (stream-ordered except create / put / get / rejects) --------------
    def bank_create(self, n_slots: int):
        """Give the handle a bank of n_slots savestate slots in device memory (pk_bank_create; once)."""
        check(self._L.pk_bank_create(self._h, int(n_slots)), "pk_bank_create")

    @property
    def bank_slots(self) -> int:
        return int(self._L.pk_bank_slots(self._h))

    def bank_put(self, slot: int, state: bytes):
        """Parse a v9 savestate into a slot (pk_bank_put; synchronous)."""
        a, p = _u8p(state)
        check(self._L.pk_bank_put(self._h, int(slot), p, len(a)), "pk_bank_put")

    def bank_get(self, slot: int) -> bytes:
        """The v9 savestate a filled slot holds (pk_bank_get; synchronous)."""
        out = np.zeros(STATE_V9_BYTES, np.uint8)
        check(self._L.pk_bank_get(self._h, int(slot), out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), len(out)),
              "pk_bank_get")
        return out.tobytes()

    def _slots_ptr(self, slot_of_env: torch.Tensor):
        if (slot_of_env.dtype != torch.int32 or slot_of_env.device != self.device or slot_of_env.numel() != self.n
                or not slot_of_env.is_contiguous()):
            raise ValueError("slot_of_env must be a contiguous int32 tensor of n_envs elements on the emulator's device")
        return ctypes.c_void_p(slot_of_env.data_ptr())

    def bank_save(self, slot_of_env: torch.Tensor, env0: int = 0, count: int | None = None):
        """slot[slot_of_env[e]] <- env e for the envs of [env0, env0 + count) with a slot >= 0
        (pk_bank_save, on the current stream; slot_of_env is a FULL-size int32 tensor)."""
        count = self.n - env0 if count is None else count
        check(self._L.pk_bank_save(self._h, self._slots_ptr(slot_of_env), env0, count, self._stream()), "pk_bank_save")

    def bank_load(self, slot_of_env: torch.Tensor, env0: int = 0, count: int | None = None):
        """env e <- slot[slot_of_env[e]] with load_env's semantics (pk_bank_load, on the current stream)."""
        count = self.n - env0 if count is None else count
        check(self._L.pk_bank_load(self._h, self._slots_ptr(slot_of_env), env0, count, self._stream()), "pk_bank_load")

    def bank_enable_episodes(self):
        """Let the bank's slots carry episode parts (pk_bank_enable_episodes; once, synchronous; needs
        reward=True and a bank)."""
        check(self._L.pk_bank_enable_episodes(self._h), "pk_bank_enable_episodes")

    @property
    def bank_has_episodes(self) -> bool:
        return bool(self._L.pk_bank_has_episodes(self._h))

    def bank_enable_generic_episodes(self, probes: bool = True, stack: bool = True):
        """Let the bank's slots of an emulator with reward=False carry generic episode parts: every lane
        register raw, with probes=True the probe state words, with stack=True the frame stack rows
        (pk_bank_enable_generic_episodes; once, synchronous; needs a bank, and probes_create /
        stack_create before it for the parts asked for).  bank_checkpoint, bank_resume and the archive
        then work as on a reward emulator."""
        parts = (_native.PK_GEP_PROBES if probes else 0) | (_native.PK_GEP_STACK if stack else 0)
        check(self._L.pk_bank_enable_generic_episodes(self._h, parts), "pk_bank_enable_generic_episodes")

    @property
    def generic_parts(self) -> int | None:
        """The PK_GEP_* parts the slots carry, None without generic episode parts."""
        v = int(self._L.pk_bank_generic_parts(self._h))
        return (v & 0x7FFFFFFF) if v else None

    @property
    def generic_episode_bytes(self) -> int:
        """Bytes per slot of the generic episode part, 0 without."""
        return int(self._L.pk_bank_generic_episode_bytes(self._h))

    def bank_checkpoint(self, slot_of_env: torch.Tensor, env0: int = 0, count: int | None = None):
        """bank_save plus the episode part of every saved env: step counter, reward bookkeeping, seen
        set, visited mask (pk_bank_checkpoint, on the current stream)."""
        count = self.n - env0 if count is None else count
        check(self._L.pk_bank_checkpoint(self._h, self._slots_ptr(slot_of_env), env0, count, self._stream()),
              "pk_bank_checkpoint")

    def bank_resume(self, slot_of_env: torch.Tensor, env0: int = 0, count: int | None = None):
        """env e continues the episode checkpointed in slot[slot_of_env[e]]: machine state, episode
        part and a rebuilt `obs` row (pk_bank_resume, on the current stream).  A slot without an
        episode part leaves its env alone and counts in bank_rejects()."""
        count = self.n - env0 if count is None else count
        check(self._L.pk_bank_resume(self._h, self._slots_ptr(slot_of_env), env0, count, self._stream()),
              "pk_bank_resume")

    def reset_range_from(self, env0: int, count: int, slot_of_env: torch.Tensor, mask: torch.Tensor | None = None):
        """reset_range with the template of env e taken from slot[slot_of_env[e]] (a negative slot:
        the emulator's own template) — pk_reset_from on the current stream."""
        mp = None
        if mask is not None:
            if mask.dtype != torch.uint8 or mask.device != self.device or mask.numel() != self.n or not mask.is_contiguous():
                raise ValueError("reset_range_from mask must be a contiguous uint8 tensor of n_envs elements on the device")
            mp = ctypes.c_void_p(mask.data_ptr())
        check(self._L.pk_reset_from(self._h, env0, count, mp, self._slots_ptr(slot_of_env), self._stream()), "pk_reset_from")
        obs = self.obs if self.reward else self.screen
        return obs[env0:env0 + count]

    def reset_from(self, slot_of_env: torch.Tensor, mask: torch.Tensor | None = None):
        """reset() with a slot per env (pk_reset_from over every env).  Returns the obs."""
        if mask is not None:
            mask = mask.to(device=self.device, dtype=torch.uint8).contiguous()
        self.reset_range_from(0, self.n, slot_of_env, mask)
        return self.obs if self.reward else self.screen

    def bank_rejects(self) -> int:
        """Envs whose slot was out of range or empty since the last call (pk_bank_rejects; synchronous)."""
        v = ctypes.c_uint64()
        check(self._L.pk_bank_rejects(self._h, ctypes.byref(v)), "pk_bank_rejects")
        return int(v.value)

    # -- exploration archive on the bank (stream-ordered except create / read) ------------
    def archive_create(self, slot0: int, n_cells: int, seed: int = 0):
        """An archive of n_cells cells over bank slots [slot0, slot0 + n_cells) (pk_archive_create;
        once, synchronous; needs bank_enable_episodes)."""
        check(self._L.pk_archive_create(self._h, int(slot0), int(n_cells), int(seed) & (2 ** 64 - 1)), "pk_archive_create")

    @property
    def archive_cells(self) -> int:
        return int(self._L.pk_archive_cells(self._h))

    def _full(self, t: torch.Tensor | None, dtype, what: str):
        """Pointer of a full-size per-env argument (None stays NULL)."""
        if t is None:
            return None
        if t.dtype != dtype or t.device != self.device or t.numel() != self.n or not t.is_contiguous():
            raise ValueError(f"{what} must be a contiguous {dtype} tensor of n_envs elements on the emulator's device")
        return ctypes.c_void_p(t.data_ptr())

    def cell_keys(self, shift: int = 0, out: torch.Tensor | None = None, env0: int = 0, count: int | None = None):
        """int64 (n,) cell keys map | (x >> shift) << 8 | (y >> shift) << 16 | badges << 24 of the
        envs of the range (pk_cell_keys, on the current stream); the rest of `out` is untouched."""
        if out is None:
            out = torch.zeros(self.n, dtype=torch.int64, device=self.device)
        count = self.n - env0 if count is None else count
        check(self._L.pk_cell_keys(self._h, int(shift), self._full(out, torch.int64, "keys"), env0, count,
                                   self._stream()), "pk_cell_keys")
        return out

    def frame_cells(self, bw: int = 16, bh: int = 16) -> int:
        """Blocks of bw x bh pixels a screen has, (160 / bw) * (144 / bh); 0 for a pair frame_keys
        does not take (pk_frame_cells)."""
        return int(self._L.pk_frame_cells(int(bw), int(bh)))

    def frame_keys(self, bw: int = 16, bh: int = 16, levels: int = 8, screen: torch.Tensor | None = None,
                   salt: torch.Tensor | None = None, out: torch.Tensor | None = None, cells: torch.Tensor | None = None,
                   env0: int = 0, count: int | None = None):
        """int64 (n,) cell keys of the envs' frames, downscaled to blocks of bw x bh pixels and
        quantised to `levels` levels (pk_frame_keys, on the current stream); the rest of `out` is
        untouched.  screen: a uint8 (n, 144, 160) tensor to read in the place of the emulator's own
        screen (which needs render=True).  salt: int64 (n,) words mixed into the keys, e.g.
        cell_keys() — `out` itself will do; a salt of -1 ("no cell") stays -1.  cells: a uint8
        (n, frame_cells(bw, bh)) tensor that receives the cell image of the range's envs."""
        if out is None:
            out = torch.zeros(self.n, dtype=torch.int64, device=self.device)
        count = self.n - env0 if count is None else count
        sp = cp = None
        if screen is not None:
            if (screen.dtype != torch.uint8 or screen.device != self.device or tuple(screen.shape) != (self.n, ROWS, COLS)
                    or not screen.is_contiguous()):
                raise ValueError("screen must be a contiguous uint8 (n_envs, 144, 160) tensor on the emulator's device")
            sp = ctypes.c_void_p(screen.data_ptr())
        if cells is not None:
            c = self.frame_cells(bw, bh)
            if (cells.dtype != torch.uint8 or cells.device != self.device or not cells.is_contiguous()
                    or (c and tuple(cells.shape) != (self.n, c))):
                raise ValueError("cells must be a contiguous uint8 (n_envs, frame_cells(bw, bh)) tensor on the emulator's device")
            cp = ctypes.c_void_p(cells.data_ptr())
        check(self._L.pk_frame_keys(self._h, int(bw), int(bh), int(levels), sp, self._full(salt, torch.int64, "salt"),
                                    self._full(out, torch.int64, "keys"), cp, env0, count, self._stream()),
              "pk_frame_keys")
        return out

    def archive_update(self, keys: torch.Tensor, scores: torch.Tensor, mask: torch.Tensor | None = None,
                       env0: int = 0, count: int | None = None, out: torch.Tensor | None = None):
        """Enter the envs of the range into the archive under keys (int64: the 64 key bits; -1 is the
        reserved "no cell") with scores (float64; NaN takes no part), full-size tensors; every
        cell's new best env is checkpointed into the cell's slot (pk_archive_update, on the
        current stream).  out (int32, full size) receives the winners' slots over the range, -1 else."""
        count = self.n - env0 if count is None else count
        check(self._L.pk_archive_update(self._h, self._full(keys, torch.int64, "keys"),
                                        self._full(scores, torch.float64, "scores"), self._full(mask, torch.uint8, "mask"),
                                        env0, count, self._full(out, torch.int32, "out"), self._stream()),
              "pk_archive_update")
        return out

    def archive_explore(self, mask: torch.Tensor | None = None, env0: int = 0, count: int | None = None,
                        out: torch.Tensor | None = None):
        """Every masked env of the range draws a cell by visit count and resumes the episode in its
        slot (pk_archive_explore, on the current stream).  out receives the slots drawn, -1 else."""
        count = self.n - env0 if count is None else count
        check(self._L.pk_archive_explore(self._h, self._full(mask, torch.uint8, "mask"), env0, count,
                                         self._full(out, torch.int32, "out"), self._stream()), "pk_archive_explore")
        return out

    def archive_read(self) -> dict:
        """The archive as host arrays (pk_archive_read; synchronous): used, overflow, and per cell
        keys (uint64), scores, lengths, visits, picks."""
        k = self.archive_cells
        used, overflow = ctypes.c_uint32(), ctypes.c_uint64()
        keys, scores = np.zeros(k, np.uint64), np.zeros(k, np.float64)
        lengths, visits, picks = np.zeros(k, np.uint32), np.zeros(k, np.uint32), np.zeros(k, np.uint32)
        check(self._L.pk_archive_read(self._h, ctypes.byref(used), *(ctypes.c_void_p(a.ctypes.data) for a in
                                                                    (keys, scores, lengths, visits, picks)),
                                      ctypes.byref(overflow)), "pk_archive_read")
        return {"used": int(used.value), "overflow": int(overflow.value), "keys": keys, "scores": scores,
                "lengths": lengths, "visits": visits, "picks": picks}

    # -- archive exchange (stream-ordered except enable) ----------------------------------
    # a packed cell: pk_xrec, 48 bytes (include/pokegym_amd.h); records travel as uint8 (k, 48) tensors
    XREC = np.dtype([("key", "<u8"), ("score", "<f8"), ("length", "<u4"), ("visits", "<u4"), ("picks", "<u4"),
                     ("payload", "<i4"), ("format", "<u4"), ("reserved", "<u4", (3,))])

    def archive_exchange_enable(self):
        """Let the archive pack its cells and merge those of other handles (pk_archive_exchange_enable;
        once, synchronous; needs archive_create)."""
        check(self._L.pk_archive_exchange_enable(self._h), "pk_archive_exchange_enable")

    @property
    def archive_payload_bytes(self) -> int:
        """Bytes of one payload (a whole slot), 0 before archive_exchange_enable."""
        return int(self._L.pk_archive_payload_bytes(self._h))

    @property
    def archive_format(self) -> int:
        """The payload layout this handle packs and accepts (pk_archive_format)."""
        return int(self._L.pk_archive_format(self._h))

    def archive_pack(self, delta: bool = False, cell0: int = 0, count: int | None = None, max_payloads: int | None = None):
        """Cells [cell0, cell0 + count) as (records, payloads, n_payloads) device tensors
        (pk_archive_pack, on the current stream): records uint8 (count, 48) — view them on the host
        with BatchedEmulator.XREC — payloads uint8 (max_payloads, archive_payload_bytes) and
        n_payloads an int32 scalar tensor, the rows written.  delta=False packs every cell in use
        with its full counts and changes nothing; delta=True packs what this handle counted since
        its last delta pack and ships only the cells whose record it replaced since (at most
        max_payloads of them, the rest with the next delta pack).  max_payloads defaults to count."""
        count = self.archive_cells - cell0 if count is None else int(count)
        max_payloads = count if max_payloads is None else int(max_payloads)
        records = torch.zeros((max(count, 1), self.XREC.itemsize), dtype=torch.uint8, device=self.device)
        payloads = torch.zeros((max_payloads, max(self.archive_payload_bytes, 16)), dtype=torch.uint8, device=self.device)
        n_payloads = torch.zeros((), dtype=torch.int32, device=self.device)
        check(self._L.pk_archive_pack(self._h, _native.PK_XCHG_DELTA if delta else 0, int(cell0), count, max_payloads,
                                      ctypes.c_void_p(records.data_ptr()),
                                      ctypes.c_void_p(payloads.data_ptr()) if max_payloads else None,
                                      ctypes.c_void_p(n_payloads.data_ptr()), self._stream()), "pk_archive_pack")
        return records[:count], payloads, n_payloads

    def archive_merge(self, records: torch.Tensor, payloads: torch.Tensor | None, out: torch.Tensor | None = None):
        """Merge packed cells into this archive (pk_archive_merge, on the current stream): records
        uint8 (k, 48), payloads uint8 (m, archive_payload_bytes) or None, both on this device; the
        winners' payloads are written into their cells' slots.  Returns out, int32 (k,): the cell
        each record won, -1 else."""
        if records.dtype != torch.uint8 or records.device != self.device or records.dim() != 2 \
                or records.shape[1] != self.XREC.itemsize or not records.is_contiguous():
            raise ValueError("records must be a contiguous uint8 (k, 48) tensor on the emulator's device")
        k = int(records.shape[0])
        m = 0
        if payloads is not None:
            m = int(payloads.shape[0])
            if payloads.dtype != torch.uint8 or payloads.device != self.device or not payloads.is_contiguous() \
                    or (m and payloads.shape[1] != self.archive_payload_bytes):
                raise ValueError("payloads must be a contiguous uint8 (m, archive_payload_bytes) tensor on the device")
        if out is None:
            out = torch.full((k,), -1, dtype=torch.int32, device=self.device)
        elif out.dtype != torch.int32 or out.device != self.device or out.numel() != k or not out.is_contiguous():
            raise ValueError("out must be a contiguous int32 tensor of one element per record on the device")
        if k == 0:
            return out
        check(self._L.pk_archive_merge(self._h, ctypes.c_void_p(records.data_ptr()), k,
                                       ctypes.c_void_p(payloads.data_ptr()) if m else None, m,
                                       ctypes.c_void_p(out.data_ptr()), self._stream()), "pk_archive_merge")
        return out

    # -- visit counts (stream-ordered except create / read; pack reads its length back) ----
    # a packed key: pk_crec {key, count}, 16 bytes; records travel as int64 (k, 2) tensors (the 64 key
    # bits as an int64, like every key tensor here)
    def counts_create(self, cap_log2: int):
        """Give the handle a visit-count table of 2**cap_log2 entries (pk_counts_create; once,
        synchronous; any handle).  It takes counts_limit distinct keys."""
        check(self._L.pk_counts_create(self._h, int(cap_log2)), "pk_counts_create")

    @property
    def counts_limit(self) -> int:
        """Distinct keys the table takes, 3/4 of its entries; 0 without a table."""
        return int(self._L.pk_counts_limit(self._h))

    def counts_update(self, keys: torch.Tensor, mask: torch.Tensor | None = None, env0: int = 0, count: int | None = None,
                      beta: float = 1.0, peek: bool = False, counts_out: torch.Tensor | None = None,
                      bonus_out: torch.Tensor | None = None):
        """Count the keys (int64: the 64 key bits; -1 is the reserved "no key") of the envs of the
        range with mask[e] != 0 and return (counts_out, bonus_out): each env's key's new count (int64)
        and beta / sqrt(count) (float64), 0 for envs that take no part or find the table full
        (pk_counts_update, on the current stream; full-size tensors, the rest of the outputs is
        untouched).  peek=True counts nothing and returns the stored counts."""
        count = self.n - env0 if count is None else count
        if counts_out is None:
            counts_out = torch.zeros(self.n, dtype=torch.int64, device=self.device)
        if bonus_out is None:
            bonus_out = torch.zeros(self.n, dtype=torch.float64, device=self.device)
        check(self._L.pk_counts_update(self._h, self._full(keys, torch.int64, "keys"), self._full(mask, torch.uint8, "mask"),
                                       env0, count, float(beta), _native.PK_COUNTS_PEEK if peek else 0,
                                       self._full(counts_out, torch.int64, "counts_out"),
                                       self._full(bonus_out, torch.float64, "bonus_out"), self._stream()), "pk_counts_update")
        return counts_out, bonus_out

    def _crecs(self, records: torch.Tensor):
        if records.dtype != torch.int64 or records.device != self.device or records.dim() != 2 \
                or records.shape[1] != 2 or not records.is_contiguous() or records.data_ptr() % 16:
            raise ValueError("records must be a contiguous, 16-byte aligned int64 (k, 2) tensor on the emulator's device")
        return ctypes.c_void_p(records.data_ptr())

    def counts_add(self, records: torch.Tensor, foreign: bool = False):
        """Add packed counts, int64 (k, 2) rows of key and count, to the table (pk_counts_add, on the
        current stream).  foreign=True: they came from another handle and are never sent on by a
        delta pack of this one."""
        p = self._crecs(records)
        if records.shape[0]:
            check(self._L.pk_counts_add(self._h, p, int(records.shape[0]), _native.PK_COUNTS_FOREIGN if foreign else 0,
                                        self._stream()), "pk_counts_add")

    def counts_pack_raw(self, delta: bool = False):
        """(records, n): an int64 (counts_limit, 2) tensor whose first n rows (n an int32 scalar tensor)
        are the packed keys, in no order (pk_counts_pack, on the current stream; no host sync)."""
        limit = self.counts_limit
        records = torch.empty((max(limit, 1), 2), dtype=torch.int64, device=self.device)
        n = torch.zeros((), dtype=torch.int32, device=self.device)
        check(self._L.pk_counts_pack(self._h, _native.PK_COUNTS_DELTA if delta else 0, self._crecs(records), limit,
                                     ctypes.c_void_p(n.data_ptr()), self._stream()), "pk_counts_pack")
        return records, n

    def counts_pack(self, delta: bool = False) -> torch.Tensor:
        """The table as int64 (k, 2) device rows of key and count, sorted by key as an unsigned number:
        every stored key, or with delta=True what this handle counted itself since its last delta
        pack (the keys it counted nothing for are left out).  Reads k back (a host sync)."""
        records, n = self.counts_pack_raw(delta)
        records = records[:int(n)]
        order = torch.argsort(records[:, 0] ^ torch.iinfo(torch.int64).min)
        return records[order].contiguous()

    def counts_read(self) -> dict:
        """{"used": distinct keys stored, "overflow": keys a full table turned away} (pk_counts_read;
        synchronous)."""
        used, overflow = ctypes.c_uint64(), ctypes.c_uint64()
        check(self._L.pk_counts_read(self._h, ctypes.byref(used), ctypes.byref(overflow)), "pk_counts_read")
        return {"used": int(used.value), "overflow": int(overflow.value)}

    def counts_clear(self):
        """Empty the table (pk_counts_clear, on the current stream)."""
        check(self._L.pk_counts_clear(self._h, self._stream()), "pk_counts_clear")

    # -- frame stack (stream-ordered except create) ----------------------------------------
    def stack_create(self, scale: int = 2, depth: int = 4, layout: str = "chw", mode: str = "mean"):
        """Give the handle a frame stack: per env `depth` frames downscaled by `scale` (1, 2, 4), newest
        first, uint8 (n, depth, 144 / scale, 160 / scale) for layout "chw" or (n, 144 / scale,
        160 / scale, depth) for "hwc" (depth 1, 2, 4, 8); mode "mean" averages a scale x scale block,
        "pick" takes its top left pixel (pk_fstack_create; once, synchronous; any handle).  `stack`
        is the tensor, all zeros until the first stack_push."""
        shape = stack_shape(scale, depth, layout)
        if mode not in ("mean", "pick"):
            raise ValueError("stack mode must be 'mean' or 'pick'")
        check(self._L.pk_fstack_create(self._h, int(scale), int(depth),
                                       _native.PK_FSTACK_HWC if layout == "hwc" else _native.PK_FSTACK_CHW,
                                       _native.PK_FSTACK_PICK if mode == "pick" else _native.PK_FSTACK_MEAN), "pk_fstack_create")
        self._stack = self._view(self._L.pk_fstack_ptr(self._h), (self.n,) + shape, "|u1")

    @property
    def stack(self) -> torch.Tensor | None:
        """The frame stack, a view of the handle's buffer (pk_fstack_ptr); None without stack_create."""
        return getattr(self, "_stack", None)

    def stack_push(self, mask: torch.Tensor | None = None, fill_only: bool = False, screen: torch.Tensor | None = None,
                   env0: int = 0, count: int | None = None):
        """Push the current frame of the envs of the range onto their stacks, in place and in one
        launch (pk_fstack_push, on the current stream).  mask: a full-size uint8 (n,) tensor; an env
        with mask[e] != 0 is filled — all its planes become the new frame — the others are pushed.
        fill_only=True touches only the envs with mask[e] != 0 (no mask: the whole range) and fills
        them.  screen: a uint8 (n, 144, 160) tensor to read in the place of the emulator's own
        screen (which needs render=True).  Returns `stack`."""
        count = self.n - env0 if count is None else count
        sp = None
        if screen is not None:
            if (screen.dtype != torch.uint8 or screen.device != self.device or tuple(screen.shape) != (self.n, ROWS, COLS)
                    or not screen.is_contiguous()):
                raise ValueError("screen must be a contiguous uint8 (n_envs, 144, 160) tensor on the emulator's device")
            sp = ctypes.c_void_p(screen.data_ptr())
        check(self._L.pk_fstack_push(self._h, sp, self._full(mask, torch.uint8, "mask"),
                                     _native.PK_FSTACK_FILL_ONLY if fill_only else 0, env0, count, self._stream()),
              "pk_fstack_push")
        return self.stack

    # -- RAM probes (stream-ordered except create) -----------------------------------------
    def probes_create(self, program):
        """Give the handle a probe program: a list of probes.Probe records (pk_probe_create; once,
        synchronous; any handle).  A program the header's rules reject raises ValueError."""
        from . import probes
        try:
            arr = probes.pack(program)
        except TypeError as e:
            raise ValueError(str(e)) from None
        check(self._L.pk_probe_create(self._h, arr, len(arr)), "pk_probe_create")
        self.probe_program = list(program)

    @property
    def probe_count(self) -> int:
        """The probes of the handle's program (pk_probe_count); 0 without probes_create."""
        return int(self._L.pk_probe_count(self._h))

    def probes_eval(self, mask: torch.Tensor | None = None, rebase_only: bool = False, set: bool = False,
                    rewards: torch.Tensor | None = None, terminals: torch.Tensor | None = None,
                    features: torch.Tensor | None = None, env0: int = 0, count: int | None = None):
        """Evaluate the program for the envs of the range in one launch (pk_probe_eval, on the current
        stream).  mask: a full-size uint8 (n,) tensor; an env with mask[e] != 0 rebases — its state
        takes the current values, its outputs stay — the others evaluate: rewards[e] += r and
        terminals[e] |= done, or = with set=True.  rebase_only=True touches only the envs with
        mask[e] != 0 (no mask: the whole range) and rebases them.  rewards float64 (n,), terminals
        uint8 (n,) and features int32 (n, m) are full-size tensors on the device, each optional;
        features takes the values of every env that took part."""
        count = self.n - env0 if count is None else count
        fp = None
        if features is not None:
            if (features.dtype != torch.int32 or features.device != self.device or not features.is_contiguous()
                    or tuple(features.shape) != (self.n, self.probe_count)):
                raise ValueError("features must be a contiguous int32 (n_envs, probe_count) tensor on the emulator's device")
            fp = ctypes.c_void_p(features.data_ptr())
        flags = (_native.PK_PROBE_REBASE_ONLY if rebase_only else 0) | (_native.PK_PROBE_SET if set else 0)
        check(self._L.pk_probe_eval(self._h, self._full(mask, torch.uint8, "mask"), flags, env0, count,
                                    self._full(rewards, torch.float64, "rewards"),
                                    self._full(terminals, torch.uint8, "terminals"), fp, self._stream()), "pk_probe_eval")

    # -- tile view (stream-ordered except create) ------------------------------------------
    def tiles_create(self, mode: str = "id", bits: int = 12, objects: bool = True):
        """Give the handle a tile view: per env the screen as 18 x 20 tile ids (mode "id") or `bits`-bit
        hashes of the tiles' data (mode "hash", bits 8..15), with objects=True a second plane of object
        tiles (pk_tiles_create; once, synchronous; any handle, render=False included).  `tiles` is the
        tensor, all -1 ("nothing", 0xFFFF) until the first tiles_eval."""
        if mode not in ("id", "hash"):
            raise ValueError('tile view mode must be "id" or "hash"')
        check(self._L.pk_tiles_create(self._h, _native.PK_TILES_HASH if mode == "hash" else _native.PK_TILES_ID, int(bits),
                                      _native.PK_TILES_OBJ if objects else 0), "pk_tiles_create")
        self._tiles = self._view(self._L.pk_tiles_ptr(self._h),
                                 (self.n, self.tile_planes, _native.TILE_ROWS, _native.TILE_COLS), "<i2")

    @property
    def tile_planes(self) -> int:
        """Planes of the tile view (pk_tiles_planes): 1, 2 with objects, 0 without tiles_create."""
        return int(self._L.pk_tiles_planes(self._h))

    @property
    def tiles(self) -> torch.Tensor | None:
        """The tile view, an int16 (n, P, 18, 20) view of the handle's buffer (pk_tiles_ptr; the u16
        values as int16, so "nothing" is -1); None without tiles_create."""
        return getattr(self, "_tiles", None)

    def tiles_eval(self, mask: torch.Tensor | None = None, salt: torch.Tensor | None = None,
                   keys: torch.Tensor | None = None, env0: int = 0, count: int | None = None):
        """Evaluate the tile view of the envs of the range in one launch (pk_tiles_eval, on the current
        stream).  mask: a full-size uint8 (n,) tensor; only the envs with mask[e] != 0 are written (no
        mask: the whole range).  keys: an int64 (n,) tensor that receives the 64-bit key of each
        written env's view, salt: int64 (n,) words mixed into the keys (`keys` itself will do; a salt
        of -1, "no cell", stays -1).  Returns `tiles`."""
        count = self.n - env0 if count is None else count
        check(self._L.pk_tiles_eval(self._h, self._full(mask, torch.uint8, "mask"), self._full(salt, torch.int64, "salt"),
                                    self._full(keys, torch.int64, "keys"), env0, count, self._stream()), "pk_tiles_eval")
        return self.tiles

    # -- action trajectories (stream-ordered except enable) -------------------------------
    def traj_enable(self):
        """Record every env's actions from here on (pk_traj_enable; once, synchronous).  Call it
        before the first step: an env that has already stepped is flagged PK_TRAJ_BROKEN until
        its next reloading reset."""
        check(self._L.pk_traj_enable(self._h), "pk_traj_enable")

    @property
    def traj_capacity(self) -> int:
        """Bytes of a trajectory row, 0 without trajectories."""
        return int(self._L.pk_traj_capacity(self._h))

    def _traj_read(self, fn, what: str, first: int, count: int, rows: int, lo: int):
        origin = torch.full((rows,), -1, dtype=torch.int32, device=self.device)
        length = torch.zeros(rows, dtype=torch.int32, device=self.device)
        flags = torch.zeros(rows, dtype=torch.uint8, device=self.device)
        actions = torch.full((rows, max(self.traj_capacity, 1)), 0xFF, dtype=torch.uint8, device=self.device)
        check(fn(self._h, first, count, *(ctypes.c_void_p(t.data_ptr()) for t in (origin, length, flags, actions)),
                 self._stream()), what)
        sl = slice(lo, lo + count)
        return {"origin": origin[sl], "length": length[sl], "flags": flags[sl], "actions": actions[sl]}

    def trajectories(self, env0: int = 0, count: int | None = None) -> dict:
        """The trajectories of envs [env0, env0 + count) (pk_traj_get, on the current stream; the
        range follows step_range's rule) as device tensors over the range: origin int32 (the slot
        the episode started from, -1 = the template), length int32, flags uint8 (PK_TRAJ_*) and
        actions uint8 (count, traj_capacity), 0xFF from the length on."""
        count = self.n - env0 if count is None else count
        return self._traj_read(self._L.pk_traj_get, "pk_traj_get", env0, count, self.n, env0)

    def bank_trajectories(self, slot0: int, count: int) -> dict:
        """The trajectory parts of bank slots [slot0, slot0 + count) (pk_bank_traj_get), as
        trajectories() returns them; a slot without an episode has flags PK_TRAJ_EMPTY."""
        return self._traj_read(self._L.pk_bank_traj_get, "pk_bank_traj_get", slot0, count, max(int(count), 1), 0)

    def replay(self, origins, actions, lengths, slots_out, flags=None, envs=None):
        """Rebuild episodes from their trajectories: trajectory i (origin origins[i], the first
        lengths[i] bytes of actions[i]) is replayed on env envs[i] (default: env i) and checkpointed
        into bank slot slots_out[i] right after its last action — at length 0 right after the reset.
        The slot then holds the machine state and the episode bookkeeping the recorded env had.

        The listed envs are reset from their origins (-1 = the template), so this handle's bank
        must hold the origin slots with the content the recording handle's had; then EVERY env of
        the handle is stepped max(lengths) times, finished and unlisted envs with action 8 (no
        button) — use a handle of its own.  Needs traj_enable() and bank_enable_episodes() on
        this handle.  Raises ValueError for a trajectory with flags (broken or overflowed), and —
        after the reset — when the reset did not reload the machine (reward=True without
        reload_on_reset and the env had been reset before) or an origin slot was rejected.
        Synchronous (it reads the reset's result back)."""
        origins = np.asarray(origins, np.int32).reshape(-1)
        lengths = np.asarray(lengths, np.int64).reshape(-1)
        slots_out = np.asarray(slots_out, np.int32).reshape(-1)
        k = len(origins)
        envs = np.arange(k) if envs is None else np.asarray(envs, np.int64).reshape(-1)
        if not (len(lengths) == len(slots_out) == len(envs) == len(actions) == k):
            raise ValueError("replay: origins, actions, lengths, slots_out and envs must have one entry per trajectory")
        if flags is not None and np.asarray(flags).reshape(-1).any():
            raise ValueError("replay: a trajectory is flagged broken or overflowed; its actions do not determine its state")
        if k == 0:
            return
        if len(set(envs.tolist())) != k or envs.min() < 0 or envs.max() >= self.n:
            raise ValueError("replay: envs must be distinct env indices of this handle")
        if not self.traj_capacity:
            raise ValueError("replay: the handle needs traj_enable() to verify its resets")
        steps = int(lengths.max())
        acts = np.full((steps, self.n), 8, np.uint8)
        for i in range(k):
            a = np.asarray(actions[i].cpu() if isinstance(actions[i], torch.Tensor) else actions[i], np.uint8).reshape(-1)
            if lengths[i] < 0 or lengths[i] > len(a):
                raise ValueError(f"replay: trajectory {i} has fewer than {lengths[i]} actions")
            acts[:lengths[i], envs[i]] = a[:lengths[i]]

        def per_env(values, fill, dtype, which=slice(None)):
            full = np.full(self.n, fill, dtype)
            full[envs[which]] = values
            return torch.from_numpy(full).to(self.device)

        mask = per_env(1, 0, np.uint8)
        if (origins >= 0).any():
            self.reset_from(per_env(origins, -1, np.int32), mask)
        else:
            self.reset(mask)
        got = self.trajectories()
        got_flags, got_origin = got["flags"].cpu().numpy()[envs], got["origin"].cpu().numpy()[envs]
        if got_flags.any():
            raise ValueError("replay: the resets of this handle do not reload the machine (reward=True without "
                             "reload_on_reset, envs already reset): nothing to replay from")
        if (got_origin != origins).any():
            raise ValueError("replay: an origin slot is empty or out of range on this handle")
        acts = torch.from_numpy(acts).to(self.device)
        for t in range(steps + 1):
            at = np.nonzero(lengths == t)[0]
            if len(at):
                self.bank_checkpoint(per_env(slots_out[at], -1, np.int32, at))
            if t < steps:
                self.step(acts[t])

    def set_episode_params(self, max_episode_steps: int, reward_scale: float):
        """Episode length and reward scale of the following steps (Environment.reset's arguments,
        environment.py:1233, :1258-1259); call before the reset they belong to."""
        check(self._L.pk_set_episode_params(self._h, int(max_episode_steps), float(reward_scale)), "pk_set_episode_params")
        self.max_episode_steps, self.reward_scale = int(max_episode_steps), float(reward_scale)

    def raise_if_failed(self, env: int | None = None):
        """Raise the exception the reference would have raised for a failed env (PK_ERR_*)."""
        if self.errors is None:
            return
        err = self.errors if env is None else self.errors[env:env + 1]
        bad = torch.nonzero(err).flatten()
        if bad.numel():
            e = int(bad[0]) + (0 if env is None else env)
            code = int(self.errors[e])
            raise ERR_EXCEPTIONS.get(code, RuntimeError)(f"env {e}: reference reward stack raises here (PK_ERR {code})")

    def info_dicts(self, envs=None) -> dict:
        """{env: info dict} for the envs whose last step built one (host sync; environment.py:1621-1704)."""
        if self.info_flag is None:
            return {}
        flag = self.info_flag if envs is None else self.info_flag[envs]
        ids = torch.nonzero(flag).flatten()
        if envs is not None:
            ids = torch.as_tensor(envs, device=self.device).reshape(-1)[ids]
        if not ids.numel():
            return {}
        rec = self.info[:, ids].t().cpu().numpy()
        bits = (self.info_bits[:, ids].t().cpu().numpy().astype(np.int64) & 0xFFFFFFFF)
        return {int(e): {**info_dict(r), **event_dicts(b)} for e, r, b in zip(ids.tolist(), rec, bits)}

    # -- bulk RAM views (stream-ordered) ------------------------------------------------
    def get_ram(self, addr: int, length: int, out: torch.Tensor | None = None) -> torch.Tensor:
        if out is None:
            out = torch.empty((self.n, length), dtype=torch.uint8, device=self.device)
        check(self._L.pk_get_ram(self._h, addr, length, ctypes.c_void_p(out.data_ptr()), self._stream()), "pk_get_ram")
        return out

    def set_ram(self, addr: int, data: torch.Tensor):
        data = data.to(device=self.device, dtype=torch.uint8).contiguous()
        length = data.numel() // self.n
        check(self._L.pk_set_ram(self._h, addr, length, ctypes.c_void_p(data.data_ptr()), self._stream()), "pk_set_ram")

    # -- host-side accessors (synchronous) --------------------------------------------
    def snapshot(self, env: int) -> bytes:
        out = np.zeros(STATE_V9_BYTES, np.uint8)
        check(self._L.pk_snapshot(self._h, env, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), len(out)),
              "pk_snapshot")
        return out.tobytes()

    def snapshot_range(self, env0: int, count: int) -> np.ndarray:
        """v9 savestates of envs [env0, env0 + count) as a (count, 142610) uint8 array (bulk pk_snapshot)."""
        out = np.zeros((count, STATE_V9_BYTES), np.uint8)
        check(self._L.pk_snapshot_range(self._h, env0, count, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                        out.size), "pk_snapshot_range")
        return out

    def render_latched(self):
        """Rasterise every env's latched scanlines into `screen` (K2 over a loaded state)."""
        check(self._L.pk_render_latched(self._h, self._stream()), "pk_render_latched")
        return self.screen

    def load_env(self, env: int, state: bytes):
        a, p = _u8p(state)
        check(self._L.pk_load_env(self._h, env, p, len(a)), "pk_load_env")

    def peek(self, env: int, addr: int, n: int = 1) -> bytes:
        out = np.zeros(n, np.uint8)
        check(self._L.pk_peek(self._h, env, addr, n, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))), "pk_peek")
        return out.tobytes()

    def poke(self, env: int, addr: int, data: bytes):
        a, p = _u8p(data)
        check(self._L.pk_poke(self._h, env, addr, len(a), p), "pk_poke")

    def last_instr_count(self) -> int:
        v = ctypes.c_uint64()
        check(self._L.pk_last_instr_count(self._h, ctypes.byref(v)), "pk_last_instr_count")
        return int(v.value)

    def launch_shape(self, env0: int = 0, count: int | None = None) -> dict:
        """The K1 launch pk_step_range(env0, count) takes (pk_launch_shape; host-side, no GPU work)."""
        out = (ctypes.c_uint32 * 5)()
        count = self.n - env0 if count is None else count
        check(self._L.pk_launch_shape(self._h, env0, count, out), "pk_launch_shape")
        return {"small": bool(out[0]), "wave_lanes": int(out[1]), "block": int(out[2]), "prio": bool(out[3]),
                "all_staged": bool(out[4])}

    def profile_enable(self, on: bool = True):
        check(self._L.pk_profile_enable(self._h, 1 if on else 0), "pk_profile_enable")

    def profile_read(self):
        """(emulate_ms, render_ms, reward_ms, steps) summed since the last read (synchronous)."""
        a, b, c, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_uint64()
        check(self._L.pk_profile_read(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(n)),
              "pk_profile_read")
        return a.value, b.value, c.value, int(n.value)

    def close(self):
        if getattr(self, "_h", None):
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
            self.screen = None
            self.obs = None
            self.errors = None
            self.info = self.info_flag = self.heatmap = self.info_bits = None
            self._stack = None
            self._tiles = None
            self._L.pk_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass
