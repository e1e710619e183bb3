"""ctypes binding of the C ABI in include/pokegym_amd.h (libpokegym_amd.so, built in-tree).

This is the reference-side binding a maintainer would add.  There is no
CPU fallback: if the HIP library is missing or fails to load, every entry point raises.
"""
from __future__ import annotations

import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# PK_LIB selects an alternative in-tree build (A/B kernel experiments); default: lib/libpokegym_amd.so
LIB_PATH = os.environ.get("PK_LIB") or os.path.join(HERE, "lib", "libpokegym_amd.so")

ABI_VERSION = 12
PK_F_RENDER = 1
PK_F_REWARD = 2
PK_F_RELOAD_ON_RESET = 4
PK_F_HEATMAP = 8
PK_TRAJ_BROKEN = 1
PK_TRAJ_OVERFLOW = 2
PK_TRAJ_EMPTY = 4
PK_XCHG_DELTA = 1
PK_COUNTS_PEEK = 1
PK_COUNTS_FOREIGN = 1
PK_COUNTS_DELTA = 1
PK_FSTACK_CHW, PK_FSTACK_HWC = 0, 1
PK_FSTACK_MEAN, PK_FSTACK_PICK = 0, 1
PK_FSTACK_FILL_ONLY = 1
PK_PV_LE, PK_PV_BE, PK_PV_BCD, PK_PV_BITS = 0, 1, 2, 3
PK_PR_SUM, PK_PR_MAX = 0, 1
PK_PO_NONE, PK_PO_DELTA, PK_PO_NEWMAX, PK_PO_CHANGE = 0, 1, 2, 3
PK_PC_NONE, PK_PC_EQ, PK_PC_NE, PK_PC_GE, PK_PC_LE = 0, 1, 2, 3, 4
PK_PROBE_REBASE_ONLY, PK_PROBE_SET = 1, 2
PK_PROBE_MAX = 64
PK_GEP_PROBES, PK_GEP_STACK = 1, 2
PK_TILES_ID, PK_TILES_HASH = 0, 1
PK_TILES_OBJ = 1
TILE_ROWS, TILE_COLS = 18, 20
HEAT_SHAPE = (444, 436)
OBS_SHAPE = (72, 80, 4)
# PK_ERR_* -> the exception the reference raises at that point (include/pokegym_amd.h)
ERR_EXCEPTIONS = {1: KeyError, 2: AttributeError, 3: IndexError, 4: UnboundLocalError, 5: IndexError,
                  6: IndexError, 7: MemoryError, 8: ValueError}
STATE_V9_BYTES = 142610
ROWS, COLS = 144, 160

# the exported symbols declared in include/pokegym_amd.h
EXPORTS = ("pk_create", "pk_destroy", "pk_last_error", "pk_abi_version", "pk_reset", "pk_step",
           "pk_screen_ptr", "pk_num_envs", "pk_peek", "pk_poke", "pk_snapshot", "pk_load_env",
           "pk_last_instr_count", "pk_profile_enable", "pk_profile_read", "pk_obs_ptr", "pk_error_ptr",
           "pk_get_ram", "pk_set_ram", "pk_info_ptr", "pk_info_flag_ptr", "pk_info_stride", "pk_heatmap_ptr", "pk_info_bits_ptr",
           "pk_snapshot_range", "pk_render_latched", "pk_step_range", "pk_reset_range",
           "pk_set_episode_params", "pk_launch_shape",
           "pk_bank_create", "pk_bank_slots", "pk_bank_put", "pk_bank_get", "pk_bank_save", "pk_bank_load",
           "pk_reset_from", "pk_bank_rejects",
           "pk_bank_enable_episodes", "pk_bank_has_episodes", "pk_bank_checkpoint", "pk_bank_resume",
           "pk_archive_create", "pk_archive_cells", "pk_cell_keys", "pk_archive_update", "pk_archive_explore",
           "pk_archive_read",
           "pk_traj_enable", "pk_traj_capacity", "pk_traj_get", "pk_bank_traj_get",
           "pk_archive_exchange_enable", "pk_archive_payload_bytes", "pk_archive_format", "pk_archive_pack",
           "pk_archive_merge",
           "pk_frame_cells", "pk_frame_keys",
           "pk_counts_create", "pk_counts_limit", "pk_counts_update", "pk_counts_add", "pk_counts_pack",
           "pk_counts_read", "pk_counts_clear",
           "pk_fstack_create", "pk_fstack_depth", "pk_fstack_scale", "pk_fstack_ptr", "pk_fstack_push",
           "pk_probe_create", "pk_probe_count", "pk_probe_eval",
           "pk_bank_enable_generic_episodes", "pk_bank_generic_parts", "pk_bank_generic_episode_bytes",
           "pk_tiles_create", "pk_tiles_planes", "pk_tiles_ptr", "pk_tiles_eval")


class PkConfig(ctypes.Structure):
    _fields_ = [
        ("n_envs", ctypes.c_uint32),
        ("device", ctypes.c_int32),
        ("rom", ctypes.POINTER(ctypes.c_uint8)),
        ("rom_len", ctypes.c_uint64),
        ("state", ctypes.POINTER(ctypes.c_uint8)),
        ("state_len", ctypes.c_uint64),
        ("frame_skip", ctypes.c_uint32),
        ("release_frame", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("max_episode_steps", ctypes.c_uint32),
        ("reward_scale", ctypes.c_double),
    ]


class PkXrec(ctypes.Structure):
    """pk_xrec: one cell of a packed archive (48 bytes)."""
    _fields_ = [
        ("key", ctypes.c_uint64),
        ("score", ctypes.c_double),
        ("length", ctypes.c_uint32),
        ("visits", ctypes.c_uint32),
        ("picks", ctypes.c_uint32),
        ("payload", ctypes.c_int32),
        ("format", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32 * 3),
    ]


class PkProbe(ctypes.Structure):
    """pk_probe: one probe of a RAM probe program (24 bytes)."""
    _fields_ = [
        ("addr", ctypes.c_uint16),
        ("len", ctypes.c_uint16),
        ("count", ctypes.c_uint16),
        ("stride", ctypes.c_uint16),
        ("kind", ctypes.c_uint8),
        ("reduce", ctypes.c_uint8),
        ("op", ctypes.c_uint8),
        ("cmp", ctypes.c_uint8),
        ("arg", ctypes.c_uint32),
        ("weight", ctypes.c_double),
    ]


class PkError(RuntimeError):
    pass


_lib = None


def load(path: str = LIB_PATH):
    """Load the HIP library; raise loudly if it is absent (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise PkError(f"{path} not found: build it with `python -m pokegym_amd.build` "
                      "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = ctypes.CDLL(path)
    bind(L)
    _lib = L
    return L


def bind(L):
    """argtypes of every entry point of include/pokegym_amd.h (shared with the host-simulation
    test build, tests/hostsim)."""
    u8p = ctypes.POINTER(ctypes.c_uint8)
    vp = ctypes.c_void_p
    L.pk_create.argtypes = [ctypes.POINTER(PkConfig), ctypes.POINTER(vp)]
    L.pk_destroy.argtypes = [vp]
    L.pk_destroy.restype = None
    L.pk_last_error.restype = ctypes.c_char_p
    L.pk_reset.argtypes = [vp, vp, vp]
    L.pk_step.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.pk_screen_ptr.argtypes = [vp]
    L.pk_screen_ptr.restype = vp
    L.pk_num_envs.argtypes = [vp]
    L.pk_num_envs.restype = ctypes.c_uint32
    L.pk_peek.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint16, ctypes.c_uint32, u8p]
    L.pk_poke.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint16, ctypes.c_uint32, u8p]
    L.pk_snapshot.argtypes = [vp, ctypes.c_uint32, u8p, ctypes.c_uint64]
    L.pk_load_env.argtypes = [vp, ctypes.c_uint32, u8p, ctypes.c_uint64]
    L.pk_snapshot_range.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, u8p, ctypes.c_uint64]
    L.pk_render_latched.argtypes = [vp, vp]
    L.pk_last_instr_count.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    L.pk_launch_shape.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
    L.pk_profile_enable.argtypes = [vp, ctypes.c_int]
    dp = ctypes.POINTER(ctypes.c_double)
    L.pk_profile_read.argtypes = [vp, dp, dp, dp, ctypes.POINTER(ctypes.c_uint64)]
    bind_v2(L)
    bind_v7(L)
    bind_v8(L)
    bind_v9(L)
    bind_v10(L)
    bind_v11(L)
    bind_v12(L)
    bind_counts(L)
    bind_fstack(L)
    bind_probes(L)
    bind_generic(L)
    bind_tiles(L)


def bind_v2(L):
    """argtypes of the ABI-v2 entry points (shared with the host-simulation test build)."""
    vp = ctypes.c_void_p
    L.pk_obs_ptr.argtypes = [vp]
    L.pk_obs_ptr.restype = vp
    L.pk_error_ptr.argtypes = [vp]
    L.pk_error_ptr.restype = vp
    L.pk_info_ptr.argtypes = [vp]
    L.pk_info_ptr.restype = vp
    L.pk_info_flag_ptr.argtypes = [vp]
    L.pk_info_flag_ptr.restype = vp
    L.pk_info_stride.argtypes = [vp]
    L.pk_info_stride.restype = ctypes.c_uint32
    L.pk_heatmap_ptr.argtypes = [vp]
    L.pk_heatmap_ptr.restype = vp
    L.pk_info_bits_ptr.argtypes = [vp]
    L.pk_info_bits_ptr.restype = vp
    L.pk_get_ram.argtypes = [vp, ctypes.c_uint16, ctypes.c_uint32, vp, vp]
    L.pk_set_ram.argtypes = [vp, ctypes.c_uint16, ctypes.c_uint32, vp, vp]
    L.pk_reset.argtypes = [vp, vp, vp]
    L.pk_step_range.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp, vp, vp]
    L.pk_reset_range.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp]
    L.pk_set_episode_params.argtypes = [vp, ctypes.c_uint32, ctypes.c_double]


def bind_v7(L):
    """argtypes of the savestate bank (ABI v7; shared with the host-simulation test build)."""
    vp = ctypes.c_void_p
    u32 = ctypes.c_uint32
    u8p = ctypes.POINTER(ctypes.c_uint8)
    L.pk_bank_create.argtypes = [vp, u32]
    L.pk_bank_slots.argtypes = [vp]
    L.pk_bank_slots.restype = u32
    L.pk_bank_put.argtypes = [vp, u32, u8p, ctypes.c_uint64]
    L.pk_bank_get.argtypes = [vp, u32, u8p, ctypes.c_uint64]
    L.pk_bank_save.argtypes = [vp, vp, u32, u32, vp]
    L.pk_bank_load.argtypes = [vp, vp, u32, u32, vp]
    L.pk_reset_from.argtypes = [vp, u32, u32, vp, vp, vp]
    L.pk_bank_rejects.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]


def bind_v8(L):
    """argtypes of the episode checkpoints (ABI v8; shared with the host-simulation test build)."""
    vp = ctypes.c_void_p
    u32 = ctypes.c_uint32
    L.pk_bank_enable_episodes.argtypes = [vp]
    L.pk_bank_has_episodes.argtypes = [vp]
    L.pk_bank_checkpoint.argtypes = [vp, vp, u32, u32, vp]
    L.pk_bank_resume.argtypes = [vp, vp, u32, u32, vp]


def bind_v9(L):
    """argtypes of the exploration archive (ABI v9; shared with the host-simulation test build)."""
    vp = ctypes.c_void_p
    u32 = ctypes.c_uint32
    L.pk_archive_create.argtypes = [vp, u32, u32, ctypes.c_uint64]
    L.pk_archive_cells.argtypes = [vp]
    L.pk_archive_cells.restype = u32
    L.pk_cell_keys.argtypes = [vp, u32, vp, u32, u32, vp]
    L.pk_archive_update.argtypes = [vp, vp, vp, vp, u32, u32, vp, vp]
    L.pk_archive_explore.argtypes = [vp, vp, u32, u32, vp, vp]
    L.pk_archive_read.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]


def bind_v10(L):
    """argtypes of the action trajectories (ABI v10; shared with the host-simulation test build)."""
    vp = ctypes.c_void_p
    u32 = ctypes.c_uint32
    L.pk_traj_enable.argtypes = [vp]
    L.pk_traj_capacity.argtypes = [vp]
    L.pk_traj_capacity.restype = u32
    L.pk_traj_get.argtypes = [vp, u32, u32, vp, vp, vp, vp, vp]
    L.pk_bank_traj_get.argtypes = [vp, u32, u32, vp, vp, vp, vp, vp]


def bind_v11(L):
    """argtypes of the archive exchange (ABI v11; shared with the host-simulation test build)."""
    vp = ctypes.c_void_p
    u32 = ctypes.c_uint32
    L.pk_archive_exchange_enable.argtypes = [vp]
    L.pk_archive_payload_bytes.argtypes = [vp]
    L.pk_archive_payload_bytes.restype = ctypes.c_uint64
    L.pk_archive_format.argtypes = [vp]
    L.pk_archive_format.restype = u32
    L.pk_archive_pack.argtypes = [vp, u32, u32, u32, u32, vp, vp, vp, vp]
    L.pk_archive_merge.argtypes = [vp, vp, u32, vp, u32, vp, vp]


def bind_v12(L):
    """argtypes of the frame cells (ABI v12; shared with the host-simulation test build)."""
    vp = ctypes.c_void_p
    u32 = ctypes.c_uint32
    L.pk_frame_cells.argtypes = [u32, u32]
    L.pk_frame_cells.restype = u32
    L.pk_frame_keys.argtypes = [vp, u32, u32, u32, vp, vp, vp, vp, u32, u32, vp]


def bind_counts(L):
    """argtypes of the visit counts (additive to ABI v12; shared with the host-simulation test build)."""
    vp = ctypes.c_void_p
    u32 = ctypes.c_uint32
    u64 = ctypes.c_uint64
    L.pk_counts_create.argtypes = [vp, u32]
    L.pk_counts_limit.argtypes = [vp]
    L.pk_counts_limit.restype = u64
    L.pk_counts_update.argtypes = [vp, vp, vp, u32, u32, ctypes.c_double, u32, vp, vp, vp]
    L.pk_counts_add.argtypes = [vp, vp, u32, u32, vp]
    L.pk_counts_pack.argtypes = [vp, u32, vp, u64, vp, vp]
    L.pk_counts_read.argtypes = [vp, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    L.pk_counts_clear.argtypes = [vp, vp]


def bind_fstack(L):
    """argtypes of the frame stack (additive to ABI v12; shared with the host-simulation test build)."""
    vp = ctypes.c_void_p
    u32 = ctypes.c_uint32
    L.pk_fstack_create.argtypes = [vp, u32, u32, u32, u32]
    L.pk_fstack_depth.argtypes = [vp]
    L.pk_fstack_depth.restype = u32
    L.pk_fstack_scale.argtypes = [vp]
    L.pk_fstack_scale.restype = u32
    L.pk_fstack_ptr.argtypes = [vp]
    L.pk_fstack_ptr.restype = vp
    L.pk_fstack_push.argtypes = [vp, vp, vp, u32, u32, u32, vp]


def bind_probes(L):
    """argtypes of the RAM probes (additive to ABI v12; shared with the host-simulation test build)."""
    vp = ctypes.c_void_p
    u32 = ctypes.c_uint32
    L.pk_probe_create.argtypes = [vp, ctypes.POINTER(PkProbe), u32]
    L.pk_probe_count.argtypes = [vp]
    L.pk_probe_count.restype = u32
    L.pk_probe_eval.argtypes = [vp, vp, u32, u32, u32, vp, vp, vp, vp]


def bind_generic(L):
    """argtypes of the generic episode parts (additive to ABI v12; shared with the host-simulation test build)."""
    vp = ctypes.c_void_p
    L.pk_bank_enable_generic_episodes.argtypes = [vp, ctypes.c_uint32]
    L.pk_bank_generic_parts.argtypes = [vp]
    L.pk_bank_generic_parts.restype = ctypes.c_uint32
    L.pk_bank_generic_episode_bytes.argtypes = [vp]
    L.pk_bank_generic_episode_bytes.restype = ctypes.c_uint64


def bind_tiles(L):
    """argtypes of the tile view (additive to ABI v12; shared with the host-simulation test build)."""
    vp = ctypes.c_void_p
    u32 = ctypes.c_uint32
    L.pk_tiles_create.argtypes = [vp, u32, u32, u32]
    L.pk_tiles_planes.argtypes = [vp]
    L.pk_tiles_planes.restype = u32
    L.pk_tiles_ptr.argtypes = [vp]
    L.pk_tiles_ptr.restype = vp
    L.pk_tiles_eval.argtypes = [vp, vp, vp, vp, u32, u32, vp]


def check(rc: int, what: str):
    if rc != 0:
        msg = load().pk_last_error().decode(errors="replace")
        raise PkError(f"{what} failed ({rc}): {msg}")
