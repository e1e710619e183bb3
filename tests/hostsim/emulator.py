"""BatchedEmulator over the host-simulation build (TEST INFRASTRUCTURE ONLY).

The unmodified kernels + C ABI compiled with g++ (tests/hostsim) keep every "device" buffer in
host memory, so the product's BatchedEmulator — its own constructor included — runs on CPU tensors
wrapped around those buffers.  Used by the CPU tests of the multi-rank benchmark flow
(tests/test_dist.py): the product path itself has no CPU fallback (pokegym_amd/emulator.py refuses
to start without a GPU)."""
from __future__ import annotations

import contextlib
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import sim  # noqa: E402
from pokegym_amd import _native  # noqa: E402
from pokegym_amd.emulator import BatchedEmulator  # noqa: E402


class HostsimEmulator(BatchedEmulator):
    def _backend(self, device):
        L = sim.lib()
        _native.bind(L)
        return L, torch.device("cpu"), contextlib.nullcontext()

    def _stream(self):
        return None
