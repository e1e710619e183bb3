"""The gfx950 K1 and the oracle side by side from the injected machine states of
tests/state_cases.py (the host simulation runs the same cases in tests/test_hostsim_states.py):
whole v9 state and screen after every step, at most 512 envs per launch, default and small-LDS
kernel, 64 / 32 / 16 envs per wave, and the cases in reversed env order."""
import pytest

from tests import state_cases as SC
from tests import state_common as CM

pytestmark = pytest.mark.gpu

SHAPES = {
    "default_l64": {},
    "default_l32": {"PK_WAVE_LANES": "32"},
    "small_l32": {"PK_K1_SMALL": "1", "PK_WAVE_LANES": "32", "PK_K1_BLOCK": "256"},
    "small_l16": {"PK_K1_SMALL": "1", "PK_WAVE_LANES": "16", "PK_K1_BLOCK": "256"},
    "default_l64_reversed": {},
}


# (ROM variant, launch of at most 512 envs): one test each, a few seconds
PARTS = [(2, 0), (2, 1), (2, 2), (8, 0), (64, 0)]


def test_parts_cover_every_case():
    assert PARTS == [(nb, k) for nb in (2, 8, 64) for k in range(len(CM.launches(SC.all_cases(), nb)))]


@pytest.mark.parametrize("part", PARTS, ids=[f"{nb}b-{k}" for nb, k in PARTS])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_states_match_the_oracle_on_device(shape, part, monkeypatch):
    for k, v in SHAPES[shape].items():
        monkeypatch.setenv(k, v)
    batch = CM.launches(SC.all_cases(), part[0], reverse=shape.endswith("reversed"))[part[1]]
    bad = CM.run_launch(CM.GpuAdapter, batch)
    assert not bad, (len(bad), bad[:12])
