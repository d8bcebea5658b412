"""Host side of tests/test_gpu_matching_routes.py (no GPU): the planning walk of every case of its table, the probe names,
and the route restatement's bookkeeping."""
import ctypes

import pytest

import practicaldeepstereo_nips2018_amd as pds
from tests import test_gpu_matching_routes as routes


@pytest.mark.parametrize('case', routes.CASES, ids=routes.case_id)
def test_workspace_planning_of_every_case(hip_library, case):
    """pds_matching_workspace_bytes plans every configuration of the table (tests/test_abi_and_host.py plans the default
    one), and one more disparity plane never needs less."""
    _, F, S, R, n, h, w, _, dc, _ = case
    params, keep = pds.MatchingOperation(2 * F, F, S, R).native_params()
    need = hip_library.pds_matching_workspace_bytes(ctypes.byref(params), n, h, w, dc)
    assert need > 0, hip_library.pds_last_error()
    more = hip_library.pds_matching_workspace_bytes(ctypes.byref(params), n, h, w, dc + 1)
    assert more >= need, (need, more)
    # (at least the signatures' worth of one 64-channel activation: a failed walk used to return a few hundred bytes)
    assert need >= n * F * dc * h * w * 4
    del keep


def test_no_probe_name_contains_another():
    """The launch probe matches by substring: a name inside another would be counted twice."""
    names = routes.PROBES
    assert len(set(names)) == len(names)
    for a in names:
        assert len(a) < 64      # g_probe_name (csrc/api.hip)
        for b in names:
            assert a == b or a not in b, (a, b)


def test_shard_cases_cover_their_ranges():
    for case in routes.SHARD_CASES:
        planes, shards = case[6], case[7]
        position = 0
        for begin, count in shards:
            assert begin == position and count > 0
            position += count
        assert position == planes


@pytest.mark.parametrize('case', routes.CASES, ids=routes.case_id)
def test_route_restatement_in_a_default_process(case):
    """What the table says each case reaches, read off `expected_route` without switches (the GPU file asserts the same
    dictionary against the launches it counts)."""
    group, F, S, R, n, h, w, d0, dc, _ = case
    counts, facts = routes.expected_route(case, {})
    assert set(counts) == set(routes.PROBES)
    assert facts['fused'] == (F != 32)
    assert facts['columns'] == (facts['fused'] and R >= 1 and F % 8 == 0)
    assert facts['cb8_level'] == (2 if (facts['fused'] and R >= 1 and F == 64 and h % 16 == 0 and w % 16 == 0) else 0)
    assert counts[routes.L0_STACK] == 1
    combine = counts[routes.L1_PLANES] + counts[routes.L1_COLS_STORE] + counts[routes.L1_COLS_STATS]
    assert combine == ((dc + 63) // 64 if facts['fused'] and R >= 1 else 0)
    assert counts[routes.MAT_SUM] == max(R - 2, 0) + (1 if not facts['fused'] and R >= 2 else 0)
    assert counts[routes.MAT_L0] == (1 if facts['fused'] and R >= 2 else 0)
    riders = sum(v for k, v in counts.items() if k.endswith('[l0]') or k.endswith('[a+l0]'))
    assert riders == (1 if facts['fused'] and R <= 1 else 0)
