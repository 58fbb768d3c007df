"""tests/tie_reference.py itself, on hand-built graphs whose tied-pair count is obvious (CPU: the
oracle's distances and numpy). The GPU tests (test_gpu_ties.py) hold every kernel that counts
srt_build_stats.tied_pairs to this reference."""
import json
import os

import numpy as np
import pytest
from conftest import GOLDEN

import oracle
from tie_reference import distances_of_oracle, tied_pairs

MS = 1_000_000


def _count(n, directed, edges, rows=None):
    """edges: (u, v, ms[, loss]); distances from the oracle's Dijkstra."""
    e = np.array([x[:3] for x in edges], np.int64)
    lat = e[:, 2] * MS
    el = oracle.EdgeList(n, directed, e[:, 0], e[:, 1], lat, np.zeros(len(e)))
    D = distances_of_oracle(oracle.table(el, True, oracle.ORC_INT_NS, 1, raw=True)["lat_int"])
    return tied_pairs(n, directed, e[:, 0], e[:, 1], lat, D, rows)


DIAMOND = [(0, 1, 1), (0, 2, 1), (1, 3, 1), (2, 3, 1)]


def test_diamond():
    """(0, 3) and (3, 0) over {1, 2}, (1, 2) and (2, 1) over {0, 3}: both predecessors at D = 1."""
    assert _count(4, False, DIAMOND) == 4
    assert _count(4, False, DIAMOND, rows=(0, 1)) == 1
    assert _count(4, False, DIAMOND, rows=(1, 4)) == 3


def test_diamond_self_loops_and_parallel_edges_change_nothing():
    extra = [(v, v, 1) for v in range(4)] + [(0, 1, 7), (1, 0, 1)]
    assert _count(4, False, DIAMOND + extra) == 4


def test_diamond_one_arm_longer():
    assert _count(4, False, [(0, 1, 1), (0, 2, 1), (1, 3, 2), (2, 3, 1)]) == 0


def test_three_equal_arms():
    """0 - {1, 2, 3} - 4: (0, 4) and (4, 0) over three predecessors, and every ordered pair of
    arms over {0, 4}."""
    e = [(0, a, 1) for a in (1, 2, 3)] + [(a, 4, 1) for a in (1, 2, 3)]
    assert _count(5, False, e) == 2 + 6


def test_two_tight_predecessors_at_different_distances():
    """The square 2+3 / 3+2: both in-arcs of 3 are tight from 0, but D[0][1] = 2 < D[0][2] = 3 --
    the smallest is reached once."""
    assert _count(4, False, [(0, 1, 2), (1, 3, 3), (0, 2, 3), (2, 3, 2)]) == 0


def test_direct_arc_against_two_hops():
    """0-2 direct (10) ties 0-1-2 (5 + 5) in length, but the source itself (D = 0) is the single
    smallest predecessor."""
    assert _count(3, False, [(0, 1, 5), (1, 2, 5), (0, 2, 10)]) == 0


def test_directed_diamond():
    """0 -> {1, 2} -> 3: only (0, 3) exists with two predecessors."""
    assert _count(4, True, DIAMOND) == 1
    assert _count(4, True, DIAMOND, rows=(0, 1)) == 1
    assert _count(4, True, DIAMOND, rows=(1, 4)) == 0


def test_unreachable_pairs_are_never_tied():
    """Two diamonds with no edge between them; a directed diamond's unreachable sources."""
    two = DIAMOND + [(a + 4, b + 4, w) for a, b, w in DIAMOND]
    assert _count(8, False, two) == 8
    assert _count(8, True, two) == 2


# hand counts of tests/golden/ties.json (make_golden.py: tie_graphs): only the diamond has a
# smallest tight D[s][u] reached twice (its four pairs above)
GOLDEN_TIED = {"triangle_direct_vs_two_hop": 0, "square_pred_by_distance": 0,
               "diamond_pred_by_index": 4, "directed_cycle": 0, "path_no_selfloops": 0,
               "parallel_edges": 0}


@pytest.mark.parametrize("name", sorted(GOLDEN_TIED))
def test_golden_tie_graphs(name):
    case = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "ties.json")))}[name]
    assert _count(case["n"], case["directed"], case["edges"]) == GOLDEN_TIED[name]
