"""tests/derive_graphs.py without a GPU: every builder constructs its graph and asserts its own
property (the builders assert before they hand a graph out; the checks here restate what
test_gpu_derive_edges.py rests on), and the CPU model of the derivation (DESIGN §5.9:
distances as neighbour minimums, predecessors as the best of the optimal neighbours' canonical
arcs and the direct arc) agrees with the oracle's Dijkstra rows on every family: no wrong distance
and no wrong predecessor, so a GPU failure on these graphs is the kernel's."""
import numpy as np
import pytest

import derive_graphs as dg
import sparse_graphs as sg

ALL = {**dg.CASES, **dg.OFF_CASES}


@pytest.mark.parametrize("name", list(ALL))
def test_builder_conditions_and_model(native, name):
    g = ALL[name]()
    print(f"{name}: {dg.describe(g)}")
    c = sg.canon(g)
    assert g.nI == int(g.inI.sum()) == sum(g.deg_hist.values())
    assert g.ties[2] == 0
    assert (sg.max_arc_weight(g) < 128) == (name != "pendants128")
    assert sg.distinct_reliabilities(g) <= 256 and c["arcs"] < 2 ** 20 and 2 * g.ecc0 <= 1022
    bad_d, bad_p, rows = dg.check_model(g)
    print(f"{name}: model on {rows} derived rows: {bad_d} wrong distances, {bad_p} wrong "
          f"predecessors")
    assert rows == (min(g.nI, 120) if g.n > 1500 else g.nI)
    assert (bad_d, bad_p) == (0, 0)


def test_model_check_sees_a_wrong_row(native):
    """The model's check is not vacuous: against rows with one distance raised, and against rows
    with one tied predecessor swapped for the other tight one, it reports exactly those."""
    g = dg.grid(40, 50, 1)
    c = sg.canon(g)
    D, _, P = dg.oracle_rows(g)
    s = int(np.nonzero(g.inI)[0][5])
    t = int(np.argmax(np.where(D[s] < dg.INF, D[s], -1)))
    D2 = D.copy()
    D2[s, t] += 1
    assert dg.model_check(c["rp"], c["col"], c["w"], g.inI, D2, P, [s])[0] == 1
    other = [int(u) for u in c["col"][c["rp"][t]:c["rp"][t + 1]]
             if D[s, u] + 1 == D[s, t] and u != P[s, t]]
    assert other  # the farthest target of a unit lattice is tied
    P2 = P.copy()
    P2[s, t] = other[0]
    assert dg.model_check(c["rp"], c["col"], c["w"], g.inI, D, P2, [s]) == (0, 1)


@pytest.mark.parametrize("wmax", [1, 2, 3])
def test_grid_degrees_core_and_depth(native, wmax):
    g = dg.grid(40, 50, wmax)
    deg = sg.canon(g)["deg"]
    assert g.n == 2000 and set(g.deg_hist) == {2, 3, 4}
    assert int(((deg <= 4) & ~g.inI).sum()) > 1000 and g.depth >= 80
    assert g.ties[1] / g.ties[0] >= {1: 0.90, 2: 0.25, 3: 0.0}[wmax]


def test_ring_even_and_odd(native):
    g = dg.ring(1000)
    assert g.nI == 500 and g.deg_hist == {2: 500} and 2 * g.ecc0 == 1000
    g = dg.ring(601, 2)
    assert g.nI == 300 and not g.inI[599] and not g.inI[600] and g.ties[1] == 0


def test_ba_degrees(native):
    assert dg.ba(1).deg_hist.get(1, 0) > 0.95 * dg.ba(1).nI
    assert max(dg.ba(2).deg_hist, key=dg.ba(2).deg_hist.get) == 2
    assert set(dg.ba(4).deg_hist) == {4}
    assert dg.ba(5).nI == 0 and dg.ba(5).deg_hist == {}


def test_pendants_in_the_set(native):
    g = dg.pendants(127)
    assert g.deg_hist[1] == 300 and g.inI[-300:].all()
    assert sg.max_arc_weight(dg.pendants(128)) == 128 and dg.pendants(128).nI > 0


def test_pendant_losses_fill_the_table_from_direct_arcs(native):
    g = dg.pendant_losses()
    c = sg.canon(g)
    assert sg.distinct_reliabilities(g) == 256
    on_pendants = np.unique(c["r"][c["rp"][-301:-1]].view(np.uint64))
    assert len(on_pendants) == 256 and g.inI[-300:].all()


def test_islands_components_and_set(native):
    g = dg.islands()
    h = g.head
    D = dg.oracle_rows(g)[0]
    assert np.array_equal(D < dg.INF, g.comp[:, None] == g.comp[None, :])
    assert (D[h, np.arange(g.n) != h] >= dg.INF).all()  # the isolated vertex
    assert int(g.inI[h + 1:h + 3].sum()) == 1 and g.inI[h + 3] and g.inI[h + 5] and not g.inI[h]
