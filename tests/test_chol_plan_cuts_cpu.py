"""The window-separator camera orders of the level-scheduled Cholesky (csrc/chol_plan.hip: cut_dissect), device-free.

mpsfm_debug_plan_create takes depth -3 for "what a handle does": the automatic choice of depth -2 plus the orders from a
dissection by minimal window separators, which replace it only with at least two levels less, the inverse accumulators
kept, on graphs of at least 64 cameras whose chain has at least eight levels, and with items that stay in the unrolled forms
of k_chol_level (two sources of a panel, four of a trailing tile).  Checked here: the level counts on the benchmark's camera graph (in the caller's order and
shuffled) and on two rings, that every such plan solves a random reduced system when its tables are interpreted with NumPy
(items of a launch in random order), that its launch records decode to its items, that the graphs on which the search
may not win keep the depth -2 tables entry for entry, and that the interpreter still catches a broken table on a
cut-search plan."""

import functools

import numpy as np
import pytest

import graph_scenes as G
import level_entry_scenes as LE
from chol_plan_interp import _eligible, _plan, interpret, reduced_system
from mpsfm_amd.synthetic import make_config
from test_level_heads_cpu import check_heads

TABLES = ("header", "slot_of_nat", "struct_start", "struct_rows", "parent", "level", "launch_start", "srcs", "rows", "asm_tiles",
          "back_cols", "back_start", "col_of_slot")
# the switches of chol_plan_interp.interpret used for the detection-power test -> (accumulators?, which item).  The first item
# the rule applies to: the last ones sit in the root's last tile column, mostly padding, where a lost product is an exact zero
MUTATIONS = {"trail_skips_last_source": (True, 0), "panel_ignores_own_tile": (True, 0), "role_skips_last_row": (True, 0),
             "back_skips_last_column": (False, -1), "padding_diagonal_zero": (True, -1)}


@functools.lru_cache(maxsize=None)
def _c3_graph():
    return G.covisibility(make_config("C3")[0])


def _solves(adj, P, seed):
    S, rhs = reduced_system(adj, P, seed=seed)
    y = interpret(P, S, rhs, np.random.default_rng(seed + 100))  # random item order inside every launch
    ref = np.linalg.solve(S, rhs)
    err = np.abs(y - ref).max()
    assert err <= 1e-9 * max(1.0, np.abs(ref).max()), err


def _same_tables(A, B):
    for k in TABLES:
        assert np.array_equal(A[k], B[k]), k
    assert A["items"] == B["items"]


def _max_nsrc(P, kind):
    return max((it["nsrc"] for it in P["items"] if it["type"] == kind), default=0)


def test_c3_camera_graph():
    adj = _c3_graph()
    P = LE.plan_with_heads(adj, depth=-3, pinv_max_tiles=64)
    legacy = _plan(adj, depth=-2, pinv_max_tiles=64)
    panel, trail = _max_nsrc(P, 0), _max_nsrc(P, 1)
    print(f"C3 depth -3: nt={P['nt']} levels={P['nlevels']} products={P['products']} roles={P['roles']} nd_depth={P['nd_depth']} "
          f"max nsrc panel={panel} trailing={trail} | depth -2: nt={legacy['nt']} levels={legacy['nlevels']} products={legacy['products']}")
    assert (legacy["nt"], legacy["nlevels"]) == (39, 14)
    assert P["nlevels"] <= 12
    assert P["nt"] <= 64 and P["use_pinv"] == 1
    _solves(adj, P, seed=11)
    check_heads(P)
    # more than 2 / 4 sources would be correct but take the slower loops of k_chol_level: the planner refuses such a plan
    assert panel <= 2 and trail <= 4


def test_c3_camera_graph_without_accumulators():
    adj = _c3_graph()
    P = LE.plan_with_heads(adj, depth=-3, pinv_max_tiles=0)
    assert P["nlevels"] <= 12 and P["use_pinv"] == 0
    _solves(adj, P, seed=12)
    check_heads(P)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_c3_camera_graph_shuffled(seed):
    """The arrangement does not lean on the caller's numbering: with the cameras renumbered at random the plan has no more
    levels than the depth -2 plan of the same graph."""
    adj = _c3_graph()
    p = np.random.default_rng(seed).permutation(adj.shape[0])
    adj = np.ascontiguousarray(adj[np.ix_(p, p)])
    P, legacy = _plan(adj, depth=-3), _plan(adj, depth=-2)
    print(f"C3 shuffled {seed}: levels {legacy['nlevels']} -> {P['nlevels']}, nt {legacy['nt']} -> {P['nt']}")
    assert P["nlevels"] <= legacy["nlevels"]
    assert sorted(P["slot_of_nat"].tolist()) == list(range(adj.shape[0]))
    _solves(adj, P, seed=20 + seed)


@pytest.mark.parametrize("pinv", [True, False])
@pytest.mark.parametrize("n,reach", [(260, 5), (120, 6)])
def test_rings(n, reach, pinv):
    adj = G.ring_graph(n, reach)
    P = LE.plan_with_heads(adj, depth=-3, pinv_max_tiles=64 if pinv else 0)
    legacy = _plan(adj, depth=-2, pinv_max_tiles=64 if pinv else 0)
    print(f"ring {n}/{reach} pinv={pinv}: levels {legacy['nlevels']} -> {P['nlevels']}, nt {legacy['nt']} -> {P['nt']}")
    assert P["nlevels"] < legacy["nlevels"]
    assert P["use_pinv"] == legacy["use_pinv"] == int(pinv)
    _solves(adj, P, seed=n)
    check_heads(P)


NO_WIN = {"orbit40": lambda: LE.problem("orbit", 40)[0], "clique4": lambda: LE.problem("clique", 4)[0]}
NO_WIN.update({f"star{L}": (lambda L=L: LE.star_adj(L)) for L in LE.STAR_LEAVES})
NO_WIN.update({name: (lambda name=name: G.graph(G.CASES[name][0], G.CASES[name][1], G.CASES[name][3])) for name in G.CASES})


@pytest.mark.parametrize("pinv", [True, False])
@pytest.mark.parametrize("name", sorted(NO_WIN))
def test_graphs_where_the_search_does_not_win_keep_their_tables(name, pinv):
    adj = NO_WIN[name]()
    tiles = 64 if pinv else 0
    _same_tables(_plan(adj, depth=-3, pinv_max_tiles=tiles), _plan(adj, depth=-2, pinv_max_tiles=tiles))


@pytest.mark.parametrize("mut", sorted(MUTATIONS))
def test_a_broken_table_of_a_cut_search_plan_is_caught(mut):
    pinv, which = MUTATIONS[mut]
    adj = _c3_graph()
    tiles = 64 if pinv else 0
    P = _plan(adj, depth=-3, pinv_max_tiles=tiles)
    assert P["nlevels"] < _plan(adj, depth=-2, pinv_max_tiles=tiles)["nlevels"]  # a cut-search plan
    S, rhs = reduced_system(adj, P, seed=31)
    ref = np.linalg.solve(S, rhs)
    tol = 1e-9 * max(1.0, np.abs(ref).max())
    assert np.abs(interpret(P, S, rhs, np.random.default_rng(7)) - ref).max() <= tol
    try:
        err = np.abs(interpret(P, S, rhs, np.random.default_rng(7), mut=mut, which=which) - ref).max()
    except np.linalg.LinAlgError:  # (a zero pivot on a padding row)
        err = np.inf
    print(f"{mut}: error {err:.3g} (bound {tol:.3g})")
    assert not err <= tol
