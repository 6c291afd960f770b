"""The camera dissection brought to a given chain (csrc/chol_plan.hip: refit, fit_dissect), device-free.

The greedy window-separator tree balances every cut in the tiles of its two sides as they are; on the benchmark's camera graph
one half of the orbit came out a tile column longer than the other (12 levels).  refit() brings that tree to a chain one tile
column shorter by cutting anew only what is too long.  Checked here, with depth -3 ("what a handle does") of
mpsfm_debug_plan_create: 11 levels on the C3 camera graph with and without the inverse accumulators, in the caller's numbering
and in three shuffled ones; the two subtrees under the root separator top out at the same level; no item leaves the unrolled
forms of k_chol_level; every such plan solves a random reduced system when its tables are interpreted with NumPy (items of a
launch in random order) and its launch records decode to its items; the interpreter still catches a broken table on it; two
rings that only the hand-over of flatten() and an uneven depth bring down are no worse than before; and the tables do not depend
on the number of planner threads.

PARENT: level counts of commit 6117f1b ("Refine an RGB-D pair's pose on the GPU: dense point-to-plane ICP"), the parent of this
change, for the same graphs (depth -3; the same with and without accumulators), from a run of that commit."""

import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import graph_scenes as G
import level_entry_scenes as LE
from chol_plan_interp import _plan, interpret, reduced_system
from mpsfm_amd.synthetic import make_config
from test_level_heads_cpu import check_heads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C3_LEVELS = 11  # DESIGN.md 8 (rounds 3 to 13): "a hand-placed root reached 11"
MUTATIONS = {"trail_skips_last_source": (True, 0), "panel_ignores_own_tile": (True, 0), "role_skips_last_row": (True, 0),
             "back_skips_last_column": (False, -1), "padding_diagonal_zero": (True, -1)}  # as in test_chol_plan_cuts_cpu.py
# (cameras, reach) -> levels at the parent commit.  224 / 8: the greedy tree has 11 tile columns on its longest path and depth -2
# has 12, one level is not taken; only the tree with a hand-over of up to 2 cameras comes down to 10 (segments one camera over a
# tile boundary).  120 / 10: the greedy tree (10) is taken at the parent; 9 needs an arc cut into two leaves of one tile column
# beside an arc left whole
PARENT = {(224, 8): 12, (120, 10): 10}
TABLES = ("header", "slot_of_nat", "struct_start", "struct_rows", "parent", "level", "items", "launch_start", "srcs", "rows",
          "asm_tiles", "back_cols", "back_start", "col_of_slot")


@functools.lru_cache(maxsize=None)
def _c3_graph():
    return G.covisibility(make_config("C3")[0])


def _shuffled(adj, seed):  # the numberings of test_chol_plan_cuts_cpu.py
    p = np.random.default_rng(seed).permutation(adj.shape[0])
    return np.ascontiguousarray(adj[np.ix_(p, p)])


def _solves(adj, P, seed):
    S, rhs = reduced_system(adj, P, seed=seed)
    y = interpret(P, S, rhs, np.random.default_rng(seed + 100))  # random item order inside every launch
    ref = np.linalg.solve(S, rhs)
    err = np.abs(y - ref).max()
    assert err <= 1e-9 * max(1.0, np.abs(ref).max()), err


def _max_nsrc(P, kind):
    return max((it["nsrc"] for it in P["items"] if it["type"] == kind), default=0)


def _under_the_root(P):
    """(columns of the root separator's chain, tops of the subtrees under it): from the last tile column down while a column has
    one child."""
    parent, nt = P["parent"], P["nt"]
    kids = [[] for _ in range(nt)]
    roots = []
    for j in range(nt):
        (kids[parent[j]] if parent[j] >= 0 else roots).append(j)
    assert roots == [nt - 1], roots  # a connected graph: one tree
    chain, j = [], nt - 1
    while len(kids[j]) == 1:
        chain.append(j)
        j = kids[j][0]
    chain.append(j)
    return chain, kids[j]


def _print_tree(P):
    lev, parent = P["level"], P["parent"]
    for l in range(P["nlevels"]):
        print(f"  level {l:2d}: " + " ".join(f"{j}->{parent[j]}" for j in range(P["nt"]) if lev[j] == l))


def _check_c3_plan(adj, P, pinv):
    chain, tops = _under_the_root(P)
    panel, trail = _max_nsrc(P, 0), _max_nsrc(P, 1)
    print(f"C3 depth -3 pinv={pinv}: nt={P['nt']} levels={P['nlevels']} products={P['products']} roles={P['roles']} max nsrc panel={panel} "
          f"trailing={trail}; root separator columns {chain[::-1]}, subtrees under it top out at "
          + ", ".join(f"column {t} level {P['level'][t]}" for t in tops))
    _print_tree(P)
    assert P["nlevels"] <= C3_LEVELS
    assert P["nt"] <= 64 and P["use_pinv"] == int(pinv)
    assert panel <= 2 and trail <= 4
    assert len(tops) == 2
    assert abs(int(P["level"][tops[0]]) - int(P["level"][tops[1]])) <= 0
    check_heads(P)


@pytest.mark.parametrize("pinv", [True, False])
def test_c3_camera_graph(pinv):
    adj = _c3_graph()
    P = LE.plan_with_heads(adj, depth=-3, pinv_max_tiles=64 if pinv else 0)
    _check_c3_plan(adj, P, pinv)
    _solves(adj, P, seed=41 + pinv)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_c3_camera_graph_shuffled(seed):
    adj = _shuffled(_c3_graph(), seed)
    P = LE.plan_with_heads(adj, depth=-3, pinv_max_tiles=64)
    print(f"C3 shuffled {seed}: levels {_plan(adj, depth=-2)['nlevels']} -> {P['nlevels']}, nt {P['nt']}, "
          f"max nsrc panel={_max_nsrc(P, 0)} trailing={_max_nsrc(P, 1)}")
    assert P["nlevels"] <= C3_LEVELS
    assert P["nt"] <= 64 and P["use_pinv"] == 1
    assert _max_nsrc(P, 0) <= 2 and _max_nsrc(P, 1) <= 4
    assert sorted(P["slot_of_nat"].tolist()) == list(range(adj.shape[0]))
    _solves(adj, P, seed=50 + seed)
    check_heads(P)


@pytest.mark.parametrize("mut", sorted(MUTATIONS))
def test_a_broken_table_of_the_c3_plan_is_caught(mut):
    pinv, which = MUTATIONS[mut]
    adj = _c3_graph()
    P = _plan(adj, depth=-3, pinv_max_tiles=64 if pinv else 0)
    assert P["nlevels"] <= C3_LEVELS  # the plan of this file, not the greedy tree's
    S, rhs = reduced_system(adj, P, seed=61)
    ref = np.linalg.solve(S, rhs)
    tol = 1e-9 * max(1.0, np.abs(ref).max())
    assert np.abs(interpret(P, S, rhs, np.random.default_rng(7)) - ref).max() <= tol
    try:
        err = np.abs(interpret(P, S, rhs, np.random.default_rng(7), mut=mut, which=which) - ref).max()
    except np.linalg.LinAlgError:  # (a zero pivot on a padding row)
        err = np.inf
    print(f"{mut}: error {err:.3g} (bound {tol:.3g})")
    assert not err <= tol


@pytest.mark.parametrize("pinv", [True, False])
@pytest.mark.parametrize("n,reach", sorted(PARENT))
def test_rings(n, reach, pinv):
    adj = G.ring_graph(n, reach)
    tiles = 64 if pinv else 0
    P = LE.plan_with_heads(adj, depth=-3, pinv_max_tiles=tiles)
    legacy = _plan(adj, depth=-2, pinv_max_tiles=tiles)
    print(f"ring {n}/{reach} pinv={pinv}: depth -2 {legacy['nlevels']} levels, parent commit {PARENT[n, reach]}, now {P['nlevels']} "
          f"(nt {legacy['nt']} -> {P['nt']}), max nsrc panel={_max_nsrc(P, 0)} trailing={_max_nsrc(P, 1)}")
    _print_tree(P)
    assert P["nlevels"] <= legacy["nlevels"]
    assert P["nlevels"] <= PARENT[n, reach]
    assert P["use_pinv"] == legacy["use_pinv"] == int(pinv)
    assert _max_nsrc(P, 0) <= 2 and _max_nsrc(P, 1) <= 4
    _solves(adj, P, seed=n)
    check_heads(P)


_DIGEST = """
import hashlib, sys
import numpy as np
import graph_scenes as G
from chol_plan_interp import _plan
from mpsfm_amd.synthetic import make_config
for adj in (G.covisibility(make_config("C3")[0]), G.ring_graph(260, 5), G.ring_graph(224, 8)):
    P = _plan(adj, depth=-3, pinv_max_tiles=64)
    h = hashlib.sha256()
    for k in %r:
        h.update(repr(P[k]).encode() if k == "items" else np.ascontiguousarray(P[k]).tobytes())
    print(P["nlevels"], h.hexdigest())
""" % (TABLES,)


def test_the_plan_does_not_depend_on_the_planner_threads():
    """Depth -3 plans on the host threads a handle plans with (MPSFM_HOST_THREADS, read once per process): every table of the
    C3 plan and of two rings (one of 256 cameras and more) is the same with 1 and with 8 of them."""
    out = {}
    for threads in ("1", "8"):
        env = dict(os.environ, MPSFM_HOST_THREADS=threads, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
        r = subprocess.run([sys.executable, "-c", _DIGEST], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        out[threads] = r.stdout.split()
        print(f"threads {threads}: {r.stdout.strip()}")
    assert len(out["1"]) == 6 and out["1"] == out["8"]
    assert int(out["1"][0]) <= C3_LEVELS
