"""Host side of the level-scheduled tile Cholesky (mpsfm_amd/csrc/chol_plan.hip), checked without a device: the camera
order, the symbolic factorisation and the launch tables are interpreted with NumPy — every item does on 32 x 32 tiles what
its workgroup does on the GPU, launches in order, items of one launch in ANY order (they run concurrently there) — and the
result is compared with a dense Cholesky solve."""

import numpy as np
import pytest

from chol_plan_interp import T, _plan, interpret, reduced_system  # noqa: F401


def ring_graph(n, reach, extra=0, seed=0):
    """Cameras on a closed orbit, every camera sharing landmarks with the `reach` next ones, plus a few random long links."""
    rng = np.random.default_rng(seed)
    adj = np.zeros((n, n), np.uint8)
    for i in range(n):
        for d in range(1, reach + 1):
            adj[i, (i + d) % n] = adj[(i + d) % n, i] = 1
    for _ in range(extra):
        a, b = rng.integers(0, n, 2)
        if a != b:
            adj[a, b] = adj[b, a] = 1
    return adj



@pytest.mark.parametrize("n,reach,extra,depth,pinv", [
    (70, 5, 0, -1, True), (70, 5, 0, 0, True), (70, 5, 0, 1, True), (120, 6, 0, 2, True), (120, 6, 3, -2, True),
    (150, 4, 0, 2, False), (260, 5, 2, 3, False), (20, 19, 0, -2, True), (7, 2, 0, -2, True),
])
def test_plan_solves_the_reduced_system(n, reach, extra, depth, pinv):
    adj = ring_graph(n, reach, extra, seed=n)
    P = _plan(adj, depth=depth, pinv_max_tiles=64 if pinv else 0)
    assert P["ncv"] == n and P["nslots"] == n and P["n"] >= 6 * n
    slot = P["slot_of_nat"]
    assert sorted(slot.tolist()) == list(range(n))  # a permutation
    c = np.sort(P["col_of_slot"])
    assert c[0] == 0 and (np.diff(c) >= 6).all() and c[-1] + 6 == P["n"]  # six columns each, no overlap
    assert P["use_pinv"] == int(pinv and P["nt"] <= 64)
    S, rhs = reduced_system(adj, P, seed=1)
    y = interpret(P, S, rhs, np.random.default_rng(5))
    ref = np.linalg.solve(S, rhs)
    assert np.abs(y - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())


def test_two_separate_scenes_are_two_chains():
    a = ring_graph(60, 4)
    adj = np.zeros((120, 120), np.uint8)
    adj[:60, :60] = a
    adj[60:, 60:] = a
    P = _plan(adj, depth=0)
    # every component is a multiple of 16 slots but the last; the two chains advance in the same launches
    assert P["nlevels"] <= (P["nt"] + 1) // 2 + 2
    S, rhs = reduced_system(adj, P, seed=2)
    y = interpret(P, S, rhs, np.random.default_rng(1))
    assert np.abs(y - np.linalg.solve(S, rhs)).max() < 1e-9


def test_dissection_shortens_the_chain_of_an_orbit():
    adj = ring_graph(199, 14)  # the C3 camera graph in shape
    ident = _plan(adj, depth=-1)
    auto = _plan(adj, depth=-2)
    assert ident["nlevels"] == ident["nt"] == 38
    assert auto["nd_depth"] >= 1 and auto["nlevels"] <= 24
    assert auto["products"] <= 2 * ident["products"]


def _graph(kind, n, seed=0):
    rng = np.random.default_rng(seed)
    adj = np.zeros((n, n), np.uint8)
    if kind == "path":
        for i in range(n - 1):
            adj[i, i + 1] = 1
    elif kind == "star":
        adj[0, 1:] = 1
    elif kind == "complete":
        adj[:] = 1
    elif kind == "grid":  # cameras on a lattice (aerial blocks): neighbours in both directions
        w = int(np.sqrt(n))
        for i in range(n):
            for d in (1, w, w + 1, w - 1):
                j = i + d
                if j < n and not (d == 1 and j % w == 0):
                    adj[i, j] = 1
    elif kind == "random":
        m = rng.random((n, n)) < 6.0 / n
        adj[m] = 1
    elif kind == "isolated":  # a sequence, a clique and cameras that share nothing with anyone
        for i in range(40):
            for d in (1, 2, 3):
                if i + d < 40:
                    adj[i, i + d] = 1
        adj[50:62, 50:62] = 1
    adj = np.maximum(adj, adj.T)
    np.fill_diagonal(adj, 0)
    return adj


@pytest.mark.parametrize("kind,n", [("path", 90), ("star", 70), ("complete", 40), ("grid", 144), ("random", 100), ("isolated", 75)])
@pytest.mark.parametrize("depth", [-2, 3])
def test_plan_on_other_camera_graphs(kind, n, depth):
    adj = _graph(kind, n, seed=n)
    P = _plan(adj, depth=depth)
    S, rhs = reduced_system(adj, P, seed=3)
    y = interpret(P, S, rhs, np.random.default_rng(9))
    ref = np.linalg.solve(S, rhs)
    assert np.abs(y - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())
    if kind == "path" and depth == -2:
        assert P["nlevels"] < P["nt"]  # a chain dissects into chains
    if kind == "complete":
        assert P["nlevels"] == P["nt"]  # nothing to gain: one dense chain, whatever the order
