"""Camera graphs and problems that put the items of the level-scheduled Cholesky on the caps of their launch records
(csrc/chol_plan.h: LevelHead, kInlineSrc sources held in the record, longer lists continue in `srcs`).  Shared by
test_level_heads_cpu.py, which asserts from the device-free plan that every graph reaches what it is named for, and
test_gpu_level_entry.py, which runs the kernels on them.

A star is L leaf cliques of 16 cameras (96 columns: three whole tiles) around a hub clique of 16, in the caller's order
(MPSFM_CHOL_ND=-1): the three tile columns of a leaf are a chain of levels 0, 1, 2 and all leaves advance in the same launches,
so the first hub column has L children at the level below it — its panel items have nsrc = L — and the hub's tiles receive
the L leaf columns of a level in one trailing item each, nsrc = L again."""

import functools

import numpy as np

import chunk_cap_scenes as CC
from chol_plan_interp import _plan
from mpsfm_amd import capi

K_INLINE_SRC = 8  # csrc/chol_plan.h
K_HEAD_ROWS = 4
CLIQUE = 16
STAR_LEAVES = (2, K_INLINE_SRC - 1, K_INLINE_SRC, K_INLINE_SRC + 1, 2 * K_INLINE_SRC + 1)
ORDER_ENV = {"MPSFM_CHOL_ND": "-1"}  # the stars are built for the caller's order


def star_adj(leaves):
    n = CLIQUE * (leaves + 1)
    adj = np.zeros((n, n), np.uint8)
    hub = slice(CLIQUE * leaves, n)
    for l in range(leaves + 1):
        s = slice(CLIQUE * l, CLIQUE * (l + 1))
        adj[s, s] = 1
        adj[s, hub] = adj[hub, s] = 1
    np.fill_diagonal(adj, 0)
    return adj


def decode_heads(words):
    """Code 14 of mpsfm_debug_plan_get -> one dict per item: type, ti, tk, nsrc, the inline sources, the inline rows, the overflow offset."""
    w = np.asarray(words, np.int64).reshape(-1, 16) & 0xffffffff
    return [dict(type=int(r[0] & 0xffff), ti=int(r[0] >> 16), tk=int(r[1] & 0xffff), nsrc=int(r[1] >> 16),
                 src=[int(x) for x in r[2:2 + K_INLINE_SRC]], row=[int(x) for x in r[2 + K_INLINE_SRC:2 + K_INLINE_SRC + K_HEAD_ROWS]],
                 over=int(r[2 + K_INLINE_SRC + K_HEAD_ROWS]), pad=int(r[15])) for r in w]


def plan_with_heads(adj, depth=-2, pinv_max_tiles=64, inv_rows=2):
    """chol_plan_interp._plan plus `heads`, the decoded launch records of the same plan (the plan is deterministic: built twice)."""
    P = _plan(adj, depth=depth, pinv_max_tiles=pinv_max_tiles, inv_rows=inv_rows)
    L = capi.lib()
    a = np.ascontiguousarray(adj, dtype=np.uint8)
    h = L.mpsfm_debug_plan_create(a.ctypes.data, a.shape[0], depth, pinv_max_tiles, inv_rows)
    assert h
    n = L.mpsfm_debug_plan_get(h, 14, None, 0)
    buf = np.zeros(max(n, 1), np.int32)
    L.mpsfm_debug_plan_get(h, 14, buf.ctypes.data, n)
    L.mpsfm_debug_plan_destroy(h)
    P["heads"] = decode_heads(buf[:n])
    return P


def item_lists(P, it):
    """(sources, rows) of an item as the tables of record give them (codes 6, 8, 9)."""
    if it["type"] == 2:
        return [], [int(x) for x in P["rows"][it["aux"]:it["aux"] + it["nsrc"]]]
    return [int(x) for x in P["srcs"][it["src"]:it["src"] + it["nsrc"]]], []


def head_lists(P, H):
    """(sources, rows) of an item as its launch record gives them, the overflow tail read from srcs / rows at `over`."""
    n = H["nsrc"]
    if H["type"] == 2:
        tail = [int(x) for x in P["rows"][H["over"]:H["over"] + max(n - K_HEAD_ROWS, 0)]]
        return [], H["row"][:min(n, K_HEAD_ROWS)] + tail
    tail = [int(x) for x in P["srcs"][H["over"]:H["over"] + max(n - K_INLINE_SRC, 0)]]
    return H["src"][:min(n, K_INLINE_SRC)] + tail, []


@functools.lru_cache(maxsize=None)
def _graph_problem(key):
    kind, arg = key
    if kind == "star":
        adj = star_adj(arg)
    elif kind == "orbit":  # every camera shares landmarks with its two next neighbours on a closed orbit
        adj = np.zeros((arg, arg), np.uint8)
        for i in range(arg):
            for d in (1, 2):
                adj[i, (i + d) % arg] = adj[(i + d) % arg, i] = 1
    elif kind == "clique":  # arg cameras that all see each other: one tile column up to five cameras
        adj = np.ones((arg, arg), np.uint8) - np.eye(arg, dtype=np.uint8)
    else:
        raise KeyError(kind)
    n = adj.shape[0]
    ei, ej = np.nonzero(np.triu(adj, 1))
    # camera 0 is constant, node i is camera i + 1; two landmarks per edge, two per camera shared with camera 0 only
    tracks = [(int(a) + 1, int(b) + 1) for a, b in zip(ei, ej) for _ in range(2)] + [(0, i + 1) for i in range(n) for _ in range(2)]
    return adj, CC.scene(n + 1, tracks, seed=100 + n)


def problem(kind, arg):
    """(adjacency of the variable cameras, a fresh copy of the problem) of ("star", L), ("orbit", n) or ("clique", n)."""
    adj, prob = _graph_problem((kind, arg))
    return adj, prob.copy()
