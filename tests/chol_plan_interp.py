"""The launch tables of the level-scheduled tile Cholesky (mpsfm_amd/csrc/chol_plan.hip), read through the debug calls and
interpreted with NumPy: every item does on 32 x 32 tiles what its workgroup does on the GPU, launches in order, items of one
launch in ANY order (they run concurrently there).  Shared by the host-side plan tests and the dense-solve tests on camera
graphs; `interpret` takes switches (`mut`, off by default) that each break one rule of the tables, for the tests that show
a check has power."""

import ctypes as C

import numpy as np

from mpsfm_amd import capi

T = 32


def _plan(adj, depth=-2, pinv_max_tiles=64, inv_rows=2):
    L = capi.lib()
    a = np.ascontiguousarray(adj, dtype=np.uint8)
    h = L.mpsfm_debug_plan_create(a.ctypes.data, a.shape[0], depth, pinv_max_tiles, inv_rows)
    assert h
    out = {}
    names = ["header", "slot_of_nat", "struct_start", "struct_rows", "parent", "level", "items", "launch_start", "srcs", "rows",
             "asm_tiles", "back_cols", "back_start", "col_of_slot"]
    for what, name in enumerate(names):
        n = L.mpsfm_debug_plan_get(h, what, None, 0)
        buf = np.zeros(max(n, 1), np.int32)
        L.mpsfm_debug_plan_get(h, what, buf.ctypes.data, n)
        out[name] = buf[:n]
    L.mpsfm_debug_plan_destroy(h)
    hd = out["header"]
    out.update(dict(zip(["ncv", "nslots", "n", "nt", "nlevels", "nd_depth", "use_pinv", "n_items", "products", "roles"], map(int, hd))))
    it = out["items"].reshape(-1, 4).astype(np.int64)
    out["items"] = [dict(type=int(a & 0xffff), ti=int((a >> 16) & 0xffff), tk=int(b & 0xffff), nsrc=int((b >> 16) & 0xffff), src=int(c), aux=int(d))
                    for a, b, c, d in it]
    return out


def reduced_system(adj, P, seed):
    """SPD matrix with the block pattern of the graph, every camera's 6 x 6 blocks at the columns the plan gives its slot
    (padding columns between segments: identity rows), and a rhs."""
    rng = np.random.default_rng(seed)
    ncv, ns, n = P["ncv"], P["nslots"], P["n"]
    slot = P["col_of_slot"][P["slot_of_nat"]] // 6 if False else None
    col = P["col_of_slot"][P["slot_of_nat"]]  # first column of every camera (caller's order)
    S = np.zeros((n, n))
    for i in range(ncv):
        for j in range(i, ncv):
            if i == j or adj[i, j]:
                B = rng.standard_normal((6, 6)) * (1.0 if i == j else 0.3)
                a, b = int(col[i]), int(col[j])
                S[a:a + 6, b:b + 6] += B
                if i != j:
                    S[b:b + 6, a:a + 6] += B.T
    S = 0.5 * (S + S.T)
    real = np.zeros(n, bool)
    for i in range(ncv):
        real[col[i]:col[i] + 6] = True
    S[np.diag_indices(n)] = np.where(real, np.abs(S).sum(1) + 1.0, 1.0)
    rhs = np.where(real, rng.standard_normal(n), 0.0)
    return S, rhs


def place(S_user, rhs_user, P):
    """A system given in the caller's camera order (6 rows per camera), put at the columns the plan gives every camera's
    slot, identity on the padding columns.  Returns (S, rhs, idx) with S[idx][:, idx] == S_user: y[idx] is the solution in
    the caller's order."""
    col = P["col_of_slot"][P["slot_of_nat"]].astype(np.int64)
    idx = (col[:, None] + np.arange(6)[None, :]).ravel()
    n = P["n"]
    assert S_user.shape == (idx.size, idx.size) and np.unique(idx).size == idx.size
    S = np.eye(n)
    S[idx, idx] = 0.0
    S[np.ix_(idx, idx)] = S_user
    rhs = np.zeros(n)
    rhs[idx] = rhs_user
    return S, rhs, idx


# Switches of `interpret` that each break ONE rule of the tables (all off by default).  Where a rule is broken for one item,
# `which` counts the items the rule applies to (negative: from the end).
MUTATIONS = ("trail_skips_last_source", "panel_ignores_own_tile", "role_skips_last_row", "back_skips_last_column",
             "padding_diagonal_zero", "item_applied_early")


def _eligible(P, mut):
    """Indices (into P["items"]) of the items a per-item mutation can break."""
    srcs = P["srcs"]
    out = []
    for q, it in enumerate(P["items"]):
        if mut == "trail_skips_last_source" and it["type"] == 1 and it["nsrc"] >= 1:
            out.append(q)
        elif mut == "panel_ignores_own_tile" and it["type"] == 0 and it["ti"] != it["tk"] and it["ti"] < P["nt"] and \
                any(int(e) >> 16 for e in srcs[it["src"]:it["src"] + it["nsrc"]]):
            out.append(q)
        elif mut == "role_skips_last_row" and it["type"] == 2 and it["ti"] != it["tk"]:
            out.append(q)
        elif mut == "item_applied_early":
            out.append(q)
    return out


def interpret(P, S, rhs, rng, mut=None, which=-1):
    nt, n = P["nt"], P["n"]
    N = nt * T
    A = np.zeros((N + T, N))
    A[:n, :n] = S
    for r in range(n, N):
        A[r, r] = 1.0
    assert mut is None or mut in MUTATIONS
    if mut == "padding_diagonal_zero":  # k_assemble leaves the padding rows as the zero fill found them
        real = np.zeros(N, bool)
        col = P["col_of_slot"][P["slot_of_nat"]]
        for c in col:
            real[c:c + 6] = True
        assert not real.all(), "this plan has no padding row"
        A[np.flatnonzero(~real), np.flatnonzero(~real)] = 0.0
    hit = -1  # the one item a per-item mutation breaks
    if mut in ("trail_skips_last_source", "panel_ignores_own_tile", "role_skips_last_row", "item_applied_early"):
        el = _eligible(P, mut)
        assert el, f"{mut}: this plan has no item the rule applies to"
        hit = el[which]
    A[N, :n] = rhs  # row 0 of the rhs tile row
    live = set(int(x) for x in P["asm_tiles"])
    lt = lambda ti, tj: ti * (ti + 1) // 2 + tj
    tile = lambda ti, tj: A[ti * T:(ti + 1) * T, tj * T:(tj + 1) * T]
    # tiles outside the plan must be structurally zero in S
    for ti in range(nt):
        for tj in range(ti):
            if lt(ti, tj) not in live:
                assert not tile(ti, tj).any(), f"tile ({ti},{tj}) of S is nonzero but not in the plan"
    Linv = {}
    Pinv = {}
    srcs, rows = P["srcs"], P["rows"]
    done_col = np.full(nt, -1)
    for l in range(P["nlevels"]):
        items = P["items"][P["launch_start"][l]:P["launch_start"][l + 1]]
        # reads see the state before the launch (what another workgroup of the same launch writes may not be there yet);
        # two items of a launch must never write the same tile
        A0 = A.copy()
        t0 = lambda ti, tj: A0[ti * T:(ti + 1) * T, tj * T:(tj + 1) * T]
        written = set()
        reads = []  # (item index, key) of everything an item reads that it does not own
        Pinv0 = {k: v.copy() for k, v in Pinv.items()}
        order = rng.permutation(len(items))
        base = int(P["launch_start"][l])
        early = mut == "item_applied_early" and base <= hit < base + len(items) and len(items) > 1
        if early:  # the chosen item first, and what it writes is what every other item of the launch then reads
            order = np.concatenate([[hit - base], order[order != hit - base]])
        for q in order:
            if early and q == order[1]:  # (the chosen item has run: the state the others read now holds what it wrote)
                A0 = A.copy()
                Pinv0 = {k: v.copy() for k, v in Pinv.items()}
            it = items[q]
            broken = base + q == hit
            if it["type"] == 2:  # inverse role: P(i,k) += L(i,j) X(j,k)
                j, k = it["ti"], it["tk"]
                assert done_col[j] >= 0 and done_col[j] < l
                X = Linv[j] if k == j else -Linv[j] @ Pinv0.get((j, k), np.zeros((T, T)))
                reads.append((q, ("Linv", j)))
                if k != j:
                    reads.append((q, ("P", j, k)))
                role_rows = rows[it["aux"]:it["aux"] + it["nsrc"]]
                if broken and mut == "role_skips_last_row":
                    role_rows = role_rows[:-1]
                for i in role_rows:
                    reads.append((q, ("A", int(i), j)))
                    key = ("P", int(i), k)
                    assert key not in written
                    written.add(key)
                    Pinv[(int(i), k)] = Pinv0.get((int(i), k), np.zeros((T, T))) + t0(int(i), j) @ X
                continue
            ti, tk = it["ti"], it["tk"]
            src = srcs[it["src"]:it["src"] + it["nsrc"]]
            if broken and mut == "trail_skips_last_source":
                src = src[:-1]
            if it["type"] == 1:  # trailing tile
                assert lt(ti, tk) in live and ("A", ti, tk) not in written
                written.add(("A", ti, tk))
                acc = t0(ti, tk).copy()
                for c in src:
                    reads += [(q, ("A", ti, int(c))), (q, ("A", tk, int(c)))]
                    assert done_col[c] >= 0 and done_col[c] < l
                    acc -= t0(ti, int(c)) @ t0(tk, int(c)).T
                tile(ti, tk)[:] = acc
                continue
            # panel tile of column tk
            D = t0(tk, tk).copy()
            X = t0(ti, tk).copy() if ti != tk else None
            reads.append((q, ("A", tk, tk)))
            for e in src:
                c, xf = int(e) & 0xffff, bool(int(e) >> 16)
                if broken and mut == "panel_ignores_own_tile":
                    xf = False
                reads.append((q, ("A", tk, c)))
                if X is not None and xf:
                    reads.append((q, ("A", ti, c)))
                assert done_col[c] >= 0 and done_col[c] < l
                D -= t0(tk, c) @ t0(tk, c).T
                if X is not None and xf:
                    X -= t0(ti, c) @ t0(tk, c).T
            Lkk = np.linalg.cholesky(D)
            if ti == tk:
                Linv[tk] = np.linalg.inv(Lkk)
                written.add(("Linv", tk))
                done_col[tk] = l
            else:
                assert ("A", ti, tk) not in written
                written.add(("A", ti, tk))
                tile(ti, tk)[:] = np.linalg.solve(Lkk, X.T).T
        # no item reads what ANOTHER item of the same launch writes (on the GPU it might see either value)
        for q, key in reads:
            assert key not in written, f"launch {l}: item {q} reads {key}, which another item of the launch writes"
    assert (done_col >= 0).all()
    z = A[N, :N].copy()  # forward-substituted rhs
    w = np.concatenate([Linv[i].T @ z[i * T:(i + 1) * T] for i in range(nt)])
    if P["use_pinv"]:
        y = w.copy()
        for (i, k), Pt in sorted(Pinv.items(), key=lambda e: e[0]):  # (a fixed order of summation, whatever order the items ran in)
            y[k * T:(k + 1) * T] -= Pt.T @ w[i * T:(i + 1) * T]
    else:
        y = np.zeros(N)
        ss, sr = P["struct_start"], P["struct_rows"]
        lev = P["level"]
        for b in range(len(P["back_start"]) - 1):
            cols = P["back_cols"][P["back_start"][b]:P["back_start"][b + 1]]
            for j in cols:
                v = z[j * T:(j + 1) * T].copy()
                for i in sr[ss[j]:ss[j + 1]]:
                    if mut == "back_skips_last_column" and i == nt - 1:
                        continue
                    if i < nt:
                        assert lev[i] > lev[j]
                        v -= tile(int(i), int(j)).T @ y[i * T:(i + 1) * T]
                y[j * T:(j + 1) * T] = Linv[int(j)].T @ v
    return y[:n]
