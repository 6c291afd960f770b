"""The pair stages without a GPU: the fp64 restatement (tests/numpy_retrieval.py) and the host-side functions of
mpsfm_amd/extraction/pairs against the fixture computed by the reference's own code (tests/golden/make_golden_retrieval.py), the
entry point's argument checks, which come before any device is touched, the empty calls, the parsers and the files.

The fixture rule: on every row whose decision margin exceeds tau32 = 4 D 2^-24 the float32 reference and the fp64 restatement list
the same db images in the same order; such rows are at least 95 % of every case."""

import ctypes as C
import importlib
import json
import os

import numpy as np
import pytest

import numpy_retrieval as NR
from mpsfm_amd import capi
from mpsfm_amd.extraction import pairs as P
from mpsfm_amd.utils.parsers import parse_image_lists, parse_retrieval, read_unique_pairs

R = importlib.import_module("mpsfm_amd.extraction.pairs.pairs_from_retrieval")  # the package binds that name to the module's main()
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_retrieval.npz"))
DESC_CASES = ["same20", "same5", "disjoint", "clipped", "quirk"]
NAME_CASES = json.loads(str(GOLD["name_cases"]))
HOST_CASES = json.loads(str(GOLD["host_cases"]))
EINVAL, ENODEVICE = -1, -2


def desc_case(tag):
    """query, db, query names, db names, num_matched, the reference's pairs [n, 2] and their float32 scores"""
    return (GOLD[f"{tag}_query"], GOLD[f"{tag}_db"], GOLD[f"{tag}_query_names"].tolist(), GOLD[f"{tag}_db_names"].tolist(),
            int(GOLD[f"{tag}_num_matched"]), GOLD[f"{tag}_pairs"], GOLD[f"{tag}_scores"])


def name_case(case):
    """the same for a case given by names and mappings: descriptors gathered as pairs_from_retrieval.main gathers them"""
    maps = {m: dict(zip(GOLD[f"map_{m}_names"].tolist(), GOLD[f"map_{m}_desc"])) for m in ("queries", "dbA", "dbB")}
    where = {}
    for m in case["dbs"] or ["queries"]:
        where.update({n: maps[m] for n in maps[m]})
    q = np.stack([maps["queries"][n] for n in case["query_names"]])
    db = np.stack([where[n][n] for n in case["db_names"]])
    qn, dn = case["query_names"], case["db_names"]
    pairs = np.array([(qn.index(a), dn.index(b)) for a, b in case["pairs"]], np.int64).reshape(-1, 2)
    return q, db, qn, dn, case["num_matched"], pairs, None


def mappings(case):
    """descriptors, db_descriptors of pairs_from_retrieval.main for a name case"""
    maps = {m: {n: {"global_descriptor": d} for n, d in zip(GOLD[f"map_{m}_names"].tolist(), GOLD[f"map_{m}_desc"])} for m in ("queries", "dbA", "dbB")}
    return maps["queries"], None if case["dbs"] is None else [maps[m] for m in case["dbs"]]


ALL_CASES = [(t, None) for t in DESC_CASES] + [(c["tag"], c) for c in NAME_CASES]


def load_case(tag, case):
    return desc_case(tag) if case is None else name_case(case)


def assert_lists_agree(tag, idx, val, cnt, margin, q, pairs, scores, tol, floor):
    """on every row above tol: the same db images in the same order, scores within tol"""
    sure = margin > tol
    assert sure.mean() >= floor, (tag, sure.mean())
    for i in np.flatnonzero(sure):
        mine = pairs[:, 0] == i
        assert pairs[mine, 1].tolist() == idx[i, :cnt[i]].tolist(), (tag, i)
        if scores is not None and mine.any():
            assert np.abs(scores[mine].astype(np.float64) - val[i, :cnt[i]]).max() <= tol
        assert (idx[i, cnt[i]:] == -1).all() and (val[i, cnt[i]:] == 0).all()


@pytest.mark.parametrize("tag,case", ALL_CASES, ids=[t for t, _ in ALL_CASES])
def test_restatement_lists_what_the_reference_lists(tag, case):
    q, db, qn, dn, num, pairs, scores = load_case(tag, case)
    assert q.dtype == np.float16 and db.dtype == np.float16
    k = min(num, len(q))
    qi, di = NR.name_ids(qn, dn)
    idx, val, cnt, margin = NR.retrieve_topk(q, db, k, 0.0, qi, di)
    assert_lists_agree(tag, idx, val, cnt, margin, q, pairs, scores, NR.tau(q.shape[1], NR.TAU32_EPS), 0.95)
    assert len(pairs) > 0 and (np.diff(pairs[:, 0]) >= 0).all()  # row-major
    if tag == "clipped":
        assert k == 40 and cnt.max() < 39
    if tag == "quirk":
        assert k == 12 < num <= len(db)


@pytest.mark.parametrize("tag,case", ALL_CASES, ids=[t for t, _ in ALL_CASES])
def test_pairs_from_score_matrix_lists_what_the_reference_lists_and_keeps_its_arguments(tag, case):
    q, db, qn, dn, num, pairs, _ = load_case(tag, case)
    sim = NR.similarities(q, db)
    _, _, _, margin = NR.retrieve_topk(q, db, min(num, len(q)), 0.0, *NR.name_ids(qn, dn))
    invalid = np.array(qn)[:, None] == np.array(dn)[None]
    sim0, invalid0 = sim.copy(), invalid.copy()
    got = R.pairs_from_score_matrix(sim, invalid, num, min_score=0)
    assert np.array_equal(sim, sim0) and np.array_equal(invalid, invalid0)
    sure = margin > NR.tau(q.shape[1], NR.TAU32_EPS)
    want = [(int(i), int(j)) for i, j in pairs if sure[i]]
    assert [p for p in got if sure[p[0]]] == want
    sim32 = sim.astype(np.float32)  # float32 scores and torch tensors are taken too
    import torch

    assert R.pairs_from_score_matrix(torch.from_numpy(sim32), invalid, num, min_score=0) == R.pairs_from_score_matrix(sim32, invalid, num, min_score=0)


def test_pairs_from_score_matrix_order_ties_and_the_missing_score_test():
    s = np.array([[0.5, 0.75, 0.5, -0.25, 0.75], [0.0, -1.0, 0.0, 0.0, 1.0]])
    inv = np.zeros((2, 5), bool)
    inv[1, 4] = True
    assert R.pairs_from_score_matrix(s, inv, 5, None) == [(0, 1), (0, 4), (1, 0), (1, 2)]  # k = min(5, 2 rows): the quirk
    assert R.pairs_from_score_matrix(s, inv, 1, 0) == [(0, 1), (1, 0)]
    assert R.pairs_from_score_matrix(np.vstack([s, s, s]), np.vstack([inv, inv, inv]), 5, 0)[:8] == [(0, 1), (0, 4), (0, 0), (0, 2), (1, 0), (1, 2), (1, 3), (2, 1)]
    assert R.pairs_from_score_matrix(np.vstack([s, s, s]), np.vstack([inv, inv, inv]), 5, None)[4] == (0, 3)
    with pytest.raises(ValueError, match="torch.topk raises"):
        R.pairs_from_score_matrix(np.zeros((7, 3)), np.zeros((7, 3), bool), 4)


# ---- branches of the restatement ------------------------------------------------------------------------------------------------
def test_restatement_ties_short_rows_excluded_rows_and_no_score_test():
    d = (np.array([[4, 0, 0], [4, 0, 0], [2, 4, 0], [-4, 0, 0], [4, 0, 0], [0, 0, 0]]) / 8.0).astype(np.float32)
    q = (np.array([[4, 0, 0], [0, 4, 0]]) / 8.0).astype(np.float32)
    idx, val, cnt, margin = NR.retrieve_topk(q, d, 2)
    assert idx.tolist() == [[0, 1], [2, 0]] and val[0].tolist() == [0.25, 0.25] and cnt.tolist() == [2, 2]
    assert margin[0] == 0.0  # a tie inside the first k + 1
    idx, val, cnt, margin = NR.retrieve_topk(q, d, 6)  # k > n_valid: the score test decides, zeros are kept
    assert idx.tolist() == [[0, 1, 4, 2, 5, -1], [2, 0, 1, 3, 4, 5]] and cnt.tolist() == [5, 6] and margin.tolist() == [0.0, 0.0]
    assert val[0].tolist() == [0.25, 0.25, 0.25, 0.125, 0.0, 0.0]
    idx, val, cnt, _ = NR.retrieve_topk(q, d, 6, None)  # no score test: negative similarities are listed
    assert idx[0].tolist() == [0, 1, 4, 2, 5, 3] and val[0, 5] == -0.25 and cnt.tolist() == [6, 6]
    idx, val, cnt, margin = NR.retrieve_topk(q, d, 3, 0.0, np.array([7, 8]), np.array([7, 1, 7, 2, 7, 7]))  # several columns share the id
    assert idx.tolist() == [[1, -1, -1], [2, 0, 1]] and cnt.tolist() == [1, 3]
    idx, val, cnt, margin = NR.retrieve_topk(q, d, 3, 0.0, np.array([7, 8]), np.full(6, 7))  # every column excluded
    assert idx[0].tolist() == [-1, -1, -1] and cnt.tolist() == [0, 3] and margin[0] == np.inf
    idx, val, cnt, margin = NR.retrieve_topk(q, d, 1, 0.25)  # a similarity equal to min_score stays
    assert idx.tolist() == [[0], [2]] and cnt.tolist() == [1, 1] and margin[0] == 0.0
    assert NR.retrieve_topk(q, d[:0], 3)[2].tolist() == [0, 0] and NR.retrieve_topk(q[:0], d, 3)[0].shape == (0, 3)
    assert NR.pairs_of(*NR.retrieve_topk(q, d, 2)[0:3:2]) == [(0, 0), (0, 1), (1, 2), (1, 0)]


# ---- the entry point without a device ---------------------------------------------------------------------------------------------
Pt = lambda a: None if a is None else a.ctypes.data  # noqa: E731


def options(**kw):
    o = capi.CRetrievalOptions()
    capi.lib().mpsfm_retrieval_default_options(C.addressof(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_default_options_are_the_reference_s():
    o = capi.CRetrievalOptions(1, 0, 5.0, 3, 1, 5)
    capi.lib().mpsfm_retrieval_default_options(C.addressof(o))
    assert (o.num_select, o.use_min_score, o.min_score, o.column_ranges, o.inputs_on_device, o.stream) == (20, 1, 0.0, 0, 0, None)
    capi.lib().mpsfm_retrieval_default_options(None)


def test_retrieve_topk_checks_arguments_before_any_device():
    L = capi.lib()
    q, d = np.ones((3, 4), np.float32), np.ones((5, 4), np.float32)
    qi, di = np.zeros(3, np.int32), np.zeros(5, np.int32)
    idx, val, cnt = np.zeros((3, 2), np.int32), np.zeros((3, 2)), np.zeros(3, np.int32)

    def call(nq=3, nd=5, dim=4, a=q, b=d, ia=None, ib=None, opts=options(num_select=2), ii=idx, vv=val, cc=cnt, info=None):
        return L.mpsfm_retrieve_topk(nq, nd, dim, Pt(a), Pt(b), Pt(ia), Pt(ib), None if opts is None else C.addressof(opts), 0, Pt(ii), Pt(vv), Pt(cc),
                                     None if info is None else C.addressof(info))

    assert call(nq=-1) == EINVAL and call(nd=-1) == EINVAL
    assert call(dim=0) == EINVAL and call(dim=65537) == EINVAL and call(dim=-3) == EINVAL
    assert call(nq=(1 << 24) + 1) == EINVAL and call(nd=(1 << 24) + 1) == EINVAL
    for ptr in ("a", "b", "ii", "vv", "cc"):
        assert call(**{ptr: None}) == EINVAL, ptr
    assert b"NULL" in L.mpsfm_last_error()
    for k in (0, -1, 129, 6):  # outside 1 .. 128, or more than the 5 db rows
        assert call(opts=options(num_select=k)) == EINVAL, k
    assert call(opts=None) == EINVAL  # the default of 20 exceeds 5 db rows
    assert call(ia=qi) == EINVAL and call(ib=di) == EINVAL
    assert b"both or neither" in L.mpsfm_last_error()
    assert call(opts=options(num_select=2, column_ranges=-1)) == EINVAL
    for bad in (np.nan, np.inf, -np.inf):
        assert call(opts=options(num_select=2, min_score=bad)) == EINVAL
        assert call(opts=options(num_select=2, min_score=bad, use_min_score=0)) == EINVAL
        x = q.copy(); x[2, 3] = bad
        assert call(a=x) == EINVAL
        y = d.copy(); y[4, 3] = bad
        assert call(b=y) == EINVAL
        assert b"non-finite" in L.mpsfm_last_error()
        assert call(nq=5, a=y, b=y, ii=np.zeros((5, 2), np.int32), vv=np.zeros((5, 2)), cc=np.zeros(5, np.int32)) == EINVAL  # query == db
    # empty sides: no device needed
    idx[:], val[:], cnt[:] = 7, 7.0, 7
    info = capi.CRetrievalInfo(5, 5, 5, 5.0, 5)
    assert call(nd=0, b=None, info=info) == 0 and (idx == -1).all() and (val == 0).all() and (cnt == 0).all()
    assert (info.num_pairs, info.num_launches, info.num_syncs, info.ms, info.column_ranges) == (0, 0, 0, 0.0, 0)
    assert call(nd=0, b=None, opts=options(num_select=128), ii=np.zeros((3, 128), np.int32), vv=np.zeros((3, 128))) == 0  # no nd to exceed
    assert call(nq=0, a=None, ii=None, vv=None, cc=None) == 0
    assert call(nq=0, nd=0, a=None, b=None, ii=None, vv=None, cc=None) == 0
    # valid calls: computed with a device, refused loudly without one
    want = 0 if capi.device_count() > 0 else ENODEVICE
    assert call() == want and call(ia=qi, ib=di) == want
    assert call(dim=65536, a=np.ones((3, 65536), np.float32), b=np.ones((5, 65536), np.float32)) == want


def test_wrapper_types_empty_calls_and_refusals_without_a_device():
    import torch

    e, d = np.zeros((0, 8), np.float32), np.ones((3, 8), np.float16)
    idx, val, cnt, info = capi.retrieve_topk(d, e, 2, return_info=True)
    assert idx.dtype == np.int64 and val.dtype == np.float64 and cnt.dtype == np.int64
    assert idx.tolist() == [[-1, -1]] * 3 and val.tolist() == [[0.0, 0.0]] * 3 and cnt.tolist() == [0, 0, 0]
    assert info == dict(num_pairs=0, num_launches=0, num_syncs=0, ms=0.0, column_ranges=0)
    idx, val, cnt = capi.retrieve_topk(e, d, 2, query_ids=np.zeros(0, np.int32), db_ids=np.zeros(3, np.int32))
    assert idx.shape == (0, 2) and val.shape == (0, 2) and cnt.shape == (0,)
    idx, _, _ = capi.retrieve_topk(torch.zeros(0, 8), torch.ones(3, 8), 2, min_score=None)
    assert idx.shape == (0, 2)
    with pytest.raises(TypeError):
        capi.retrieve_topk(np.ones((3, 8)), np.ones((3, 8)), 2)
    with pytest.raises(TypeError):
        capi.retrieve_topk(torch.ones(3, 8, dtype=torch.float64), torch.ones(3, 8, dtype=torch.float64), 2)
    with pytest.raises(ValueError):
        capi.retrieve_topk(d, np.ones((3, 7), np.float32), 2)
    with pytest.raises(ValueError):
        capi.retrieve_topk(d, d, 2, query_ids=np.zeros(3, np.int32))
    with pytest.raises(ValueError):
        capi.retrieve_topk(d, d, 2, query_ids=np.zeros(2, np.int32), db_ids=np.zeros(3, np.int32))
    for k in (0, 4, 129):
        with pytest.raises(capi.MpsfmHipError) as err:
            capi.retrieve_topk(d, d, k)
        assert err.value.code == EINVAL
    assert R.pairs_from_descriptors(e, d, 5) == [] and R.pairs_from_descriptors(d, d, 0) == []
    if capi.device_count() == 0:  # with a device the same calls are computed: tests/test_gpu_retrieval.py
        feats = {f"im{i}": {"global_descriptor": d[i]} for i in range(3)}
        for call in (lambda: capi.retrieve_topk(d, d, 2), lambda: R.pairs_from_descriptors(d, d, 2), lambda: P.pairs_from_retrieval(feats, None, 2)):
            with pytest.raises(capi.MpsfmHipError) as err:
                call()
            assert err.value.code == ENODEVICE


def test_the_quirk_and_the_cap_are_value_errors():
    q, d = np.ones((12, 8), np.float32), np.ones((5, 8), np.float32)
    with pytest.raises(ValueError, match="QUERY images"):
        R.pairs_from_descriptors(q, d, 20)  # min(20, 12 queries) = 12 > 5 db images: torch.topk raises in the reference
    with pytest.raises(ValueError, match="QUERY images"):
        P.pairs_from_retrieval({f"q{i}": {"global_descriptor": q[i]} for i in range(12)}, None, 20,
                               db_descriptors={f"d{i}": {"global_descriptor": d[i]} for i in range(5)})
    big = np.ones((130, 4), np.float32)
    with pytest.raises(ValueError, match="cap of 128"):
        R.pairs_from_descriptors(big, big, 129)
    assert capi.MAX_NUM_SELECT == 128
    with pytest.raises(ValueError, match="database image"):
        P.pairs_from_retrieval({"a": {"global_descriptor": q[0]}}, None, 1, db_descriptors=[{}])
    with pytest.raises(ValueError, match="prefix"):
        P.pairs_from_retrieval({"a": {"global_descriptor": q[0]}}, None, 1, query_prefix="zz")


# ---- names, files, parsers --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NAME_CASES, ids=[c["tag"] for c in NAME_CASES])
def test_parse_names_and_the_last_mapping_wins(case):
    descriptors, dbs = mappings(case)
    name2db = R._named(descriptors if dbs is None else dbs)
    assert R.parse_names(case["db_prefix"], case["db_list"], list(name2db)) == case["db_names"]
    assert R.parse_names(case["query_prefix"], case["query_list"], list(descriptors)) == case["query_names"]
    if dbs is not None:
        assert name2db["shared/s0.jpg"] is dbs[-1] and "shared/s0.jpg" in dbs[0]
    with pytest.raises(ValueError):
        R.parse_names(None, 5, [])
    assert R.parse_names(None, (n for n in ["b", "a"]), ["x"]) == ["b", "a"] and R.parse_names(None, None, ["x"]) == ["x"]


def test_parse_names_reads_a_list_file(tmp_path):
    (tmp_path / "list_a.txt").write_text("# header\nim1.jpg PINHOLE 4 3\n\nim0.jpg\n")
    (tmp_path / "list_b.txt").write_text("im7.jpg\n")
    assert R.parse_names(None, tmp_path / "list_a.txt", ["x"]) == ["im1.jpg", "im0.jpg"]
    assert parse_image_lists(str(tmp_path / "list_*.txt")) == ["im1.jpg", "im0.jpg", "im7.jpg"]
    assert P.pairs_from_sequential(None, image_list=tmp_path / "list_a.txt", overlap=1) == [("im0.jpg", "im1.jpg")]
    with pytest.raises(ValueError):
        parse_image_lists(tmp_path / "none*.txt")


@pytest.mark.parametrize("n", range(len(HOST_CASES)))
def test_sequential_and_exhaustive_pairs_and_files_byte_for_byte(n, tmp_path):
    case = HOST_CASES[n]
    out = tmp_path / "pairs.txt"
    if case["kind"] == "sequential":
        got = P.pairs_from_sequential(out, image_list=case["names"], overlap=case["overlap"], quadratic_overlap=case["quadratic_overlap"])
        feats = {name: {} for name in case["names"]}
        assert P.pairs_from_sequential(None, features=feats, overlap=case["overlap"], quadratic_overlap=case["quadratic_overlap"]) == got
    else:
        got = P.pairs_from_exhaustive(out, image_list=case["names"], ref_list=case["ref"])
        feats, refs = {name: {} for name in case["names"]}, None if case["ref"] is None else {name: {} for name in case["ref"]}
        assert P.pairs_from_exhaustive(None, features=feats, ref_features=refs) == got
    assert [list(p) for p in got] == case["pairs"]
    assert out.read_bytes() == case["text"].encode()
    with pytest.raises(ValueError):
        P.pairs_from_sequential(None)
    with pytest.raises(ValueError):
        P.pairs_from_exhaustive(None, image_list=3)


def test_host_cases_cover_what_they_should():
    seq = [c for c in HOST_CASES if c["kind"] == "sequential"]
    exh = [c for c in HOST_CASES if c["kind"] == "exhaustive"]
    assert {(len(c["names"]), c["overlap"], c["quadratic_overlap"]) for c in seq} == {(n, o, q) for n in (1, 2, 9) for o in (1, 3) for q in (True, False)}
    assert {(len(c["names"]), c["ref"] is None) for c in exh} == {(n, r) for n in (1, 2, 9) for r in (True, False)}
    assert any(c["text"] == "" for c in seq) and any(len(c["pairs"]) == 36 for c in exh)


def test_parse_retrieval_and_read_unique_pairs(tmp_path):
    path = tmp_path / "pairs.txt"
    path.write_text("b a\n\na b\nc a\na c\nb c\n\nb a\nd d\n")
    assert parse_retrieval(path) == {"b": ["a", "c", "a"], "a": ["b", "c"], "c": ["a"], "d": ["d"]}
    assert list(parse_retrieval(path)) == ["b", "a", "c", "d"]
    assert read_unique_pairs(path) == [["a", "b"], ["a", "c"], ["b", "c"], ["d"]]
    path.write_text("x y")  # what the pair stages write: no trailing newline
    assert parse_retrieval(path) == {"x": ["y"]} and read_unique_pairs(path) == [["x", "y"]]
    path.write_text("")
    assert parse_retrieval(path) == {} and read_unique_pairs(path) == []


@pytest.mark.parametrize("case", NAME_CASES, ids=[c["tag"] for c in NAME_CASES])
def test_main_writes_the_reference_s_file(case, tmp_path, monkeypatch):
    """main() with the device call replaced by the restatement: names, ids, the pair names and the file are the host's"""
    q, db, qn, dn, num, pairs, _ = name_case(case)
    _, _, _, margin = NR.retrieve_topk(q, db, min(num, len(q)), 0.0, *NR.name_ids(qn, dn))
    assert (margin > NR.tau(q.shape[1], NR.TAU32_EPS)).all()  # every row of the name cases is decided
    seen = {}

    def restated(query, dbd, k, min_score=0.0, query_ids=None, db_ids=None, **kw):
        seen.update(k=k, min_score=min_score, ids=(query_ids.tolist(), db_ids.tolist()), dtype=query.dtype)
        return NR.retrieve_topk(query, dbd, k, min_score, query_ids, db_ids)[:3]

    monkeypatch.setattr(capi, "retrieve_topk", restated)
    descriptors, dbs = mappings(case)
    out = tmp_path / "pairs.txt"
    got = P.pairs_from_retrieval(descriptors, out, case["num_matched"], query_prefix=case["query_prefix"], query_list=case["query_list"],
                                 db_prefix=case["db_prefix"], db_list=case["db_list"], db_descriptors=dbs)
    assert [list(p) for p in got] == case["pairs"]
    assert out.read_bytes() == case["text"].encode()
    assert seen["k"] == min(case["num_matched"], len(qn)) and seen["min_score"] == 0 and seen["dtype"] == np.float16
    qi, di = seen["ids"]
    assert [[a == b for b in di] for a in qi] == [[a == b for b in dn] for a in qn]  # the ids mirror name equality
    one = dbs[0] if dbs else None
    if dbs and len(dbs) == 1:
        assert P.pairs_from_retrieval(descriptors, None, case["num_matched"], db_descriptors=one) is not None
