"""Descriptor matching without a GPU: the fp64 restatement (tests/numpy_descriptor_matches.py) against the fixture computed by
the reference's own NearestNeighbor / NNs_sparse (tests/golden/make_golden_descriptor_matches.py), the entry points' argument
checks, which come before any device is touched, and the wrappers' handling of empty inputs.

The fixture rule: on every row whose decision margin exceeds tau32 = 4 D 2^-24 (sampled: 8 C 2^-24), the float32 reference and
the fp64 restatement must take the same decision; such rows are at least 99 % of every case."""

import ctypes as C
import os

import numpy as np
import pytest

import numpy_descriptor_matches as NM
from mpsfm_amd import capi
from mpsfm_amd.extraction.pairwise import NearestNeighbor, NNs_sparse, match_descriptors

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_descriptor_matches.npz"))
EINVAL, ENODEVICE = -1, -2


@pytest.mark.parametrize("case", ["plain", "ratio", "ratio_distance", "no_mutual"])
def test_restatement_equals_the_reference_matcher(case):
    d0, d1 = GOLD["desc0"], GOLD["desc1"]
    assert d0.dtype == np.float16 and d1.dtype == np.float16
    ratio, distance, mutual = float(GOLD[f"{case}_ratio"]), float(GOLD[f"{case}_distance"]), bool(GOLD[f"{case}_mutual"])
    m, s, margin = NM.match_descriptors(d0, d1, ratio or None, distance or None, mutual)
    t32 = NM.tau(d0.shape[1], NM.TAU32_EPS)
    sure = margin > t32
    assert sure.mean() >= 0.99
    assert np.array_equal(m[sure], GOLD[f"{case}_matches0"][sure])
    assert np.abs(s - GOLD[f"{case}_scores0"])[sure].max() <= t32
    assert (m >= 0).mean() >= 0.2


def test_restatement_equals_the_reference_sampled_leg():
    g = {k: GOLD[f"maps_{k}"] for k in ("map0", "map1", "conf0", "conf1", "kps0", "kps1", "matches0", "scores0")}
    m, s, margin = NM.nns_sparse(g["map0"], g["map1"], g["conf0"], g["conf1"], g["kps0"], g["kps1"], float(GOLD["maps_scores_thresh"]))
    t32 = 8.0 * g["map0"].shape[2] * NM.TAU32_EPS
    sure = margin > t32
    assert sure.mean() >= 0.99
    assert np.array_equal(m[sure], g["matches0"][sure])
    assert np.abs(s - g["scores0"])[sure].max() <= t32
    assert (m >= 0).mean() >= 0.2 and (g["kps0"].astype(np.float32).astype(np.float64) != g["kps0"]).any()


def test_restatement_ties_go_to_the_lowest_index_and_duplicates_tie_bitwise():
    rng = np.random.default_rng(3)
    d1 = rng.normal(size=(9, 7)).astype(np.float32)
    d1[6] = d1[2]
    d0 = np.stack([d1[2] * np.float32(0.5), d1[4]])
    sim = NM.similarities(d0, d1)
    assert sim[0, 2] == sim[0, 6]
    v1, i1, v2 = NM.top2(sim)
    assert i1[0] == 2 and v2[0] == v1[0]
    m, s, margin = NM.match_descriptors(d0, d1, do_mutual_check=False)
    assert m[0] == 2 and margin[0] == 0.0 and margin[1] > 0


def test_restatement_single_descriptor_and_single_channel_branches():
    one = np.array([[0.5]], np.float32)
    m, s, margin = NM.match_descriptors(one, one, ratio_threshold=0.5)  # N == 1 on both sides: no ratio test
    assert m.tolist() == [0] and s.tolist() == [0.625] and margin[0] == np.inf
    d0, d1 = np.array([[1.0], [-1.0], [0.5]], np.float32), np.array([[1.0], [-0.5]], np.float32)
    m, s, _ = NM.match_descriptors(d0, d1)  # dim == 1
    assert m.tolist() == [0, 1, -1] and s.tolist() == [1.0, 0.75, 0.75]
    m, _, _ = NM.match_descriptors(d0, d1[:1], ratio_threshold=0.5, do_mutual_check=False)  # one column: the ratio test is skipped
    assert m.tolist() == [0, 0, 0]
    m, _, _ = NM.match_descriptors(d0, d1, ratio_threshold=0.5, do_mutual_check=False)
    assert m.tolist() == [0, 1, -1]  # row 1: dist 1 against 0.25 * 4, on the boundary: kept; row 2: dist 1 against 0.25 * 2.5


def test_restatement_sampling_is_the_pixel_on_pixels_and_zero_outside():
    rng = np.random.default_rng(4)
    m = rng.random((5, 6, 3)).astype(np.float32)
    k = np.array([[0, 0], [5, 4], [2, 3], [5.5, 4.0], [-1.0, 2.0], [7.0, 1.0], [2.5, 1.0]])
    s = NM.sample_map(m, k)
    assert np.array_equal(s[0], m[0, 0]) and np.array_equal(s[1], m[4, 5]) and np.array_equal(s[2], m[3, 2])
    assert np.array_equal(s[3], 0.5 * m[4, 5].astype(np.float64)) and (s[4] == 0).all() and (s[5] == 0).all()
    assert np.array_equal(s[6], 0.5 * m[1, 2].astype(np.float64) + 0.5 * m[1, 3].astype(np.float64))


def _lib():
    L = capi.lib()
    return L


P = lambda a: None if a is None else a.ctypes.data  # noqa: E731


def test_default_options_are_the_reference_s():
    o = capi.CMatchOptions(1.0, 1.0, 1.0, 0, 1, 5)
    _lib().mpsfm_match_default_options(C.addressof(o))
    assert (o.ratio_threshold, o.distance_threshold, o.score_threshold, o.mutual_check, o.inputs_on_device, o.stream) == (0, 0, 0, 1, 0, None)


def test_match_descriptors_checks_arguments_before_any_device():
    L = _lib()
    d0, d1 = np.ones((3, 4), np.float32), np.ones((2, 4), np.float32)
    m, s = np.zeros(3, np.int32), np.zeros(3)

    def call(n0=3, n1=2, dim=4, a=d0, b=d1, opts=None, mm=m, ss=s):
        return L.mpsfm_match_descriptors(n0, n1, dim, P(a), P(b), None if opts is None else C.addressof(opts), 0, P(mm), P(ss), None)

    assert call(n0=-1) == EINVAL and call(n1=-1) == EINVAL
    assert call(dim=0) == EINVAL and call(dim=1025) == EINVAL and call(dim=-3) == EINVAL
    assert call(n0=(1 << 24) + 1) == EINVAL and call(n1=(1 << 24) + 1) == EINVAL
    assert call(a=None) == EINVAL and call(b=None) == EINVAL and call(mm=None) == EINVAL and call(ss=None) == EINVAL
    for bad in (np.nan, np.inf, -np.inf):
        x = d0.copy(); x[2, 3] = bad
        assert call(a=x) == EINVAL
        y = d1.copy(); y[0, 0] = bad
        assert call(b=y) == EINVAL
        assert b"non-finite" in L.mpsfm_last_error()
        for field in ("ratio_threshold", "distance_threshold", "score_threshold"):
            o = capi._match_options(None, None, None, True)
            setattr(o, field, bad)
            assert call(opts=o) == EINVAL
    # either side empty: all -1 / 0 without a device
    m[:], s[:] = 7, 7.0
    assert call(n1=0, b=None) == 0 and m.tolist() == [-1, -1, -1] and s.tolist() == [0, 0, 0]
    assert call(n0=0, a=None, mm=None, ss=None) == 0
    info = capi.CMatchInfo(5, 5.0, 0)
    assert L.mpsfm_match_descriptors(3, 0, 4, P(d0), None, None, 0, P(m), P(s), C.addressof(info)) == 0 and info.num_matches == 0 and info.ms == 0
    # a valid call: computed with a device, refused loudly without one
    assert call() == (0 if capi.device_count() > 0 else ENODEVICE)
    assert call(opts=capi._match_options(0.8, 0.7, None, False)) == (0 if capi.device_count() > 0 else ENODEVICE)


def test_match_map_descriptors_checks_arguments_before_any_device():
    L = _lib()
    mp, cf = np.ones((3, 4, 5), np.float32), np.ones((3, 4), np.float32)
    k0, k1 = np.ones((2, 2)), np.ones((3, 2))
    m, s = np.zeros(2, np.int32), np.zeros(2)

    def call(m0=mp, c0=cf, H0=3, W0=4, m1=mp, c1=cf, H1=3, W1=4, Cc=5, n0=2, kk0=k0, n1=3, kk1=k1, opts=None, mm=m, ss=s):
        return L.mpsfm_match_map_descriptors(P(m0), P(c0), H0, W0, P(m1), P(c1), H1, W1, Cc, n0, P(kk0), n1, P(kk1),
                                             None if opts is None else C.addressof(opts), 0, P(mm), P(ss), None)

    assert call(n0=-1) == EINVAL and call(n1=-1) == EINVAL and call(n0=(1 << 24) + 1) == EINVAL
    assert call(Cc=0) == EINVAL and call(Cc=1025) == EINVAL
    for dims in (dict(H0=1), dict(W0=1), dict(H1=1), dict(W1=0), dict(H0=-4)):  # the reference divides by zero there
        assert call(**dims) == EINVAL
    for ptr in ("m0", "c0", "m1", "c1", "kk0", "kk1", "mm", "ss"):
        assert call(**{ptr: None}) == EINVAL
    for bad in (np.nan, np.inf):
        x = mp.copy(); x[2, 3, 4] = bad
        assert call(m0=x) == EINVAL and call(m1=x) == EINVAL
        c = cf.copy(); c[0, 0] = bad
        assert call(c0=c) == EINVAL and call(c1=c) == EINVAL
        k = k1.copy(); k[2, 1] = bad
        assert call(kk1=k) == EINVAL
        o = capi._match_options(None, None, None, True)
        o.score_threshold = bad
        assert call(opts=o) == EINVAL
    assert call(kk0=np.array([[1e300, 0.0], [0.0, 0.0]])) == EINVAL  # finite as float64, infinite as float32
    m[:], s[:] = 7, 7.0
    assert call(n1=0, kk1=None) == 0 and m.tolist() == [-1, -1] and s.tolist() == [0, 0]
    assert call(n0=0, kk0=None, mm=None, ss=None) == 0
    assert call() == (0 if capi.device_count() > 0 else ENODEVICE)


def test_wrappers_return_types_and_empty_inputs_without_a_device():
    import torch

    e, d = np.zeros((0, 8), np.float32), np.ones((3, 8), np.float32)
    for a, b, n in ((e, d, 0), (d, e, 3), (e, e, 0)):
        m, s = match_descriptors(a, b)
        assert m.dtype == np.int64 and s.dtype == np.float64 and m.tolist() == [-1] * n and s.tolist() == [0.0] * n
        m, s, info = capi.match_descriptors(a, b, return_info=True)
        assert info == dict(num_matches=0, ms=0.0, column_ranges=0)
    nn = NearestNeighbor({"ratio_threshold": 0.8})
    assert nn.conf == {"ratio_threshold": 0.8, "distance_threshold": None, "do_mutual_check": True, "require_download": False}
    assert set(NearestNeighbor.default_conf) == {"ratio_threshold", "distance_threshold", "do_mutual_check", "require_download"}
    out = nn({"descriptors0": np.ones((2, 8, 3), np.float16), "descriptors1": np.ones((2, 8, 0), np.float16)})
    assert isinstance(out["matches0"], np.ndarray) and out["matches0"].shape == (2, 3) and (out["matches0"] == -1).all()
    assert out["matching_scores0"].shape == (2, 3) and (out["matching_scores0"] == 0).all()
    out = nn({"descriptors0": torch.ones(1, 8, 0), "descriptors1": torch.ones(1, 8, 4)})
    assert isinstance(out["matches0"], torch.Tensor) and out["matches0"].dtype == torch.int64 and out["matches0"].shape == (1, 0)
    assert out["matching_scores0"].dtype == torch.float64
    with pytest.raises(TypeError):
        nn({"descriptors0": np.ones((1, 8, 3)), "descriptors1": np.ones((1, 8, 3))})
    with pytest.raises(TypeError):
        match_descriptors(np.ones((3, 8)), np.ones((3, 8)))
    with pytest.raises(ValueError):
        match_descriptors(np.ones((3, 8), np.float32), np.ones((3, 7), np.float32))
    with pytest.raises(AssertionError):
        nn({"descriptors0": np.ones((1, 8, 3), np.float32)})
    mp, cf = np.ones((4, 5, 6), np.float32), np.ones((4, 5), np.float32)
    m, s = NNs_sparse(mp, mp, cf, cf, np.ones((3, 2)), np.zeros((0, 2)))
    assert m.dtype == np.int64 and s.dtype == np.float64 and m.tolist() == [-1, -1, -1] and s.tolist() == [0, 0, 0]
    m, s = NNs_sparse(torch.from_numpy(mp), torch.from_numpy(mp), torch.from_numpy(cf), torch.from_numpy(cf), np.zeros((0, 2)), np.ones((3, 2)))
    assert isinstance(m, np.ndarray) and m.shape == (0,) and s.shape == (0,)
    with pytest.raises(ValueError):
        NNs_sparse(mp, mp, cf[:3], cf, np.ones((3, 2)), np.ones((3, 2)))
    with pytest.raises(capi.MpsfmHipError) as err:
        NNs_sparse(mp[:1], mp, cf[:1], cf, np.ones((3, 2)), np.ones((3, 2)))
    assert err.value.code == EINVAL


def test_nns_sparse_takes_the_keywords_of_the_reference_s_call_site():
    """mast3r.py calls NNs_sparse(A, B, QA, QB, kps0, kps1, subsample_or_initxy1=..., ret_xy=False, scores_thresh=..., dist="dot",
    block_size=2**13) or (..., workers=32); the reference swallows those keywords and ignores them."""
    mp, cf = np.ones((4, 5, 6), np.float32), np.ones((4, 5), np.float32)
    for opt in (dict(dist="dot", block_size=2 ** 13), dict(workers=32)):
        for thr in (0.85, None):
            m, s = NNs_sparse(mp, mp, cf, cf, np.ones((3, 2)), np.zeros((0, 2)), subsample_or_initxy1=8, ret_xy=False, scores_thresh=thr, **opt)
            assert m.tolist() == [-1, -1, -1] and s.tolist() == [0, 0, 0]
    # matcher options are ignored too, as in the reference: the call gets as far as the device either way
    try:
        m, s = NNs_sparse(mp, mp, cf, cf, np.ones((3, 2)), np.ones((2, 2)), subsample_or_initxy1=8, ret_xy=False, do_mutual_check=False,
                          ratio_threshold=0.5, dist="dot", block_size=2 ** 13)
        assert capi.device_count() > 0 and m.shape == (3,)
    except capi.MpsfmHipError as e:
        assert capi.device_count() == 0 and e.code == ENODEVICE


def test_nearest_neighbor_works_behind_a_reference_style_loader():
    """The reference's loader keeps classes DEFINED in the model's module that subclass its BaseModel (a torch Module), builds one
    from the configuration and calls .eval().to(device) on it: a subclass whose _forward delegates passes, and the
    plain class answers eval() and to() itself."""
    import torch

    class BaseModel(torch.nn.Module):  # the protocol of the reference's base class
        default_conf, required_inputs = {}, []

        def __init__(self, conf):
            super().__init__()
            self.conf = {**self.default_conf, **conf}
            self._init(self.conf)

        def forward(self, data):
            for key in self.required_inputs:
                assert key in data
            return self._forward(data)

    class Shim(BaseModel):
        default_conf = dict(NearestNeighbor.default_conf)
        required_inputs = ["descriptors0", "descriptors1"]

        def _init(self, conf):
            self.matcher = NearestNeighbor({k: conf[k] for k in ("ratio_threshold", "distance_threshold", "do_mutual_check")})

        def _forward(self, data):
            return self.matcher(data)

    data = {"descriptors0": torch.ones(1, 8, 3, dtype=torch.float16), "descriptors1": torch.ones(1, 8, 0, dtype=torch.float16)}
    for model in (Shim({"name": "nearest_neighbor", "ratio_threshold": 0.8}).eval().to("cpu"), NearestNeighbor({"ratio_threshold": 0.8}).eval().to("cpu")):
        out = model(data)
        assert out["matches0"].tolist() == [[-1, -1, -1]] and out["matching_scores0"].tolist() == [[0.0, 0.0, 0.0]]
    assert Shim({}).matcher.conf["do_mutual_check"] is True and Shim({"ratio_threshold": 0.8}).matcher.conf["ratio_threshold"] == 0.8
    with pytest.raises(TypeError):  # the dtype itself is compared, not its name
        NearestNeighbor()({"descriptors0": torch.ones(1, 8, 3, dtype=torch.float64), "descriptors1": torch.ones(1, 8, 3, dtype=torch.float64)})


def test_calls_fail_loudly_without_a_device():
    if capi.device_count() > 0:
        return  # with a device the same calls are computed: tests/test_gpu_descriptor_matches.py
    d0, d1 = GOLD["desc0"][:20], GOLD["desc1"][:20]
    g = {k: GOLD[f"maps_{k}"] for k in ("map0", "map1", "conf0", "conf1", "kps0", "kps1")}
    for call in (lambda: match_descriptors(d0, d1), lambda: NearestNeighbor()({"descriptors0": d0.T[None], "descriptors1": d1.T[None]}),
                 lambda: NNs_sparse(g["map0"], g["map1"], g["conf0"], g["conf1"], g["kps0"], g["kps1"])):
        with pytest.raises(capi.MpsfmHipError) as e:
            call()
        assert e.value.code == ENODEVICE
