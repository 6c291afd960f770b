"""Warp to match lists without a GPU: the NumPy restatement (tests/numpy_warp_matches.py) against the fixture computed by the
reference's own warp.py (tests/golden/make_golden_warp_matches.py), bitwise and on every row; the restatement's tie, empty and
r = 0 branches; the entry points' argument checks and empty calls, which come before any device is touched; the wrappers' return
types and lengths."""

import ctypes as C
import os

import numpy as np
import pytest

import numpy_warp_matches as NW
from mpsfm_amd import capi
from mpsfm_amd.extraction.pairwise import warp as WM

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_warp_matches.npz"))
EINVAL, ENODEVICE = -1, -2
NMS_MAPS, RADII = ("random", "quantised", "saturated", "negative"), (0, 1, 4, 8)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", NMS_MAPS)
def test_restatement_equals_the_reference_simple_nms_bitwise(name):
    for r in RADII:
        assert np.array_equal(bits(NW.simple_nms(GOLD[f"nms_{name}"], r)), bits(GOLD[f"nms_{name}_r{r}"]))
    assert np.array_equal(bits(GOLD[f"nms_{name}_r0"]), bits(GOLD[f"nms_{name}"]))  # r = 0 keeps everything


def test_restatement_equals_the_reference_unique_matches():
    m, s, keep = NW.kpids_to_matches0(GOLD["uniq_ids0"], GOLD["uniq_ids1"], GOLD["uniq_scores"])
    assert np.array_equal(m, GOLD["uniq_matches0"]) and np.array_equal(s.astype(np.float16), GOLD["uniq_scores0"])
    assert len(np.unique(GOLD["uniq_scores"])) == len(GOLD["uniq_scores"]) and len(keep) >= 10


def roma_inputs():
    g = {k[5:]: GOLD[k] for k in GOLD.files if k.startswith("roma_")}
    kw = dict(skpts0=g["skpts0"], skpts1=g["skpts1"], scale0=g["scale0"], scale1=g["scale1"], nms_radius=int(g["nms_radius"]),
              sample_thresh=float(g["sample_thresh"]), max_error=float(g["max_error"]))
    return g, kw


def test_restatement_equals_the_reference_on_both_legs():
    g, kw = roma_inputs()
    out = NW.warp_to_matches(g["warp"], g["certainty"], tuple(g["sizes"]), True, True, **kw)
    assert np.array_equal(out["ids0"], g["ids0"]) and np.array_equal(out["ids1"], g["ids1"])
    assert np.array_equal(out["smatches0"], g["smatches0"])
    assert np.array_equal(out["smatching_scores0"].astype(np.float16), g["smatching_scores0"])
    for k in ("dkeypoints0", "dkeypoints1", "dscores"):
        assert np.array_equal(bits(out[k]), bits(g[k])), k
    valid = (g["ids0"] >= 0) & (g["ids1"] >= 0)
    assert (g["smatches0"] >= 0).sum() >= 100 and valid.sum() - (g["smatches0"] >= 0).sum() >= 10
    assert len(g["smatches0"]) < len(g["skpts0"])  # the reference's length rule, not the number of keypoints


def test_restatement_ties_go_to_the_lowest_row_and_zero_signs_tie():
    ids0 = np.array([0, 0, 1, 1, 2, 2, -1])
    ids1 = np.array([0, 1, 2, 2, 3, 4, 5])
    sc = np.array([0.5, 0.5, 0.25, 0.25, -0.0, 0.0, 9.0], np.float32)
    m, s, keep = NW.kpids_to_matches0(ids0, ids1, sc)
    assert keep.tolist() == [0, 2, 4] and m.tolist() == [0, 2, 3]
    assert np.signbit(s[2]) and s[2] == 0  # the kept row's own score, sign included
    # wins its ids0 group, loses its ids1 group
    m, s, keep = NW.kpids_to_matches0([0, 1, 1], [0, 0, 1], np.array([0.9, 0.8, 0.7], np.float32))
    assert keep.tolist() == [0] and m.tolist() == [0]


def test_restatement_empty_and_radius_zero_branches():
    m, s, keep = NW.kpids_to_matches0([-1, 2], [3, -1], np.array([1, 2], np.float32))
    assert m.shape == (0,) and m.dtype == np.int32 and s.shape == (0,) and len(keep) == 0
    m, s, _ = NW.kpids_to_matches0([], [], np.zeros(0, np.float32))
    assert m.shape == (0,)
    x = np.array([[0.0, -1.0, 2.0]], np.float32)
    assert np.array_equal(bits(NW.simple_nms(x, 0)), bits(x))
    assert NW.simple_nms(x, 1).tolist() == [[0.0, 0.0, 2.0]]  # every pixel has a maximum in its window: nothing is recovered, and 0.0 stays as its own value
    assert NW.simple_nms(np.full((3, 4), 0.5, np.float32), 2).tolist() == [[0.5] * 4] * 3  # a plateau keeps every pixel
    neg = np.array([[-1.0, -3.0, -2.0]], np.float32)
    # the window of -2 at the border holds only -3 and -2: a second maximum
    assert NW.simple_nms(neg, 1).tolist() == [[-1.0, 0.0, -2.0]]
    pa, pb = NW.to_pixel_coordinates(np.array([[-1, 1, 0, 0.5]], np.float32), 10, 21, 7, 8)
    assert pa.dtype == np.float32 and pa.tolist() == [[0.0, 10.0]] and pb.tolist() == [[4.0, 5.25]]


# ---- the C ABI without a device -------------------------------------------------------------------------------------------
def _lib():
    L = capi.lib()
    return L


P = lambda a: None if a is None else a.ctypes.data  # noqa: E731
ANSWER = lambda: 0 if capi.device_count() > 0 else ENODEVICE  # noqa: E731


def test_default_options_are_the_reference_s():
    o = capi.CWarpOptions(9.0, 9.0, (C.c_double * 2)(3, 3), (C.c_double * 2)(3, 3), 1, 1, 5)
    _lib().mpsfm_warp_default_options(C.addressof(o))
    assert (o.sample_thresh, o.max_error, list(o.scale0), list(o.scale1), o.nms_radius, o.inputs_on_device, o.stream) == (
        0.1, 2.0, [1.0, 1.0], [1.0, 1.0], 8, 0, None)
    assert WM.warp_to_matches.__defaults__ == ("sparse", None, None, (1, 1), (1, 1), 8, 0.1, 2)


def test_simple_nms_checks_arguments_before_any_device():
    L = _lib()
    s, out = np.ones((3, 4), np.float32), np.zeros((3, 4), np.float32)

    def call(H=3, W=4, a=s, r=1, b=out):
        return L.mpsfm_simple_nms(H, W, P(a), r, 0, None, 0, P(b), None)

    assert call(H=0) == EINVAL and call(W=0) == EINVAL and call(H=-2) == EINVAL
    assert call(H=1 << 14, W=(1 << 13) + 1) == EINVAL  # above 2^27 pixels
    assert call(r=-1) == EINVAL and call(r=65) == EINVAL
    assert call(a=None) == EINVAL and call(b=None) == EINVAL
    for bad in (np.nan, np.inf, -np.inf):
        x = s.copy(); x[2, 3] = bad
        assert call(a=x) == EINVAL and b"non-finite" in L.mpsfm_last_error()
    assert call() == ANSWER() and call(r=0) == ANSWER() and call(r=64) == ANSWER()
    # device ranges that overlap are refused from the addresses alone; disjoint ones get as far as the device
    big = np.zeros(40, np.float32)
    for off in (0, 1, 11, -11):
        assert L.mpsfm_simple_nms(3, 4, big.ctypes.data + 4 * 12, 1, 1, None, 0, big.ctypes.data + 4 * (12 + off), None) == EINVAL
        assert b"overlap" in L.mpsfm_last_error()
    assert L.mpsfm_simple_nms(3, 4, big.ctypes.data, 1, 1, None, 0, big.ctypes.data + 4 * 12, None) in (EINVAL, ENODEVICE)
    assert b"overlap" not in L.mpsfm_last_error()  # host memory passed as device memory: refused by the pointer check, with a device


def test_kpids_to_matches0_checks_arguments_before_any_device():
    L = _lib()
    i0, i1, sc = np.array([0, 1, -1], np.int64), np.array([1, -1, 0], np.int64), np.array([0.5, 0.25, 1.0], np.float32)
    m, s, nk = np.zeros(2, np.int32), np.zeros(2, np.float32), C.c_int64(7)

    def call(n=3, a=i0, b=i1, c=sc, n0=2, n1=2, mm=m, ss=s, k=nk):
        return L.mpsfm_kpids_to_matches0(n, P(a), P(b), P(c), n0, n1, 0, None, 0, P(mm), P(ss), None if k is None else C.addressof(k), None)

    assert call(n=-1) == EINVAL and call(n0=-1) == EINVAL and call(n1=-1) == EINVAL
    assert call(n=(1 << 27) + 1) == EINVAL and call(n0=(1 << 27) + 1) == EINVAL
    for ptr in ("a", "b", "c", "mm", "ss", "k"):
        assert call(**{ptr: None}) == EINVAL
    assert call(a=np.array([0, 2, -1], np.int64)) == EINVAL and call(b=np.array([2, -1, 0], np.int64)) == EINVAL  # ids >= n0 / n1
    assert call(a=np.array([0, -2, -1], np.int64)) == EINVAL and call(b=np.array([1, -1, -5], np.int64)) == EINVAL
    for bad in (np.nan, np.inf):
        x = sc.copy(); x[1] = bad
        assert call(c=x) == EINVAL
    # empty calls: all -1 / 0 / count 0 without a device
    m[:], s[:], nk.value = 7, 7.0, 7
    assert call(n=0, a=None, b=None, c=None) == 0 and m.tolist() == [-1, -1] and s.tolist() == [0, 0] and nk.value == 0
    m[:], nk.value = 7, 7
    assert call(n1=0, b=np.array([-1, -1, -1], np.int64)) == 0 and m.tolist() == [-1, -1] and nk.value == 0
    assert call(n0=0, a=np.array([-1, -1, -1], np.int64), mm=None, ss=None) == 0
    info = capi.CWarpInfo(5, 5, 5, 5.0, 0)
    assert L.mpsfm_kpids_to_matches0(0, None, None, None, 2, 2, 0, None, 0, P(m), P(s), C.addressof(nk), C.addressof(info)) == 0
    assert (info.num_dense, info.num_valid, info.num_matches, info.ms) == (0, 0, 0, 0)
    assert call() == ANSWER()


def test_warp_matches_checks_arguments_before_any_device():
    L = _lib()
    H, W = 3, 4
    cert, warp = np.full((H, W), 0.5, np.float32), np.zeros((H * W, 4), np.float32)
    k0, k1 = np.ones((2, 2)), np.ones((3, 2))
    d0, d1, ds = np.zeros((H * W, 2), np.float32), np.zeros((H * W, 2), np.float32), np.zeros(H * W, np.float32)
    m, s = np.zeros(2, np.int32), np.zeros(2, np.float32)
    nd, nk = C.c_int64(7), C.c_int64(7)

    def call(H=H, W=W, c=cert, w=warp, sizes=(30, 40, 30, 40), mode=3, opts=None, n0=2, kk0=k0, n1=3, kk1=k1, o0=d0, o1=d1, os_=ds, cnt=nd,
             mm=m, ss=s, k=nk):
        return L.mpsfm_warp_matches(H, W, P(c), P(w), *sizes, mode, None if opts is None else C.addressof(opts), n0, P(kk0), n1, P(kk1), 0,
                                    P(o0), P(o1), P(os_), None if cnt is None else C.addressof(cnt), P(mm), P(ss),
                                    None if k is None else C.addressof(k), None)

    assert call(H=0) == EINVAL and call(W=0) == EINVAL and call(H=1 << 14, W=(1 << 13) + 1) == EINVAL
    assert call(mode=0) == EINVAL and call(mode=4) == EINVAL and call(mode=7) == EINVAL
    for sizes in ((0, 40, 30, 40), (30, 0, 30, 40), (30, 40, -1, 40), (30, 40, 30, 0)):
        assert call(sizes=sizes) == EINVAL
    for ptr in ("c", "w", "kk0", "kk1", "o0", "o1", "os_", "cnt", "mm", "ss", "k"):
        assert call(**{ptr: None}) == EINVAL, ptr
    assert call(mode=1, kk0=None, kk1=None, mm=None, ss=None, k=None) == ANSWER()  # the dense leg does not need the sparse leg's arguments
    assert call(n0=-1) == EINVAL and call(n1=-1) == EINVAL and call(n0=(1 << 27) + 1) == EINVAL
    for field, bad in (("nms_radius", -1), ("nms_radius", 65), ("sample_thresh", np.nan), ("sample_thresh", np.inf), ("sample_thresh", 1e300), ("sample_thresh", -3.5e38), ("max_error", np.nan),
                       ("max_error", -1.0), ("max_error", np.inf), ("scale0", (np.nan, 1.0)), ("scale1", (1.0, np.inf))):
        o = capi._warp_options()
        setattr(o, field, (C.c_double * 2)(*bad) if isinstance(bad, tuple) else bad)
        assert call(opts=o) == EINVAL, field
    for bad in (np.nan, np.inf):
        x = cert.copy(); x[2, 3] = bad
        assert call(c=x) == EINVAL
        y = warp.copy(); y[11, 3] = bad
        assert call(w=y) == EINVAL
        z = k1.copy(); z[2, 1] = bad
        assert call(kk1=z) == EINVAL and call(kk0=z[1:]) == EINVAL
    assert call(kk0=np.array([[1e308, 0.0], [-1e308, 0.0]])) == EINVAL  # a bounding box wider than DBL_MAX
    # the sparse leg alone with an empty side: all -1 / 0 / count 0 without a device
    m[:], s[:], nk.value = 7, 7.0, 7
    assert call(mode=2, n1=0, kk1=None) == 0 and m.tolist() == [-1, -1] and s.tolist() == [0, 0] and nk.value == 0
    assert call(mode=2, n0=0, kk0=None, mm=None, ss=None) == 0
    assert call() == ANSWER() and call(mode=2) == ANSWER()


# ---- the wrappers ---------------------------------------------------------------------------------------------------------
def test_wrappers_return_types_and_lengths_without_a_device():
    import torch

    m, s = WM.kpids_to_matches0(np.array([-1, 3]), np.array([2, -1]), np.array([0.5, 0.25], np.float32))
    assert m.dtype == np.int32 and s.dtype == np.float16 and m.shape == (0,) and s.shape == (0,)
    m, s = WM.kpids_to_matches0(np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32))
    assert m.dtype == np.int32 and s.dtype == np.float16 and m.shape == (0,)
    m, s = WM.kpids_to_matches0(torch.tensor([-1, -1]), torch.tensor([0, 1]), torch.tensor([0.5, 0.25]))
    assert isinstance(m, np.ndarray) and m.shape == (0,)
    with pytest.raises(TypeError):
        WM.kpids_to_matches0(np.array([0]), np.array([0]), np.array([0.1]))  # a float64 score float32 does not hold
    with pytest.raises(TypeError):
        WM.kpids_to_matches0(np.array([0]), np.array([0]), np.array([1]))
    with pytest.raises(ValueError):
        WM.kpids_to_matches0(np.array([0, 1]), np.array([0]), np.array([0.5], np.float32))
    with pytest.raises(TypeError):
        WM.kpids_to_matches0(np.array([0.5]), np.array([0]), np.array([0.5], np.float32))  # a float id is not truncated
    with pytest.raises(capi.MpsfmHipError) as e:
        WM.kpids_to_matches0(np.array([0, -3]), np.array([0, 0]), np.array([0.5, 0.5], np.float32))
    assert e.value.code == EINVAL
    warp, cert = np.zeros((3, 4, 4), np.float32), np.full((3, 4), 0.5, np.float32)
    pred = WM.warp_to_matches(warp, cert, (30, 40, 30, 40), "sparse", np.zeros((0, 2)), np.ones((5, 2)))
    assert set(pred) == {"smatches0", "smatching_scores0"}
    assert pred["smatches0"].dtype == np.int32 and pred["smatching_scores0"].dtype == np.float16 and pred["smatches0"].shape == (0,)
    pred = WM.warp_to_matches(torch.from_numpy(warp), torch.from_numpy(cert), (30, 40, 30, 40), "sparse", np.ones((5, 2)), np.zeros((0, 2)))
    assert pred["smatches0"].shape == (0,) and pred["smatching_scores0"].shape == (0,)
    assert WM.warp_to_matches(warp, cert, (30, 40, 30, 40), "none") == {}
    with pytest.raises(ValueError):
        WM.warp_to_matches(warp, cert, (30, 40, 30, 40), "sparse")
    with pytest.raises(ValueError):
        WM.warp_to_matches(warp[:2], cert, (30, 40, 30, 40), "dense")
    with pytest.raises(TypeError):
        WM.warp_to_matches(warp.astype(np.float64), cert, (30, 40, 30, 40), "dense")
    with pytest.raises(TypeError):
        WM.simple_nms(np.ones((3, 3)), 1)
    with pytest.raises(AssertionError):
        WM.simple_nms(np.ones(3, np.float32), 1)
    with pytest.raises(AssertionError):
        WM.simple_nms(np.ones((3, 3), np.float32), -1)
    e0 = WM.simple_nms(np.zeros((0, 5), np.float32), 2)
    assert isinstance(e0, np.ndarray) and e0.shape == (0, 5) and e0.dtype == np.float32
    # to_pixel_coordinates: torch and NumPy inputs, bitwise the restatement
    w = GOLD["roma_warp"]
    sizes = tuple(int(v) for v in GOLD["roma_sizes"])
    ra, rb = NW.to_pixel_coordinates(w, *sizes)
    na, nb = WM.to_pixel_coordinates(w, *sizes)
    ta, tb = WM.to_pixel_coordinates(torch.from_numpy(w), *sizes)
    assert na.shape == w.shape[:2] + (2,) and isinstance(ta, torch.Tensor) and ta.dtype == torch.float32
    assert np.array_equal(bits(na.reshape(-1, 2)), bits(ra)) and np.array_equal(bits(ta.numpy().reshape(-1, 2)), bits(ra))
    assert np.array_equal(bits(nb.reshape(-1, 2)), bits(rb)) and np.array_equal(bits(tb.numpy().reshape(-1, 2)), bits(rb))
    from mpsfm_amd.extraction.pairwise import utils
    assert WM.assign_keypoints is utils.assign_keypoints


def test_calls_fail_loudly_without_a_device():
    if capi.device_count() > 0:
        return  # with a device the same calls are computed: tests/test_gpu_warp_matches.py
    g, kw = roma_inputs()
    for call in (lambda: WM.simple_nms(GOLD["nms_random"], 4), lambda: WM.kpids_to_matches0(GOLD["uniq_ids0"], GOLD["uniq_ids1"], GOLD["uniq_scores"]),
                 lambda: WM.warp_to_matches(g["warp"], g["certainty"], tuple(g["sizes"]), "sparse+dense", **kw)):
        with pytest.raises(capi.MpsfmHipError) as e:
            call()
        assert e.value.code == ENODEVICE
