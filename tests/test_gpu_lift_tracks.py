"""GPU tests of mpsfm_lift_tracks (csrc/lift_tracks.hip) and of MpsfmTriangulator(..., lift="batch") on it, against the NumPy
restatement tests/numpy_lift_tracks.py and against the per-point loop.

Bounds (derived, not measured).  risky: equal to capi.filter_tracks(...)[0] < threshold (the same kernel, the same
comparison).  lift_el, el_keep, counts: exact; the inputs keep every camera-frame depth of a lifted point 1e-9 away from 0
except where it is exactly 0, 2^-53 or 2^-52 by construction (identity rotations, keypoints on pixel centres, translations
that are sums of a few powers of two: no operation rounds on either side).  lift_depth: rtol = atol = 1e-13, the bound
tests/test_gpu_prior.py holds the same sampler to.  lift_xyz: 16 eps (|ray d| + |t|) per component (tests/test_registration_cpu.py)."""

import copy
import ctypes as C

import numpy as np
import pytest

import numpy_lift_tracks as NL
from mpsfm_amd import capi
from mpsfm_amd.abi import CLiftInfo, CLiftMaps, MpsfmHipError
from mpsfm_amd.problem import Tracks
from mpsfm_amd.sfm.mapper.triangulator import MpsfmTriangulator, track_quality
from mpsfm_amd.synthetic import quat_from_R
from test_lift_tracks_cpu import (Recorder, assert_every_branch, check_batch_against_loop, elements_of, first_lifting_element, lift_scene,
                                  midpoint_threshold_deg)
from test_registration_cpu import assert_lift_close

pytestmark = pytest.mark.gpu

EINVAL = -1
W, H = 33, 25
SX, SY = W / 1600.0, H / 1200.0
K = np.array([[1000.0, 1000.0, 800.0, 600.0]])
N_CAMS, OFF_CAM = 8, 7  # camera 7 is not activated
LENGTHS = (0, 1, 2, 3, 63, 64, 65, 128, 129, 200)
FAR, NEAR = np.array([0.3, -0.2, 2000.0]), np.array([0.1, 0.1, 1.0])
THR_DEG = 1.0
VALID, NOT_ACTIVATED, FRACTIONAL, OFF_MAP = 0, 1, 2, 3


def _rot(rng, scale):
    w = rng.normal(0, scale, 3)
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def cameras():
    """Cameras 0-3: identity rotations and translations that are exact in a few bits; 4-7: small rotations."""
    rng = np.random.default_rng(5)
    quat, t = np.zeros((N_CAMS, 4)), np.zeros((N_CAMS, 3))
    quat[:4, 3] = 1.0
    t[1] = (0.5, 0.0, 0.25)
    t[2] = (-0.5, 0.25, -1.0 + 2.0**-52)
    t[3] = (0.25, -0.5, -1.0 + 2.0**-53)
    for c in range(4, N_CAMS):
        quat[c] = quat_from_R(_rot(rng, 0.05)[None])[0]
        t[c] = rng.uniform(-0.6, 0.6, 3)
    return quat, t


def maps():
    """Per camera: a smooth positive depth map with a block of 0 and a block of -2 in the last rows, a validity map with
    the columns 4-7 invalid; pixel (0, 0) of camera 0 has depth exactly 1.  Camera 7: no maps."""
    depth, valid = [], []
    yy, xx = np.mgrid[0:H, 0:W]
    for c in range(N_CAMS):
        d = 3.0 + 0.11 * xx + 0.07 * yy + 0.3 * c
        d[20:, 8:16] = 0.0
        d[20:, 16:24] = -2.0
        v = np.ones((H, W), np.uint8)
        v[:, 4:8] = 0
        depth.append(d)
        valid.append(v)
    depth[0][0, 0] = 1.0
    depth[OFF_CAM], valid[OFF_CAM] = None, None
    return depth, valid


def exact_map_coordinate(m, s, must=True):
    """A keypoint coordinate x with x * s == m exactly in floating point (m a map coordinate with few bits)."""
    x = m / s
    for cand in [x] + [v for k in range(1, 9) for v in (x + k * np.spacing(x), x - k * np.spacing(x))]:
        if cand * s == float(m):
            return cand
    assert not must, f"no keypoint coordinate maps to {m} exactly"
    return None


def _element(rng, kind, exact=False):
    """(camera, keypoint) of one element of the given kind; valid keypoints lie in the columns 9-31 and rows 1-18.  `exact`: a
    valid keypoint whose map coordinates are multiples of 1/8 and 3/4 reached without rounding (x / 32 and y / 24 are exact
    then), so that its four weights, their products and the validity sample of exactly 1 carry no rounding at all; a
    generic keypoint may sample 1 - 2^-53 over four valid pixels, as in the reference."""
    cam = OFF_CAM if kind == NOT_ACTIVATED else int(rng.integers(0, OFF_CAM))
    while exact:
        x = exact_map_coordinate(int(rng.integers(9, 31)) + int(rng.integers(0, 8)) / 8.0, SX, must=False)
        y = exact_map_coordinate(0.75 * int(rng.integers(2, 25)), SY, must=False)
        if x is not None and y is not None:
            return cam, (x, y)
    if kind == FRACTIONAL:    # between an invalid and a valid pixel
        mx, my = 7.0 + rng.uniform(0.2, 0.8), rng.uniform(1.1, 17.9)
    elif kind == OFF_MAP:
        mx, my = (rng.uniform(-400, -40), rng.uniform(1.1, 17.9)) if rng.integers(2) else (rng.uniform(9.1, 30.9), rng.uniform(60, 500))
    else:
        mx, my = rng.uniform(9.1, 30.9), rng.uniform(1.1, 17.9)
    return cam, (mx / SX, my / SY)


def build_tracks():
    """The tracks of the shape test: (Tracks, xyz, per track the expected position of the first valid element or -1,
    whether it is meant to be risky, a set of tags)."""
    rng = np.random.default_rng(17)
    specs = []  # (elements [(cam, (x, y))], xyz, expected first, risky, tag)
    for L in LENGTHS:
        for P in sorted({p for p in (0, 1, 62, 63, 64, 127, 128, L - 1) if 0 <= p < L}) + [None]:
            for way in range(3):  # which of the three invalid kinds the element before the first valid one gets
                els = []
                for i in range(L):
                    if P is None or i < P:
                        kind = (NOT_ACTIVATED, FRACTIONAL, OFF_MAP)[(way + (P if P is not None else L) - 1 - i) % 3]
                    elif i == P:
                        kind = VALID
                    else:
                        kind = int(rng.integers(0, 4))
                    els.append(_element(rng, kind, exact=i == P))
                specs.append((els, FAR + rng.normal(0, 0.05, 3), -1 if P is None else P, True, "shape"))
    # keypoints exactly on the last column / the last row
    xl, yl = exact_map_coordinate(W - 1, SX), exact_map_coordinate(H - 1, SY)
    specs.append(([(4, (xl, exact_map_coordinate(5.25, SY))), (5, (12.2 / SX, 3.3 / SY))], FAR.copy(), 0, True, "last_col"))
    specs.append(([(OFF_CAM, (12.2 / SX, 3.3 / SY)), (6, (exact_map_coordinate(19.5, SX), yl)), (5, (12.2 / SX, 3.3 / SY))], FAR.copy(), 1, True, "last_row_neg"))
    y3 = exact_map_coordinate(3.0, SY)
    specs.append(([(5, (xl + 1e-9, y3)), (6, (xl, y3))], FAR.copy(), 1, True, "last_col"))  # just past the column: a tap off the map
    # sampled depth exactly 0 (identity cameras, keypoint on a pixel centre) and below 0
    x0, y0 = exact_map_coordinate(10, SX), exact_map_coordinate(22, SY)
    specs.append(([(1, (x0, y0)), (0, (700.0, 500.0)), (2, (900.0, 640.0)), (3, (100.0, 90.0))], FAR.copy(), 0, True, "depth0"))
    specs.append(([(OFF_CAM, (700.0, 500.0)), (5, (19.4 / SX, 22.3 / SY)), (1, (700.0, 500.0)), (4, (10.0, 10.0))], FAR.copy(), 1, True, "depth_neg"))
    # camera-frame depth exactly 2^-52 (kept) and 2^-53 (dropped): camera 0 lifts d = 1 at pixel (0, 0), t = 0
    specs.append(([(0, (0.0, 0.0)), (2, (5.0, 5.0)), (3, (5.0, 5.0)), (1, (5.0, 5.0))], FAR.copy(), 0, True, "eps"))
    # not risky: a near point seen by cameras 0, 1, 2 first
    for L in (2, 3, 5, 64, 70):
        els = [(c, (rng.uniform(9.1, 30.9) / SX, rng.uniform(1.1, 17.9) / SY)) for c in (0, 1, 2)][:max(2, min(L, 3))]
        els += [_element(rng, VALID) for _ in range(L - len(els))]
        for _ in range(4):
            specs.append((els, NEAR + rng.normal(0, 0.01, 3), -1, False, "not_risky"))
    order = rng.permutation(len(specs))
    specs = [specs[i] for i in order]
    quat, t = cameras()
    start = np.concatenate([[0], np.cumsum([len(s[0]) for s in specs])])
    el_cam = np.array([c for s in specs for c, _ in s[0]], np.int32)
    el_xy = np.array([xy for s in specs for _, xy in s[0]], np.float64).reshape(-1, 2)
    tr = Tracks(cam_quat=quat, cam_t=t, cam_intr=K, cam_intr_idx=np.zeros(N_CAMS, np.int32), track_start=start, el_cam=el_cam, el_xy=el_xy)
    return tr, np.array([s[1] for s in specs]), np.array([s[2] for s in specs]), np.array([s[3] for s in specs]), [s[4] for s in specs]


def map_arguments():
    depth, valid = maps()
    activated = np.array([m is not None for m in depth])
    return activated, depth, valid, np.full(N_CAMS, SX), np.full(N_CAMS, SY)


def check_expectations(tr, want, first, risky, tags):
    """The construction against the restatement (no GPU): every planned case is what the restatement finds, and the depths
    keep their distance from 0."""
    np.testing.assert_array_equal(want["risky"], risky)
    np.testing.assert_array_equal(want["lift_el"], np.where(risky, first, -1))
    start = tr.track_start
    exact = np.zeros(tr.n_el, bool)
    for t, tag in enumerate(tags):
        z, keep = want["z"][start[t]:start[t + 1]], want["el_keep"][start[t]:start[t + 1]]
        if tag == "eps":    # cameras 0, 2, 3, 1: depths 1, 2^-52, 2^-53, 1.25
            assert list(z) == [1.0, 2.0**-52, 2.0**-53, 1.25] and list(keep) == [True, True, False, True]
            exact[start[t]:start[t + 1]] = True
        elif tag == "depth0":    # the point is the centre of camera 1: depths 0, -0.25, -1.25 + 2^-52, -1.25 + 2^-53
            assert want["lift_depth"][t] == 0.0 and z[0] == 0.0 and not keep.any() and np.all(z[1:] < -0.2)
            exact[start[t]] = True
        elif tag == "depth_neg":
            assert want["lift_depth"][t] < -1.9 and not keep[1]
        elif tag == "last_row_neg":
            assert want["lift_depth"][t] == -2.0
    lifted_el = np.repeat(want["lift_el"] >= 0, np.diff(start))
    assert np.all(np.abs(want["z"][lifted_el & ~exact]) > 1e-9)
    assert (want["el_keep"][lifted_el]).sum() > 1000 and (~want["el_keep"][lifted_el]).sum() > 10


@pytest.fixture(scope="module")
def shape_case():
    tr, xyz, first, risky, tags = build_tracks()
    args = map_arguments()
    ang = capi.filter_tracks(tr, xyz)[0]
    assert np.all(np.abs(ang - np.deg2rad(THR_DEG)) > 1e-3)
    want = NL.lift_tracks(tr, xyz, *args, THR_DEG, angles=ang)
    check_expectations(tr, want, first, risky, tags)
    got = capi.lift_tracks(tr, xyz, *args, THR_DEG)
    return dict(tr=tr, xyz=xyz, args=args, ang=ang, want=want, got=got)


def assert_outputs(got, want):
    np.testing.assert_array_equal(got["risky"], want["risky"])
    np.testing.assert_array_equal(got["lift_el"], want["lift_el"])
    np.testing.assert_array_equal(got["el_keep"], want["el_keep"])
    np.testing.assert_allclose(got["lift_depth"], want["lift_depth"], rtol=1e-13, atol=1e-13)
    assert_lift_close(got["lift_xyz"], want["lift_xyz"], want["scale"])
    for k in ("n_risky", "n_lifted", "n_no_lift", "n_maps_uploaded", "bytes_uploaded"):
        assert got["info"][k] == want["info"][k], k


def test_every_track_shape_matches_the_restatement(shape_case):
    s = shape_case
    np.testing.assert_array_equal(s["got"]["risky"], s["ang"] < np.deg2rad(THR_DEG))  # bit for bit the angle of mpsfm_filter_tracks
    assert_outputs(s["got"], s["want"])
    assert s["got"]["info"]["n_no_lift"] >= 3 * len(LENGTHS) and s["got"]["info"]["ms"] > 0
    assert s["got"]["risky"].dtype == bool and s["got"]["lift_el"].dtype == np.int32 and s["got"]["el_keep"].dtype == bool
    # a second call gives the same answer bit for bit (no state between calls, no atomics)
    again = capi.lift_tracks(s["tr"], s["xyz"], *s["args"], THR_DEG)
    for k in ("risky", "lift_el", "lift_depth", "lift_xyz", "el_keep"):
        np.testing.assert_array_equal(again[k], s["got"][k])


def test_only_the_maps_of_risky_tracks_go_up(shape_case):
    s = shape_case
    none = capi.lift_tracks(s["tr"], s["xyz"], *s["args"], 0.0)  # angle < 0 never holds
    assert none["info"]["n_risky"] == 0 and none["info"]["n_maps_uploaded"] == 0 and none["info"]["bytes_uploaded"] == 0
    assert not none["risky"].any() and np.all(none["lift_el"] == -1) and not none["el_keep"].any()
    assert not none["lift_depth"].any() and not none["lift_xyz"].any()
    # tracks of the cameras {0, 1, 7} far away (risky; 7 is not activated and has no maps), of {2, 3, 4} close by (not risky)
    quat, t = cameras()
    kp = (15.5 / SX, 9.5 / SY)
    cams = [[0, 1], [2, 3, 4], [OFF_CAM, 1, 0], [4, 3], [OFF_CAM]]
    pts = np.array([FAR, NEAR, FAR, NEAR, FAR])
    tr = Tracks(cam_quat=quat, cam_t=t, cam_intr=K, cam_intr_idx=np.zeros(N_CAMS, np.int32), track_start=np.cumsum([0] + [len(c) for c in cams]),
                el_cam=np.concatenate(cams).astype(np.int32), el_xy=np.tile(kp, (sum(len(c) for c in cams), 1)))
    ang = capi.filter_tracks(tr, pts)[0]
    got = capi.lift_tracks(tr, pts, *s["args"], THR_DEG)
    np.testing.assert_array_equal(got["risky"], [True, False, True, False, True])
    np.testing.assert_array_equal(got["lift_el"], [0, -1, 1, -1, -1])
    assert got["info"]["n_maps_uploaded"] == 2 and got["info"]["bytes_uploaded"] == 2 * W * H * 9
    assert (got["info"]["n_risky"], got["info"]["n_lifted"], got["info"]["n_no_lift"]) == (3, 2, 1)
    assert_outputs(got, NL.lift_tracks(tr, pts, *s["args"], THR_DEG, angles=ang))


def test_drop_in_batch_equals_the_loop_on_the_library():
    sc = lift_scene()
    ids = np.array(sorted(sc.points3D))
    ang, _, _ = track_quality(sc, ids)
    thr = midpoint_threshold_deg(ang)
    risky_ids = [int(p) for p in ids[ang < np.deg2rad(thr)]]
    before = {p: elements_of(sc, p) for p in risky_ids}
    first = {p: first_lifting_element(sc, p) for p in risky_ids}
    a, b = copy.deepcopy(sc), copy.deepcopy(sc)
    # the library's answer, with the error scale of the restatement next to it
    backend = Recorder(lambda *args, **kw: dict(capi.lift_tracks(*args, **kw), scale=NL.lift_tracks(*args, angles=ang, **kw)["scale"]))
    new_a = MpsfmTriangulator({"colmap_options": {}}, a, None, lift="batch", lift_backend=backend).lift_low_parallax(ids, thr)
    new_b = MpsfmTriangulator({"colmap_options": {}}, b, None, lift="loop").lift_low_parallax(ids, thr)
    out = backend.calls[0]
    got, want, lifted = check_batch_against_loop(a, b, ids, new_a, new_b, out, before, first)
    assert_lift_close(got, want, out["scale"][lifted])
    assert_every_branch(out["lift_el"][out["risky"]], before, [elements_of(a, p) for p in new_a])
    # without a backend the object goes to the library itself
    c = copy.deepcopy(sc)
    tri = MpsfmTriangulator({"colmap_options": {}}, c, None, lift="batch")
    assert tri.lift_low_parallax(ids, thr) == new_a and tri.last_lift_info["n_lifted"] == len(new_a)
    assert tri.last_lift_info["n_maps_uploaded"] == 5  # six images, one of them not activated


def _raw(tr, xyz, M, thr_rad, outs=None):
    nt, ne = tr.n_tracks, tr.n_el
    o = outs or [np.zeros(nt, np.uint8), np.zeros(nt, np.int32), np.zeros(nt), np.zeros((nt, 3)), np.zeros(ne, np.uint8)]
    ct, I = tr.c_tracks(), CLiftInfo()
    xyz = np.ascontiguousarray(xyz, np.float64)
    rc = capi.lib().mpsfm_lift_tracks(C.byref(ct), xyz.ctypes.data, C.byref(M) if M is not None else None, thr_rad, 0,
                                      *[a.ctypes.data if a is not None else None for a in o], C.byref(I))
    return rc, (capi.lib().mpsfm_last_error() or b"").decode()


def test_refused_inputs_leave_the_library_usable(shape_case):
    s = shape_case
    tr, xyz, args = s["tr"], s["xyz"], s["args"]
    activated, depth, valid, sx, sy = args

    def refused(call, *a, **kw):
        with pytest.raises(MpsfmHipError) as e:
            call(*a, **kw)
        assert e.value.code == EINVAL and len(str(e.value)) > 30
        again = capi.lift_tracks(tr, xyz, *args, THR_DEG)  # the next call works
        np.testing.assert_array_equal(again["lift_el"], s["got"]["lift_el"])

    refused(capi.lift_tracks, tr, xyz, *args, float("nan"))
    refused(capi.lift_tracks, tr, xyz, *args, -1.0)
    bad = copy.deepcopy(tr)
    bad.el_cam[3] = N_CAMS  # check_tracks
    refused(capi.lift_tracks, bad, xyz, *args, THR_DEG)
    bad = copy.deepcopy(tr)
    bad.track_start[1] = bad.track_start[2] + 1
    refused(capi.lift_tracks, bad, xyz, *args, THR_DEG)
    # an activated camera of a risky track without a map, with a map of one row, of one column
    for broken in (None, np.ones((1, W)), np.ones((H, 1))):
        d, v = list(depth), list(valid)
        d[2], v[2] = broken, (None if broken is None else np.ones(broken.shape, np.uint8))
        refused(capi.lift_tracks, tr, xyz, activated, d, v, sx, sy, THR_DEG)
    d, v = list(depth), list(valid)
    v[3] = None
    refused(capi.lift_tracks, tr, xyz, activated, d, v, sx, sy, THR_DEG)
    # ... but not where no track is risky, and not for a camera that is not activated
    d[2] = None
    assert capi.lift_tracks(tr, xyz, activated, d, v, sx, sy, 0.0)["info"]["n_risky"] == 0
    # NULL arrays and more than 2^30 pixels: only the raw call can say that
    hh, ww = np.full(N_CAMS, H, np.int32), np.full(N_CAMS, W, np.int32)
    act = activated.astype(np.uint8)
    dm = [np.ascontiguousarray(m if m is not None else np.zeros((H, W))) for m in depth]
    vm = [np.ascontiguousarray(m if m is not None else np.zeros((H, W), np.uint8)) for m in valid]
    dptr, vptr = (C.c_void_p * N_CAMS)(*[m.ctypes.data for m in dm]), (C.c_void_p * N_CAMS)(*[m.ctypes.data for m in vm])
    fields = dict(activated=act.ctypes.data, map_h=hh.ctypes.data, map_w=ww.ctypes.data, depth_map=C.addressof(dptr),
                  valid_map=C.addressof(vptr), sx=sx.ctypes.data, sy=sy.ctypes.data)
    thr = float(np.deg2rad(THR_DEG))
    assert _raw(tr, xyz, CLiftMaps(**fields), thr)[0] == 0
    for name in fields:
        rc, msg = _raw(tr, xyz, CLiftMaps(**dict(fields, **{name: None})), thr)
        assert rc == EINVAL and "NULL" in msg, name
    assert _raw(tr, xyz, None, thr)[0] == EINVAL
    for k in range(5):
        outs = [np.zeros(tr.n_tracks, np.uint8), np.zeros(tr.n_tracks, np.int32), np.zeros(tr.n_tracks), np.zeros((tr.n_tracks, 3)), np.zeros(tr.n_el, np.uint8)]
        outs[k] = None
        assert _raw(tr, xyz, CLiftMaps(**fields), thr, outs)[0] == EINVAL
    hh[1], ww[1] = 40000, 40000  # 1.6e9 pixels: refused before anything is read
    rc, msg = _raw(tr, xyz, CLiftMaps(**fields), thr)
    assert rc == EINVAL and "2^30" in msg
    again = capi.lift_tracks(tr, xyz, *args, THR_DEG)
    np.testing.assert_array_equal(again["el_keep"], s["got"]["el_keep"])


def test_no_tracks_give_empty_arrays():
    quat, t = cameras()
    tr = Tracks(cam_quat=quat, cam_t=t, cam_intr=K, cam_intr_idx=np.zeros(N_CAMS, np.int32), track_start=np.zeros(1, np.int64),
                el_cam=np.zeros(0, np.int32), el_xy=np.zeros((0, 2)))
    got = capi.lift_tracks(tr, np.zeros((0, 3)), *map_arguments(), THR_DEG)
    assert [len(got[k]) for k in ("risky", "lift_el", "lift_depth", "lift_xyz", "el_keep")] == [0] * 5
    assert got["lift_xyz"].shape == (0, 3) and got["info"]["n_risky"] == 0 and got["info"]["n_maps_uploaded"] == 0
