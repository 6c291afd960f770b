"""GPU checks of the batched two-view geometry (csrc/two_view_batch.hip through capi.two_view_geometry_batch and the
drop-ins).  The yardstick is capi.two_view_geometry on the same device: every pair of a batch must be IDENTICAL to its own
single call, `ms` apart: config, success, watermark, the counts, every field of all four legs (lo_rounds and num_batches
included), the mask by array_equal, E, F, H and the pose by their bytes, tri_angle by ==.  No tolerance: both sides run the same
arithmetic in the same order.  Single-pair HIP against the NumPy restatement is
tests/test_gpu_two_view_geometry.py's subject; the restatement only supplies inputs here."""

import threading

import numpy as np
import pytest

import numpy_two_view_geometry as TV
from mpsfm_amd import capi
from mpsfm_amd.sfm.scene.correspondences import geometric_verification

pytestmark = pytest.mark.gpu

SCALARS = ("config", "success", "watermark", "num_inliers", "num_cheirality_points", "num_border_inliers")


def _args(s):
    return s["points1"], s["points2"], s["intr1"], s["intr2"], s["size1"], s["size2"]


def _identical(a, b, legs_but=()):
    for k in SCALARS:
        assert a[k] == b[k], (k, a[k], b[k])
    assert set(a["legs"]) == set(b["legs"]) == set("EFHT")
    for k in "EFHT":
        la = {f: v for f, v in a["legs"][k].items() if f not in legs_but}
        lb = {f: v for f, v in b["legs"][k].items() if f not in legs_but}
        assert la == lb, (k, la, lb)
    assert a["inlier_mask"].shape == b["inlier_mask"].shape and np.array_equal(a["inlier_mask"], b["inlier_mask"])
    for k in ("E", "F", "H", "cam2_from_cam1"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["tri_angle"] == b["tri_angle"]


def _pair(kind, n, outliers, noise, seed):
    return _args(TV.synthetic_pair(kind, n, outliers, seed=seed, noise_px=noise))


K1, K2 = np.array(TV.NR.INTR1), np.array(TV.NR.INTR2)
OPTS = dict(compute_relative_pose=True, seed=3, max_num_trials=600)
_cache = {}


def _mixed():
    """the issue's mixed batch (pairs, their single calls), built once"""
    if "mixed" not in _cache:
        g50 = _pair("general", 50, 0.2, 0.0, 100)
        empty = (np.zeros((0, 2)), np.zeros((0, 2)), K1, K2, TV.SIZE1, TV.SIZE2)
        same = (np.tile([[400.0, 300.0]], (40, 1)), np.tile([[350.0, 320.0]], (40, 1)), K1, K2, TV.SIZE1, TV.SIZE2)
        pairs = [g50, empty, _pair("general", 14, 0.0, 0.0, 101), _pair("general", 300, 0.5, 0.5, 102), _pair("planar", 1000, 0.5, 0.5, 103),
                 _pair("rotation", 800, 0.5, 0.5, 104), _pair("watermark", 400, 0.2, 0.5, 105), _pair("weak", 60, 0.83, 0.5, 106),
                 _pair("wrong_intrinsics", 500, 0.2, 0.5, 107), _pair("general", 3000, 0.5, 0.5, 108), same,
                 _pair("general", 70000, 0.2, 0.5, 109)]
        _cache["mixed"] = (pairs, [capi.two_view_geometry(*p, **OPTS) for p in pairs])
    return _cache["mixed"]


def test_mixed_batch_equals_the_loop_of_single_calls():
    pairs, single = _mixed()
    got = capi.two_view_geometry_batch(pairs, **OPTS)
    assert len(got) == len(pairs)
    for k, (a, b) in enumerate(zip(got, single)):
        print(k, "n", len(pairs[k][0]), "config", b["config"], {g: (v["num_trials"], v["lo_rounds"], v["num_batches"]) for g, v in b["legs"].items()})
        _identical(a, b)
    assert single[6]["legs"]["T"]["num_trials"] > 0  # the watermark pair reaches the translation leg
    assert {1, 2, 3, 4, 5, 7} <= {r["config"] for r in single}


def test_legs_that_do_not_exist():
    s = TV.synthetic_pair("general", 20, 0.0, seed=110, noise_px=0.0)
    pairs = [(s["points1"][:n], s["points2"][:n], s["intr1"], s["intr2"], s["size1"], s["size2"]) for n in (3, 4, 5, 6, 7, 8, 20)]
    o = dict(compute_relative_pose=True, seed=3, max_num_trials=600, min_num_inliers=0)
    single = [capi.two_view_geometry(*p, **o) for p in pairs]
    ran = [[g for g in "EFH" if r["legs"][g]["num_trials"] > 0] for r in single]
    assert ran == [[], ["H"], ["E", "H"], ["E", "H"], ["E", "F", "H"], ["E", "F", "H"], ["E", "F", "H"]] and single[0]["config"] == 1
    for a, b in zip(capi.two_view_geometry_batch(pairs, **o), single):
        _identical(a, b)


def test_group_size_and_order_do_not_matter():
    pairs, single = _mixed()
    pairs, single = pairs[:-1], single[:-1]
    for g in (1, 2, 5, 0):
        got, rep = capi.two_view_geometry_batch(pairs, pairs_per_group=g, return_report=True, **OPTS)
        assert rep["num_groups"] == {1: 11, 2: 6, 5: 3, 0: 1}[g]
        for a, b in zip(got, single):
            _identical(a, b)
    for a, b in zip(capi.two_view_geometry_batch(pairs[::-1], **OPTS), single[::-1]):
        _identical(a, b)


def test_batch_size_does_not_change_the_result():
    pairs = [_pair(kind, 3000, 0.5, 0.5, 21) for kind in ("general", "planar", "watermark")]
    o = dict(compute_relative_pose=True, seed=5, max_num_trials=700)
    base = capi.two_view_geometry_batch(pairs, **o)
    for a, p in zip(base, pairs):
        _identical(a, capi.two_view_geometry(*p, **o))
    for batch in (1, 7, 256):
        for a, b in zip(capi.two_view_geometry_batch(pairs, batch_trials=batch, **o), base):
            _identical(a, b, legs_but=("num_batches",))


def test_lockstep_one_synchronisation_serves_all_pairs():
    p = _pair("general", 1000, 0.3, 0.5, 120)
    _, one = capi.two_view_geometry_batch([p], pairs_per_group=16, return_report=True, **OPTS)
    got, many = capi.two_view_geometry_batch([p] * 16, pairs_per_group=16, return_report=True, **OPTS)
    print("one", one, "sixteen copies", many)
    assert many["num_groups"] == one["num_groups"] == 1 and many["num_syncs"] == one["num_syncs"] and many["num_launches"] == one["num_launches"]
    for a in got[1:]:
        _identical(a, got[0])
    pairs, _ = _mixed()
    pairs = pairs[:-1]
    _, mixed = capi.two_view_geometry_batch(pairs, pairs_per_group=16, return_report=True, **OPTS)
    alone = [capi.two_view_geometry_batch([q], pairs_per_group=16, return_report=True, **OPTS)[1]["num_syncs"] for q in pairs]
    print("mixed", mixed, "alone", alone)
    assert mixed["num_syncs"] < sum(alone) and mixed["num_syncs"] >= max(alone)


def test_two_host_threads_agree_with_the_serial_result():
    batches = [[_pair(kind, 2000, 0.4, 0.5, 41 + 3 * i + j) for j, kind in enumerate(("general", "planar", "watermark"))] for i in range(2)]
    batches[1] = batches[1][::-1]
    o = dict(compute_relative_pose=True, seed=2, max_num_trials=700)
    serial = [capi.two_view_geometry_batch(b, **o) for b in batches]
    out, err = [None, None], []

    def work(i):
        try:
            for _ in range(3):
                out[i] = capi.two_view_geometry_batch(batches[i], **o)
        except Exception as e:  # noqa: BLE001
            err.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not err, err
    for sa, sb in zip(serial, out):
        for a, b in zip(sa, sb):
            _identical(a, b)


class _Cam:
    def __init__(self, params, size):
        self.model, self.params, self.width, self.height = "PINHOLE", np.asarray(params, np.float64), size[0], size[1]


class _Image:
    def __init__(self, name, image_id, camera_id):
        self.name, self.image_id, self.camera_id = name, image_id, camera_id


class _Reconstruction:
    def __init__(self):
        self.images, self.cameras = {}, {}


def test_end_to_end_geometric_verification_batched_equals_the_loop():
    """The three scene pairs of test_end_to_end_geometric_verification_of_three_scene_pairs, built the same way."""
    from mpsfm_amd.synthetic import R_from_quat, make_scene

    prob, truth = make_scene(6, 3000, False, seed=4, outlier_frac=0.1)
    rng = np.random.default_rng(7)
    rec, kps, matches, names_all = _Reconstruction(), {}, {}, []
    for a, b in [(0, 1), (1, 2), (2, 3)]:
        K = prob.cam_intr[prob.cam_intr_idx[a]]
        size = (int(round(2 * K[2])), int(round(2 * K[3])))
        common = sorted(set(prob.obs_pt[prob.obs_cam == a].tolist()) & set(prob.obs_pt[prob.obs_cam == b].tolist()))
        X = truth["pts"][np.array(common)]
        Ra, Rb = R_from_quat(truth["cam_quat"][a])[0], R_from_quat(truth["cam_quat"][b])[0]
        ta, tb = truth["cam_t"][a], truth["cam_t"][b]

        def project(R, t, K=K, X=X):
            Y = X @ R.T + t
            return np.c_[K[0] * Y[:, 0] / Y[:, 2] + K[2], K[1] * Y[:, 1] / Y[:, 2] + K[3]]

        pa, pb = project(Ra, ta), project(Rb, tb)
        Rr = Rb @ Ra.T
        tr = tb - Rr @ ta
        Ki = np.linalg.inv(TV.Kmat(K))
        F = Ki.T @ np.array([[0, -tr[2], tr[1]], [tr[2], 0, -tr[0]], [-tr[1], tr[0], 0]]) @ Rr @ Ki
        for i in np.nonzero(rng.random(len(common)) < 0.1)[0]:
            line = F @ np.r_[pa[i], 1.0]
            while True:
                q = pb[i] + rng.uniform(-80, 80, 2)
                if abs(line @ np.r_[q, 1.0]) > 40.0 * np.hypot(line[0], line[1]):
                    break
            pb[i] = q
        names = (f"im{a}_{b}_0.jpg", f"im{a}_{b}_1.jpg")
        for j, (name, kp) in enumerate(zip(names, (pa, pb))):
            iid = 10 * a + j + 1
            rec.images[iid] = _Image(name, iid, iid)
            rec.cameras[iid] = _Cam(K, size)
            kps[name] = kp
        perm = rng.permutation(len(common))
        matches[names] = np.c_[perm, perm].astype(np.int32)
        names_all.append(names)
    masks, cache = geometric_verification(rec, names_all, max_error=4.0, keypoints=kps, matches=matches)
    bmasks, bcache = geometric_verification(rec, names_all, max_error=4.0, keypoints=kps, matches=matches, batched=True)
    assert list(masks) == list(bmasks) == names_all and list(cache) == list(bcache)
    for names in names_all:
        assert bmasks[names].dtype == bool and np.array_equal(masks[names], bmasks[names]) and masks[names].sum() > 400
        a, b = cache[names], bcache[names]
        _identical(b.estimate, a.estimate)
        assert a.config == b.config == 2 and np.array_equal(a.inlier_matches, b.inlier_matches) and a.tri_angle == b.tri_angle
        assert a.cam2_from_cam1.matrix().tobytes() == b.cam2_from_cam1.matrix().tobytes()
