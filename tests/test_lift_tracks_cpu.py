"""CPU tests of the batched depth lifting (MpsfmTriangulator(..., lift="batch"), csrc/lift_tracks.hip): the host side of
the drop-in driven through the NumPy restatement of the kernel (tests/numpy_lift_tracks.py) against the per-point loop
(`_lift_points`, the reference's mpsfm/sfm/mapper/triangulator.py:49-83), and the bulk form of retriangulate()'s count
of safe points.

Bounds (derived, not measured).  Ids, id order, track elements and their order, keypoint bookkeeping: exact.  Lifted
coordinates: per component |d| <= 16 eps (|ray d| + |t|), the bound tests/test_registration_cpu.py derives for the same
formula (the loop rotates with R^T p - R^T t through a quaternion round trip, the kernel with R^T (p - t))."""

import copy

import numpy as np
import pytest

import numpy_lift_tracks as NL
from mpsfm_amd.sfm.mapper.triangulator import MpsfmTriangulator, tracks_from_scene
from mpsfm_amd.synthetic import make_scene
from numpy_scene import scene_from_problem
from test_observations_cpu import assert_same_state, oracle_numerics
from test_registration_cpu import assert_lift_close


def lift_scene(map_size=(129, 97)):
    """The scene of test_gpu_seam.py's lifting test with one image of every kind the lift has to step over."""
    prob, truth = make_scene(6, 300, True, seed=11)
    sc = scene_from_problem(prob, truth, map_size=map_size, seed=1)
    ims = sorted(sc.images)
    W, H = map_size
    sc.images[ims[0]].depth.activated = False
    sc.images[ims[1]].depth.valid[:, : W // 2] = 0
    sc.images[ims[2]].depth.data[H // 3:, :] = -1.0
    sc.images[ims[3]].kps[::2] += 1.0e5  # off the map
    return sc


def midpoint_threshold_deg(ang):
    """Between two neighbouring sorted angles near the median: no angle within rounding of the threshold."""
    s = np.unique(ang)
    k = len(s) // 2
    assert s[k] - s[k - 1] > 1e-9
    return float(np.rad2deg(0.5 * (s[k - 1] + s[k])))


def first_lifting_element(sc, pid):
    """The loop's rule by the loop's own accessors: position of the first element that would lift, -1 for none."""
    for k, el in enumerate(sc.points3D[pid].track.elements):
        image = sc.images[el.image_id]
        if image.depth.activated and image.depth.valid_at_kps(np.array([image.points2D[el.point2D_idx].xy]))[0]:
            return k
    return -1


class Recorder:
    """The restatement as the drop-in's backend, keeping what it returned."""

    def __init__(self, backend):
        self.backend, self.calls = backend, []

    def __call__(self, *args, **kwargs):
        self.calls.append(self.backend(*args, **kwargs))
        return self.calls[-1]


def elements_of(sc, pid):
    return [(e.image_id, e.point2D_idx) for e in sc.points3D[pid].track.elements]


def check_batch_against_loop(a, b, ids, new_a, new_b, out, before, first):
    """a: after lift="batch", b: after the loop, `out`: what the backend returned, `before`: {pid: elements} and `first`:
    {pid: position of the lifting element by the loop's rule} of the risky points before the run."""
    assert new_a == new_b and len(new_a) > 0
    assert_same_state(a, b)
    risky = np.flatnonzero(out["risky"])
    assert [int(ids[k]) for k in risky] == list(before)
    np.testing.assert_array_equal(out["lift_el"][risky], [first[p] for p in before])
    lifted = risky[out["lift_el"][risky] >= 0]
    assert len(lifted) == len(new_a)
    for pid in new_a:
        assert elements_of(a, pid) == elements_of(b, pid)  # the same elements in the same order
    got = np.array([a.points3D[p].xyz for p in new_a])
    want = np.array([b.points3D[p].xyz for p in new_b])
    return got, want, lifted


def assert_every_branch(el, before, new_elements):
    """lifted by element 0, lifted by a later element, deleted without a lift, an element dropped by cheirality; `el`: the
    position of the lifting element per risky point, `before` / `new_elements`: the tracks before and after"""
    el = np.asarray(el)
    assert (el == 0).sum() > 0 and (el > 0).sum() > 0 and (el < 0).sum() > 0, np.bincount(el + 1)
    lifted_before = [els for els, e in zip(before.values(), el) if e >= 0]
    dropped = sum(len(o) - len(n) for o, n in zip(lifted_before, new_elements))
    assert dropped > 0 and all(set(n) <= set(o) for o, n in zip(lifted_before, new_elements))
    return dict(by_first=int((el == 0).sum()), by_later=int((el > 0).sum()), no_lift=int((el < 0).sum()), dropped=int(dropped))


@pytest.fixture(scope="module")
def runs():
    sc = lift_scene()
    ids = np.array(sorted(sc.points3D))
    tr, _ = tracks_from_scene(sc, ids)
    ang, _, _ = oracle_numerics(tr, sc.point3D_coordinates(ids), 0)
    thr = midpoint_threshold_deg(ang)
    risky_ids = [int(p) for p in ids[ang < np.deg2rad(thr)]]
    before = {p: elements_of(sc, p) for p in risky_ids}
    first = {p: first_lifting_element(sc, p) for p in risky_ids}
    a, b = copy.deepcopy(sc), copy.deepcopy(sc)
    backend = Recorder(NL.lift_tracks)
    new_a = MpsfmTriangulator({"colmap_options": {}}, a, None, lift="batch", lift_backend=backend).lift_low_parallax(ids, thr)
    tri_b = MpsfmTriangulator({"colmap_options": {}}, b, None, lift="loop")
    new_b = tri_b._lift_points(ids[ang < np.deg2rad(thr)])  # the loop with the same angles
    return dict(sc=sc, ids=ids, thr=thr, a=a, b=b, new_a=new_a, new_b=new_b, calls=backend.calls, before=before, first=first)


def test_batch_lift_through_the_restatement_equals_the_loop(runs):
    r = runs
    assert len(r["calls"]) == 1  # one call replaces the angle call and the loop
    out = r["calls"][0]
    got, want, lifted = check_batch_against_loop(r["a"], r["b"], r["ids"], r["new_a"], r["new_b"], out, r["before"], r["first"])
    assert_lift_close(got, want, out["scale"][lifted])
    # the loop alone takes every branch on this scene
    seen = assert_every_branch([r["first"][p] for p in r["before"]], r["before"], [elements_of(r["b"], p) for p in r["new_b"]])
    print(seen)
    assert out["info"]["n_risky"] == len(r["before"]) and out["info"]["n_lifted"] == len(r["new_b"])
    assert out["info"]["n_no_lift"] == seen["no_lift"]


def test_default_is_the_loop_and_unknown_modes_are_refused():
    sc = lift_scene()
    tri = MpsfmTriangulator({"colmap_options": {}}, sc, None)
    assert tri.lift == "loop" and tri.lift_backend is None
    assert sorted(MpsfmTriangulator.default_conf) == sorted(["hard_angle", "colmap_options", "new_retry_nbatch", "re_ignore_two_view_tracks",
                                                             "retri_min_angle", "lift_low_parallax", "nsafe_threshold", "verbose"])
    with pytest.raises(ValueError):
        MpsfmTriangulator({"colmap_options": {}}, sc, None, lift="wave")
    assert MpsfmTriangulator({"colmap_options": {}}, sc, None, lift="batch", lift_backend=NL.lift_tracks).lift_low_parallax([], 1.5) == []


class _NoBulk:
    """The scene without the optional bulk accessor."""

    def __init__(self, sc):
        self._sc = sc

    def __getattr__(self, name):
        if name == "point3D_track_lengths":
            raise AttributeError(name)
        return getattr(self._sc, name)


class _Engine:
    def __init__(self):
        self.seen = []

    def retriangulate(self, options, imids):
        self.seen.append(imids)
        return 0


def test_safe_point_count_in_bulk_gives_the_same_risky_images(runs):
    sc = copy.deepcopy(runs["b"])  # after a lift: tracks of many lengths, shortened ones among them
    sc.obs.delete_observation(*elements_of(sc, runs["new_b"][0])[0])  # and one shortened through the manager

    def old_nsafe(imid):
        image = sc.images[imid]
        p3d = set(image.point3D_ids(image.get_observation_point2D_idxs()))
        return sum(1 for p in p3d if len(sc.points3D[p].track.elements) > 2)

    counts = {imid: old_nsafe(imid) for imid in sc.registered_images}
    assert len(set(counts.values())) > 2
    thr = int(np.median(list(counts.values())))
    want = [imid for imid in sc.registered_images if counts[imid] < thr]
    assert 0 < len(want) < len(counts)
    want = want + sum((sc.find_local_bundle_ids(i, 1) for i in want), [])
    conf = {"colmap_options": {}, "nsafe_threshold": thr, "new_retry_nbatch": 1}
    for scene in (sc, _NoBulk(sc)):
        tri = MpsfmTriangulator(conf, copy.deepcopy(scene) if scene is sc else scene, None, _Engine(), lift="batch", lift_backend=NL.lift_tracks)
        assert [tri._num_safe_points(i) for i in counts] == list(counts.values())
        assert hasattr(tri.mpsfm_rec, "point3D_track_lengths") == (scene is sc)
        tri.retriangulate()
        assert tri._triangulator.seen == [set(want)]
