"""Scene queries without a device: the restatement (tests/numpy_scene_queries.py) on cases worked out by hand, every path of the
local-bundle walk on scenes placed by hand together with the margins that let the GPU tests compare decisions exactly, and the
argument checks of the two entry points, which return before any device is touched."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import numpy_scene_queries as NQ
from mpsfm_amd import capi
from mpsfm_amd.baseclass import to_conf
from mpsfm_amd.sfm.scene.scene_queries import SceneQueries

EINVAL, ENODEVICE = -1, -2


# ---- the visibility pyramid by hand ----------------------------------------------------------------------------------------------------
def _one_image(xy, width=640, height=480, num_levels=6, linked=None):
    """Image 0 with the keypoints `xy`, image 1 with one keypoint that has a point and is matched to the keypoints `linked` of image 0
    (all by default): exactly those are visible."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    n = len(xy)
    linked = list(range(n)) if linked is None else list(linked)
    kp_start = np.array([0, n, n + 1], np.int64)
    corr_start = np.zeros(n + 2, np.int64)
    for k in linked:
        corr_start[k + 1] = 1
    corr_start[n + 1] = len(linked)
    corr_start = np.cumsum(corr_start)
    corr_kp = np.array([n] * len(linked) + linked, np.int64)
    kp_point = np.array([-1] * n + [0], np.int64)
    size = np.array([[width, height], [width, height]], np.int32)
    return kp_start, np.concatenate([xy, [[1.0, 1.0]]]), corr_start, corr_kp, kp_point, size, num_levels


def test_one_visible_keypoint_scores_the_sum_of_4_to_the_l():
    out = NQ.visibility(*_one_image([[100.5, 200.25], [3.0, 4.0]], linked=[0]))
    assert out["num_visible"].tolist() == [1, 0] and out["kp_visible"].tolist() == [1, 0, 0]
    assert out["score"].tolist() == [sum(4**l for l in range(1, 7)), 0] == [5460, 0]


def test_all_4096_finest_cells_occupied():
    xs, ys = np.meshgrid((np.arange(64) + 0.5) * 10.0, (np.arange(64) + 0.5) * 7.5)  # 640 x 480: cells of 10 x 7.5
    out = NQ.visibility(*_one_image(np.stack([xs.ravel(), ys.ravel()], 1)))
    assert out["num_visible"][0] == 4096 and out["score"][0] == 17_895_696 == sum(16**l for l in range(1, 7))


@pytest.mark.parametrize("x, cell", [(-0.5, 0), (-1e300, 0), (float("nan"), 0), (640.0, 63), (1e300, 63), (float("inf"), 63), (639.999, 63),
                                     (30.0, 3), (np.nextafter(30.0, 0.0), 2), (0.0, 0)])
def test_cell_of_an_x_outside_the_image_and_on_a_cell_edge(x, cell):
    assert NQ.pyramid_cell(x, 640, 64) == cell


def test_a_width_that_is_no_power_of_two():
    # 1000 / 64 = 15.625 per cell: x = 31.25 is the edge of cell 2 exactly, 31.249 lies in cell 1; 999.99 in cell 63
    assert [NQ.pyramid_cell(x, 1000, 64) for x in (31.25, 31.249, 15.625, 999.99, 500.0)] == [2, 1, 1, 63, 32]
    a = NQ.visibility(*_one_image([[31.25, 10.0], [47.0, 10.0]], width=1000, height=750))
    b = NQ.visibility(*_one_image([[31.25, 10.0], [31.26, 10.0]], width=1000, height=750))
    c = NQ.visibility(*_one_image([[31.25, 10.0], [31.249, 10.0]], width=1000, height=750))
    # cells 2 and 3 share every coarser cell; one finest cell seen twice; cells 2 and 1 part at level 5 as well (parents 1 and 0)
    assert a["score"][0] == 5460 + 4**6 and b["score"][0] == 5460 and c["score"][0] == 5460 + 4**6 + 4**5
    assert a["num_visible"][0] == b["num_visible"][0] == c["num_visible"][0] == 2


def test_visibility_does_not_count_the_keypoint_s_own_point():
    kp_start, xy, corr_start, corr_kp, kp_point, size, L = _one_image([[5.0, 5.0]])
    kp_point[:] = [3, -1]  # the keypoint of image 0 has a point, its partner has none
    out = NQ.visibility(kp_start, xy, corr_start, corr_kp, kp_point, size, L)
    assert out["num_visible"].tolist() == [0, 1] and out["kp_visible"].tolist() == [0, 1]


# ---- every path of the walk ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(NQ.walk_cases()))
def test_walk_paths_on_scenes_placed_by_hand(name):
    scene, ref, num_images, expected = NQ.walk_cases()[name]
    out = NQ.local_bundle(*NQ.state_args(scene), ref, num_images, NQ.MIN_TRI_ANGLE_DEG)
    NQ.assert_margins(out)  # the margin condition: the GPU tests reuse these scenes and compare the decisions exactly
    assert out["bundle"] == expected
    took_all = len(expected) == int((out["shared"] > 0).sum())
    assert (len(out["compared"]) == 0) == took_all  # the shortcut compares nothing, every other scene walks


def test_walk_paths_take_the_paths_their_names_say():
    cases = NQ.walk_cases()
    out = {name: NQ.local_bundle(*NQ.state_args(sc), ref, n, NQ.MIN_TRI_ANGLE_DEG) for name, (sc, ref, n, _) in cases.items()}
    rad = NQ.MIN_TRI_ANGLE_DEG * np.pi / 180.0
    # third threshold: image 1 was refused at rad and rad / 1.5 and taken at rad / 2
    mine = [thr for a, thr in out["third threshold"]["compared"] if a == out["third threshold"]["angle75"][1]]
    assert np.allclose(mine, [rad, rad / 1.5, rad / 2.0], rtol=1e-15)
    # overlap break: image 3 (the widest angle) was never compared
    assert out["overlap break"]["angle75"][3] > rad and all(a != out["overlap break"]["angle75"][3] for a, _ in out["overlap break"]["compared"])
    # fill up: nothing passed a comparison
    assert all(a < thr for a, thr in out["fill up"]["compared"]) and len(out["fill up"]["compared"]) > 8
    # ties: images 1, 3 and 4 share 6 points with the reference
    assert out["ties"]["shared"].tolist() == [0, 6, 7, 6, 6]
    # multiplicity: the reference's two keypoints on point 0 count twice for image 2; image 2's two keypoints on point 1 give two angles
    assert out["multiplicity"]["shared"].tolist() == [0, 4, 5] and len(out["multiplicity"]["angles"]) == 8


def test_percentile_rounds_half_up_at_every_residue():
    for n, rank in ((1, 0), (2, 1), (3, 2), (4, 2), (5, 3), (255, 191), (256, 191), (257, 192)):
        assert NQ.percentile75(list(range(n))) == rank == (3 * (n - 1) + 2) // 4


def test_unregistered_images_are_ignored_and_the_zero_angle():
    sc = NQ.order_statistic_scene([5, 5, 5], zero_at=2)
    out = NQ.local_bundle(*NQ.state_args(sc), 0, 10, NQ.MIN_TRI_ANGLE_DEG)
    NQ.assert_margins(out, zero_allowed=True)
    assert min(out["angles"]) == 0.0 and out["bundle"] == [1, 2, 3]
    sc["registered"][2] = 0
    out = NQ.local_bundle(*NQ.state_args(sc), 0, 10, NQ.MIN_TRI_ANGLE_DEG)
    assert out["bundle"] == [1, 3] and out["shared"][2] == 0 and out["angle75"][2] == -1.0


def test_local_ba_options_are_looked_up_as_the_reference_does():
    q = SceneQueries.__new__(SceneQueries)
    q.rec = SimpleNamespace()  # a scene without a conf: COLMAP's defaults
    assert q._local_ba_options() == (6, 6.0) and q._local_ba_options(4) == (4, 6.0)
    q.rec = SimpleNamespace(conf=to_conf({"colmap_options": "<--->"}))
    assert q._local_ba_options() == (6, 6.0)
    q.rec = SimpleNamespace(conf=to_conf({"colmap_options": {"local_ba_num_images": 9, "local_ba_min_tri_angle": 3.5, "ba_refine_focal_length": False}}))
    assert q._local_ba_options() == (9, 3.5) and q._local_ba_options(num_images=2) == (2, 3.5)


# ---- argument checks, before any device ------------------------------------------------------------------------------------------------
def _rc(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except capi.MpsfmHipError as e:
        return e.code
    return 0


def test_visibility_scores_checks_arguments_before_any_device():
    good = list(_one_image([[5.0, 5.0], [6.0, 6.0]]))

    def call(**changes):
        a = dict(zip(("kp_start", "kp_xy", "corr_start", "corr_kp", "kp_point", "image_size", "num_levels"), good))
        a.update(changes)
        return _rc(capi.visibility_scores, **a)

    for name in ("kp_start", "kp_xy", "corr_start", "corr_kp", "kp_point", "image_size"):
        assert call(**{name: None}) == EINVAL, name
    assert call(num_levels=0) == EINVAL and call(num_levels=9) == EINVAL
    assert call(kp_start=np.array([1, 2, 3], np.int64)) == EINVAL and b"kp_start" in capi.lib().mpsfm_last_error()
    assert call(kp_start=np.array([0, 3, 2], np.int64)) == EINVAL
    assert call(corr_start=np.array([1, 1, 2, 4], np.int64)) == EINVAL
    assert call(corr_start=np.array([0, 2, 1, 4], np.int64)) == EINVAL
    assert call(corr_kp=np.array([2, 2, 0, 3], np.int64)) == EINVAL and call(corr_kp=np.array([2, -1, 0, 1], np.int64)) == EINVAL
    assert call(image_size=np.array([[640, 0], [640, 480]], np.int32)) == EINVAL
    # NULL outputs, a negative count: the raw entry point
    L = capi.lib()
    p = [a.ctypes.data for a in good[:6]]
    nv, sc = np.zeros(2, np.int32), np.zeros(2, np.int64)
    assert L.mpsfm_visibility_scores(2, *p, 6, 0, None, sc.ctypes.data, None, None) == EINVAL
    assert L.mpsfm_visibility_scores(2, *p, 6, 0, nv.ctypes.data, None, None, None) == EINVAL
    assert L.mpsfm_visibility_scores(-1, *p, 6, 0, nv.ctypes.data, sc.ctypes.data, None, None) == EINVAL
    # valid input reaches the device check, and only then
    assert call() in (0, ENODEVICE)
    # no keypoints: zeros without a device
    out = capi.visibility_scores(np.zeros(3, np.int64), None, None, None, None, np.array([[4, 4], [4, 4]], np.int32))
    assert out["num_visible"].tolist() == [0, 0] and out["score"].tolist() == [0, 0] and out["info"]["num_syncs"] == 0


def test_local_bundles_checks_arguments_before_any_device():
    scene, ref, num_images, _ = NQ.walk_cases()["third threshold"]

    def call(ref_image=(ref,), num_images=num_images, angle=6.0, **changes):
        a = dict(scene)
        a.update(changes)
        return _rc(capi.local_bundles, *NQ.state_args(a), list(ref_image), num_images, angle)

    assert call(num_images=0) == EINVAL and call(num_images=-3) == EINVAL
    assert call(ref_image=[5]) == EINVAL and call(ref_image=[-1]) == EINVAL
    reg = scene["registered"].copy()
    reg[0] = 0
    assert call(registered=reg) == EINVAL and b"not registered" in capi.lib().mpsfm_last_error()
    kp_start = scene["kp_start"].copy()
    kp_start[0] = 1
    assert call(kp_start=kp_start) == EINVAL
    kp_point = scene["kp_point"].copy()
    kp_point[3] = len(scene["xyz"])
    assert call(kp_point=kp_point) == EINVAL
    kp_point[3] = -2
    assert call(kp_point=kp_point) == EINVAL
    xyz = scene["xyz"].copy()
    xyz[1, 2] = np.nan
    assert call(xyz=xyz) == EINVAL
    t = scene["cam_t"].copy()
    t[2, 0] = np.inf
    assert call(cam_t=t) == EINVAL
    assert call(angle=-1.0) == EINVAL and call(angle=float("nan")) == EINVAL
    # NULL pointers and a negative count: the raw entry point
    L = capi.lib()
    st = capi.CTriState(scene["registered"].ctypes.data, scene["cam_quat_xyzw"].ctypes.data, scene["cam_t"].ctypes.data,
                        scene["kp_point"].ctypes.data, len(scene["xyz"]), scene["xyz"].ctypes.data)
    n = len(scene["registered"])
    refs, bundle, blen = np.array([0], np.int32), np.zeros(2, np.int32), np.zeros(1, np.int32)
    shared, a75 = np.zeros(n, np.int32), np.zeros(n)
    args = [n, scene["kp_start"].ctypes.data, C.addressof(st), 1, refs.ctypes.data, 3, 6.0, 0, bundle.ctypes.data, blen.ctypes.data,
            shared.ctypes.data, a75.ctypes.data, None]
    for i in (1, 2, 4, 8, 9, 10, 11):
        bad = list(args)
        bad[i] = None
        assert L.mpsfm_local_bundles(*bad) == EINVAL, i
    assert L.mpsfm_local_bundles(*([-1] + args[1:])) == EINVAL and L.mpsfm_local_bundles(*(args[:3] + [-1] + args[4:])) == EINVAL
    st.xyz = None
    assert L.mpsfm_local_bundles(*args) == EINVAL
    assert call() in (0, ENODEVICE)
    # nothing can be shared (no keypoint has a point): the empty answer without a device
    out = capi.local_bundles(*NQ.state_args(dict(scene, kp_point=np.full(len(scene["kp_point"]), -1, np.int64))), [0, 0], 3, 6.0)
    assert out["bundle"].tolist() == [[-1, -1], [-1, -1]] and out["bundle_len"].tolist() == [0, 0]
    assert not out["shared"].any() and (out["angle75"] == -1.0).all() and out["info"]["num_syncs"] == 0
