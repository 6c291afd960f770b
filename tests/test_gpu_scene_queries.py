"""mpsfm_visibility_scores and mpsfm_local_bundles (csrc/scene_queries.hip) against the restatement of tests/numpy_scene_queries.py,
through the C ABI and through SceneQueries / ImageSelection.  Integer outputs and decisions are compared exactly (the scenes keep
the margins that tests/test_scene_queries_cpu.py asserts), angle75 within 1e-12 rad, the bound tests/test_gpu_seam.py uses for
tri_angle against its oracle."""
from types import SimpleNamespace

import numpy as np
import pytest

import numpy_scene_queries as NQ
from mpsfm_amd import capi
from mpsfm_amd.sfm.mapper.image_selection import VISIBILITY_METHODS, ImageSelection
from mpsfm_amd.sfm.mapper.track_engine import state_arrays
from mpsfm_amd.sfm.scene.scene_queries import SceneQueries
from mpsfm_amd.synthetic import make_scene
from numpy_scene import INVALID_POINT3D, correspondences_from_problem, scene_from_problem

pytestmark = pytest.mark.gpu

ANGLE_ATOL = 1e-12
WORKGROUP = 256      # threads of k_sq_visibility
SELECT_LDS = 2048    # angles k_lb_select keeps in LDS


# ---- visibility ------------------------------------------------------------------------------------------------------------------------
def _visibility_input(seed=3):
    """Images of 0, 1, 63, 64, 65, one more than the workgroup and 5000 keypoints (the stride loop) plus one of 300; rows of 0, 1 and
    100 entries; widths that are no power of two; coordinates outside the image, on cell edges, NaN and infinite."""
    rng = np.random.default_rng(seed)
    counts = [0, 1, 63, 64, 65, WORKGROUP + 1, 5000, 300, 0]
    sizes = np.array([[640, 480], [640, 480], [1000, 750], [641, 479], [1600, 1200], [97, 33], [640, 480], [1000, 750], [8, 8]], np.int32)
    kp_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    n_kp = int(kp_start[-1])
    image_of = np.repeat(np.arange(len(counts)), counts)
    wh = sizes[image_of].astype(np.float64)
    xy = rng.uniform(-0.05, 1.05, (n_kp, 2)) * wh
    big = int(kp_start[6])  # the image of 5000 keypoints, 640 x 480: cells of 10 x 7.5 at 6 levels
    xy[big:big + 12] = [[-3.0, 5.0], [640.0, 5.0], [5.0, 480.0], [5.0, -1e-9], [30.0, 7.5], [np.nextafter(30.0, 0), np.nextafter(7.5, 0)],
                        [np.nan, 5.0], [5.0, np.nan], [np.inf, 5.0], [-np.inf, np.inf], [639.999, 479.999], [0.0, 0.0]]
    a, b = rng.integers(0, n_kp, 3000), rng.choice(np.flatnonzero(image_of != 6), 3000)  # few pairs inside the large image
    a[:12], b[:12] = np.arange(big, big + 12), int(kp_start[7]) + np.arange(12)     # the special coordinates have partners
    a[12:112], b[12:112] = big + 20, np.r_[int(kp_start[2]) + np.arange(50), int(kp_start[7]) + 20 + np.arange(50)]  # a row of 100
    a[112], b[112] = int(kp_start[1]), int(kp_start[7]) + 100                        # the image of one keypoint
    keep = image_of[a] != image_of[b]
    a, b = a[keep], b[keep]
    und = np.unique(np.stack([np.minimum(a, b), np.maximum(a, b)], 1), axis=0)
    src, dst = np.r_[und[:, 0], und[:, 1]], np.r_[und[:, 1], und[:, 0]]
    order = np.lexsort((dst, src))
    src, dst = src[order], dst[order]
    corr_start = np.searchsorted(src, np.arange(n_kp + 1)).astype(np.int64)
    kp_point = np.where(rng.uniform(size=n_kp) < 0.4, rng.integers(0, 50, n_kp), -1).astype(np.int64)
    kp_point[int(kp_start[7]):int(kp_start[7]) + 120] = 7  # the partners of the special keypoints have points
    rows = np.diff(corr_start)
    assert rows.min() == 0 and (rows == 1).any() and rows.max() >= 100
    return kp_start, xy, corr_start, dst.astype(np.int64), kp_point, sizes


@pytest.fixture(scope="module")
def visibility_input():
    return _visibility_input()


@pytest.mark.parametrize("num_levels", [1, 6, 8])
def test_visibility_equals_the_restatement_exactly(visibility_input, num_levels):
    want = NQ.visibility(*visibility_input, num_levels=num_levels)
    got = capi.visibility_scores(*visibility_input, num_levels=num_levels)
    print("num_visible", got["num_visible"].tolist(), "score", got["score"].tolist())
    np.testing.assert_array_equal(got["kp_visible"], want["kp_visible"])
    np.testing.assert_array_equal(got["num_visible"], want["num_visible"])
    np.testing.assert_array_equal(got["score"], want["score"])
    assert got["score"].dtype == np.int64 and got["num_visible"][[0, 8]].tolist() == [0, 0] and got["num_visible"][1] == 1
    big = int(visibility_input[0][6])
    assert want["kp_visible"][big + WORKGROUP:big + 5000].any()  # the stride loop met visible keypoints
    assert got["info"]["num_syncs"] == 1 and got["info"]["num_launches"] == 1
    again = capi.visibility_scores(*visibility_input, num_levels=num_levels, return_kp_visible=False)
    assert again["kp_visible"] is None
    assert again["score"].tobytes() == got["score"].tobytes() and again["num_visible"].tobytes() == got["num_visible"].tobytes()


def test_visibility_of_a_full_pyramid_at_8_levels():
    """All 65536 finest cells of one image occupied: every word of the bitmap full, every fold level at its maximum."""
    xs, ys = np.meshgrid(np.arange(256) + 0.5, np.arange(256) + 0.5)
    xy = np.concatenate([np.stack([xs.ravel(), ys.ravel()], 1), [[1.0, 1.0]]])
    n = 65536
    kp_start = np.array([0, n, n + 1], np.int64)
    corr_start = np.r_[np.arange(n + 1), 2 * n].astype(np.int64)
    corr_kp = np.r_[np.full(n, n), np.arange(n)].astype(np.int64)
    kp_point = np.r_[np.full(n, -1), 0].astype(np.int64)
    got = capi.visibility_scores(kp_start, xy, corr_start, corr_kp, kp_point, np.array([[256, 256], [256, 256]], np.int32), num_levels=8)
    assert got["num_visible"].tolist() == [n, 0] and got["score"].tolist() == [sum(16**l for l in range(1, 9)), 0]


# ---- local bundles ---------------------------------------------------------------------------------------------------------------------
def _check_rows(got, row, want, width):
    np.testing.assert_array_equal(got["shared"][row], want["shared"])
    err = np.abs(got["angle75"][row] - want["angle75"]).max()
    print("max |angle75 - restatement| =", err)
    assert err <= ANGLE_ATOL
    assert (got["angle75"][row] == -1.0).tolist() == (want["shared"] == 0).tolist()
    assert got["bundle_len"][row] == len(want["bundle"])
    assert got["bundle"][row].tolist() == want["bundle"] + [-1] * (width - len(want["bundle"]))


@pytest.mark.parametrize("name", list(NQ.walk_cases()))
def test_every_walk_path(name):
    scene, ref, num_images, expected = NQ.walk_cases()[name]
    want = NQ.local_bundle(*NQ.state_args(scene), ref, num_images, NQ.MIN_TRI_ANGLE_DEG)
    assert want["bundle"] == expected
    got = capi.local_bundles(*NQ.state_args(scene), [ref], num_images, NQ.MIN_TRI_ANGLE_DEG)
    _check_rows(got, 0, want, num_images - 1)
    assert got["info"]["num_syncs"] == 1 and got["info"]["num_groups"] == 1


ORDER_LENGTHS = [1, 2, 3, 4, 5, 255, 256, 257, SELECT_LDS - 1, SELECT_LDS, SELECT_LDS + 1, 5000, 300, 300, 7]
EQUAL, TWO_VALUES, ZERO_AT = 13, 14, 15  # image indices (lengths 300, 300, 7)


@pytest.fixture(scope="module")
def order_scene():
    scene = NQ.order_statistic_scene(ORDER_LENGTHS, seed=1, equal={EQUAL}, two_values={TWO_VALUES}, zero_at=ZERO_AT)
    want = {ref: NQ.local_bundle(*NQ.state_args(scene), ref, 4, NQ.MIN_TRI_ANGLE_DEG) for ref in (0, 12, 9)}
    for w in want.values():
        NQ.assert_margins(w, zero_allowed=True)
    return scene, want


def test_order_statistic_at_every_segment_length(order_scene):
    """Segments of 1 .. 5 (every residue of n - 1 mod 4, the .5 rounding among them), around a histogram's 256 bins, around the LDS
    buffer, 5000 from global memory; all values equal; two values with the rank inside the tie; a zero angle."""
    scene, want = order_scene
    w = want[0]
    assert w["shared"][1:].tolist() == ORDER_LENGTHS
    pts = scene["kp_point"][int(scene["kp_start"][TWO_VALUES]):int(scene["kp_start"][TWO_VALUES + 1])]
    assert sorted(set(pts.tolist())) == [0, 1] and len(set(scene["kp_point"][int(scene["kp_start"][EQUAL]):int(scene["kp_start"][EQUAL + 1])].tolist())) == 1
    got = capi.local_bundles(*NQ.state_args(scene), [0], 4, NQ.MIN_TRI_ANGLE_DEG)
    _check_rows(got, 0, w, 3)
    # the zero angle: the smallest of its image's 7, so not the selected one, but present in the list
    assert min(w["angles"]) == 0.0
    # a selected value is an element of the list: of the two values, bitwise one of the two
    two = {NQ.tri_angle(np.zeros(3), -scene["cam_t"][TWO_VALUES], scene["xyz"][p]) for p in (0, 1)}
    assert min(abs(got["angle75"][0][TWO_VALUES] - v) for v in two) <= ANGLE_ATOL
    again = capi.local_bundles(*NQ.state_args(scene), [0], 4, NQ.MIN_TRI_ANGLE_DEG)
    for k in ("bundle", "bundle_len", "shared", "angle75"):
        assert again[k].tobytes() == got[k].tobytes(), k


@pytest.mark.parametrize("refs", [[0], [0, 12, 9], [9, 9], [12, 0, 12]])
def test_rows_of_a_reference_do_not_depend_on_the_call(order_scene, refs):
    scene, want = order_scene
    got = capi.local_bundles(*NQ.state_args(scene), refs, 4, NQ.MIN_TRI_ANGLE_DEG)
    alone = {ref: capi.local_bundles(*NQ.state_args(scene), [ref], 4, NQ.MIN_TRI_ANGLE_DEG) for ref in set(refs)}
    for row, ref in enumerate(refs):
        _check_rows(got, row, want[ref], 3)
        for k in ("bundle", "bundle_len", "shared", "angle75"):
            assert got[k][row].tobytes() == alone[ref][k][0].tobytes(), (k, row)
    assert got["info"]["num_syncs"] == 1


def test_many_references_are_worked_off_in_groups_with_one_wait(order_scene):
    scene, want = order_scene
    refs = [0, 12, 9] * 334  # beyond one group's share of the workspace at this scene's 18 000 keypoints
    got = capi.local_bundles(*NQ.state_args(scene), refs, 4, NQ.MIN_TRI_ANGLE_DEG)
    print(got["info"])
    assert got["info"]["num_groups"] >= 2 and got["info"]["num_syncs"] == 1
    for row in (0, 1, 2, len(refs) - 3, len(refs) - 2, len(refs) - 1):
        _check_rows(got, row, want[refs[row]], 3)
    for k in ("bundle", "shared", "angle75"):
        rows = got[k].reshape(334, 3, -1)
        assert (rows == rows[:1]).all(), k  # every occurrence of a reference has the same row, whatever its group


# ---- a scene of the synthetic generator, through the Python classes -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mapped_scene():
    """12 images, 4000 points; images 3, 7 and 10 lose their observations and their pose: what a reconstruction looks like midway."""
    prob, _ = make_scene(12, 4000, True, seed=5)
    scene = scene_from_problem(prob, None, map_size=(33, 25), seed=5)
    cg = correspondences_from_problem(scene, prob, false_matches=40, seed=5)
    ids = sorted(scene.images)
    for imid in (ids[3], ids[7], ids[10]):
        for idx in list(scene.images[imid].get_observation_point2D_idxs()):
            if scene.images[imid].kp_point3D[idx] != INVALID_POINT3D:  # not gone with a short track meanwhile
                scene.obs.delete_observation(imid, int(idx))
        scene.images[imid].has_pose = False
    return scene, cg


def test_scene_queries_on_a_synthetic_scene(mapped_scene):
    scene, cg = mapped_scene
    q = SceneQueries(scene, cg)
    st, _ = state_arrays(scene, q.image_ids, q.kp_start)
    want = NQ.visibility(q.kp_start, q.kp_xy, q.corr_start, q.corr_kp, st["kp_point"], q.image_size)
    got = q.visibility()
    assert q.last_info["num_syncs"] == 1
    unregistered = [i for i, imid in enumerate(q.image_ids) if not scene.images[imid].has_pose]
    assert len(unregistered) == 3 and all(want["num_visible"][i] > 100 for i in unregistered)
    for i, imid in enumerate(q.image_ids):
        assert got[imid] == {"num_visible_points3D": int(want["num_visible"][i]), "point3D_visibility_score": int(want["score"][i]),
                             "num_observations": int((np.diff(q.corr_start)[q.kp_start[i]:q.kp_start[i + 1]] > 0).sum())}
    registered = [imid for imid in q.image_ids if scene.images[imid].has_pose]
    refs = [registered[0], registered[4], registered[0]]
    bundles = q.find_local_bundles(refs, 4)
    assert q.last_info["num_syncs"] == 1
    for ref, bundle in zip(refs, bundles):
        w = NQ.local_bundle(q.kp_start, st["registered"], st["cam_quat_xyzw"], st["cam_t"], st["kp_point"], st["xyz"], q.im_index[ref], 4,
                            NQ.MIN_TRI_ANGLE_DEG)
        NQ.assert_margins(w, min_angle=1e-3)  # a generated scene: a few points seen under 0.5 degrees; 1e-16 / sin(1e-3) = 1e-13 rad
        assert bundle == [q.image_ids[j] for j in w["bundle"]] and len(bundle) == 3
        assert not set(bundle) & {q.image_ids[i] for i in unregistered} and ref not in bundle
        assert q.find_local_bundle_ids(ref, 4) == bundle
    assert len(q.find_local_bundle_ids(refs[0])) == 5  # COLMAP's local_ba_num_images = 6
    with pytest.raises(capi.MpsfmHipError):
        q.find_local_bundle_ids(q.image_ids[unregistered[0]])


@pytest.mark.parametrize("method", VISIBILITY_METHODS)
def test_image_selection_end_to_end(mapped_scene, method):
    scene, cg = mapped_scene
    sel = ImageSelection({"image_selection_method": method}, scene, SimpleNamespace(cg=cg))
    q = SceneQueries(scene, cg)
    st, _ = state_arrays(scene, q.image_ids, q.kp_start)
    want = NQ.visibility(q.kp_start, q.kp_xy, q.corr_start, q.corr_kp, st["kp_point"], q.image_size)
    candidates = [imid for imid in scene.images if not scene.images[imid].has_pose]
    idx = [q.im_index[i] for i in candidates]
    score = {"MAX_VISIBLE_POINTS_NUM": want["num_visible"][idx].astype(float), "MIN_UNCERTAINTY": want["score"][idx].astype(float),
             "MAX_VISIBLE_POINTS_RATIO": want["num_visible"][idx] / q.num_observations[idx]}[method]
    assert len(set(score.tolist())) == len(score)  # distinct: the choice is determined
    assert sel.next_image() is True
    assert sel.candid == candidates[int(np.argsort(score)[-1])] and scene.best_next_ref_imid is None
    sel.at_failure(sel.candid)
    assert sel.next_image() is True and sel.candid == candidates[int(np.argsort(score)[-2])]
