"""mpsfm_corr_graph_build and HipCorrespondenceGraph on the GPU against the restatement (tests/numpy_correspondence_graph.py), and the
chain from in-memory matches to the track engine.  Every output is integers: equal exactly, no tolerance."""

from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import numpy_correspondence_graph as NG
from mpsfm_amd import capi
from mpsfm_amd.sfm.scene.correspondence_graph import HipCorrespondenceGraph

pytestmark = pytest.mark.gpu


def random_case(rng, n_images, n_kp, n_matches, n_lists, dup=0.1):
    """images of random sizes that sum to n_kp, lists between random (ordered) pairs, a share of repeated and of bad rows"""
    cuts = np.sort(rng.integers(0, n_kp + 1, n_images - 1))
    kp_start = np.concatenate([[0], cuts, [n_kp]]).astype(np.int64)
    nkp = np.diff(kp_start)
    li0 = rng.integers(0, n_images, n_lists).astype(np.int32)
    li1 = rng.integers(0, n_images, n_lists).astype(np.int32)
    lstart = np.concatenate([[0], np.sort(rng.integers(0, n_matches + 1, n_lists - 1)), [n_matches]]).astype(np.int64)
    l_of = np.searchsorted(lstart, np.arange(n_matches), side="right") - 1
    m = np.stack([rng.integers(-1, np.maximum(nkp[li0[l_of]], 1) + 1), rng.integers(-1, np.maximum(nkp[li1[l_of]], 1) + 1)], 1).astype(np.int32)
    rep = np.flatnonzero(rng.uniform(size=n_matches) < dup)
    src = rng.integers(0, n_matches, len(rep))
    same = (li0[l_of[rep]] == li0[l_of[src]]) & (li1[l_of[rep]] == li1[l_of[src]])
    flip = (li0[l_of[rep]] == li1[l_of[src]]) & (li1[l_of[rep]] == li0[l_of[src]])
    m[rep[same]] = m[src[same]]
    m[rep[flip & ~same]] = m[src[flip & ~same]][:, ::-1]
    return kp_start, li0, li1, lstart, m


def test_every_status_and_every_output_on_five_small_images():
    kp_start = np.array([0, 0, 1, 4, 68, 133], np.int64)  # 0, 1, 3, 64 and 65 keypoints
    groups = [
        (3, 4, [[0, 0], [1, 1], [1, 1], [2, 5], [2, 6], [63, 64], [64, 0], [-1, 3], [5, 65], [5, -7]]),  # a copy inside the list, two partners
        (4, 3, [[0, 0], [1, 1], [7, 7], [64, 63], [65, 0]]),      # copies in the other orientation
        (3, 4, [[7, 7], [10, 11], [63, 64]]),                     # copies across lists
        (2, 2, [[0, 1], [1, 1]]),                                 # a self pair
        (1, 2, [[0, 0], [0, 2], [1, 0]]),
        (2, 3, [[0, 0]]),
        (0, 1, [[0, 0]]),                                         # image 0 has no keypoint
        (4, 3, []),
        (1, 4, [[0, 64], [0, 64]]),
    ]
    args = NG.lists_of(groups)
    want = NG.build(kp_start, *args)
    assert want["match_status"].tolist() == [0, 0, 3, 0, 0, 0, 1, 1, 1, 1, 3, 3, 0, 3, 1, 3, 0, 3, 2, 2, 0, 0, 1, 0, 1, 0, 3]
    got = capi.corr_graph_build(kp_start, *args)
    NG.assert_equal(got, want)
    assert got["info"]["num_syncs"] == 1
    assert [got["info"][k] for k in ("num_added", "num_invalid", "num_self_pairs", "num_duplicates")] == [11, 7, 2, 7]
    assert len(got["corr_kp"]) == 22 and got["pair_image0"].tolist() == [1, 1, 2, 3] and got["pair_image1"].tolist() == [2, 4, 3, 4]
    assert got["kp_two_view"][4 + 7] == 1 and got["kp_two_view"][4 + 2] == 0  # (3, 7) - (4, 7) alone; (3, 2) has two partners in image 4


def ladder():
    """130 images: keypoint 0 of image 0 is matched in every other image (degree 129), keypoints 1, 2, 3 of image 0 in 63, 64 and 65
    images, every other row has one or two entries"""
    n = 130
    degs = ((1, 63), (2, 64), (3, 65))
    nkp = [4] + [2 + sum(j <= d for _, d in degs) for j in range(1, n)]  # image j: the partners of image 0's keypoints, then the chain's
    kp_start = np.concatenate([[0], np.cumsum(nkp)]).astype(np.int64)
    groups = []
    for j in range(1, n):
        rows = [0] + [r for r, d in degs if j <= d]
        groups.append((0, j, [[r, i] for i, r in enumerate(rows)]))
        if j + 1 < n:
            groups.append((j, j + 1, [[nkp[j] - 1, nkp[j + 1] - 1]]))  # a chain through the last keypoint of every image
    groups.append((0, 7, [[0, 0], [3, 3]]))  # two copies: which position is the duplicate depends on the order of the lists
    return kp_start, groups


def test_row_lengths_from_1_to_129_and_three_orders_of_the_lists():
    # The build is a global sort of the directed entries and has no threshold between a short-row and a long-row path; the sizes a
    # threshold could sit at here are the wavefront's: rows of 63, 64 and 65 entries next to one of 129 and many of 1 and 2.
    kp_start, groups = ladder()
    rng = np.random.default_rng(3)
    orders = [groups, groups[::-1], [(b, a, np.asarray(m)[:, ::-1]) if k % 2 else (a, b, m) for k, (a, b, m) in
                                     enumerate(groups[i] for i in rng.permutation(len(groups)))]]
    want = NG.build(kp_start, *NG.lists_of(groups))
    deg = np.diff(want["corr_start"])
    assert deg[:4].tolist() == [129, 63, 64, 65] and set(deg[4:].tolist()) == {1, 2}
    statuses = []
    for order in orders:
        args = NG.lists_of(order)
        got = capi.corr_graph_build(kp_start, *args)
        NG.assert_equal(got, want, skip=("match_status",))
        assert np.array_equal(got["match_status"], NG.build(kp_start, *args)["match_status"])
        statuses.append(np.flatnonzero(got["match_status"]).tolist())
    assert len({tuple(s) for s in statuses}) > 1 and all(len(s) == 2 for s in statuses)


@pytest.mark.parametrize("n_kp", [1023, 1024, 1025, 4097])
def test_sizes_on_both_sides_of_a_block_of_the_scan_and_of_the_fill(n_kp):
    rng = np.random.default_rng(n_kp)
    case = random_case(rng, 7, n_kp, 2 * n_kp + 1, 30)
    want = NG.build(*case)
    assert len(set(want["match_status"].tolist())) == 4
    NG.assert_equal(capi.corr_graph_build(*case), want)


def test_60000_matches_twice_and_four_graphs_from_four_threads():
    rng = np.random.default_rng(11)
    big = random_case(rng, 40, 50000, 60000, 300, dup=0.2)
    want = NG.build(*big)
    one, two = capi.corr_graph_build(*big), capi.corr_graph_build(*big)
    NG.assert_equal(one, want)
    for name in NG.OUTPUTS:
        assert one[name].tobytes() == two[name].tobytes(), name
    cases = [random_case(np.random.default_rng(100 + t), 12 + t, 3000 + 700 * t, 9000 + 1000 * t, 40 + t) for t in range(4)]
    wants = [NG.build(*c) for c in cases]
    with ThreadPoolExecutor(4) as pool:
        for _ in range(3):
            gots = list(pool.map(lambda c: capi.corr_graph_build(*c), cases))
            for got, w in zip(gots, wants):
                NG.assert_equal(got, w)


# ---- the class on a scene, and the chain to the track engine -------------------------------------------------------------------------
def hip_graph_like(cg):
    """a HipCorrespondenceGraph filled with what a NumpyCorrespondenceGraph holds"""
    g = HipCorrespondenceGraph()
    for imid, n in cg.num_kp.items():
        g.add_image(imid, n)
    for (a, b), m in cg.matches.items():
        g.add_correspondences(a, b, m)
    return g


def test_csr_equals_graph_arrays_and_the_engine_logs_the_same_operations():
    from numpy_scene import correspondences_from_problem, scene_from_problem
    from mpsfm_amd.sfm.mapper.track_engine import HipIncrementalTriangulator, graph_arrays
    from mpsfm_amd.synthetic import make_scene

    logs = []
    arrays = []
    for kind in ("numpy", "hip"):
        prob, truth = make_scene(10, 1500, seed=71)
        scene = scene_from_problem(prob, truth, with_points=False)
        cg = correspondences_from_problem(scene, prob, false_matches=300, seed=71)
        if kind == "hip":
            cg = hip_graph_like(cg)
            cg.finalize()
            assert cg.rejected() == {"invalid": 0, "self_pair": 0, "duplicate": 0}
        ga = graph_arrays(cg, scene)
        arrays.append(ga)
        tri = HipIncrementalTriangulator(cg, scene)
        ops = []
        for imid in sorted(scene.images):
            tri.triangulate_image({}, imid)
            ops.append({k: v.copy() for k, v in tri.last_ops.items()})
        tri.close()
        logs.append(ops)
    for name in ("kp_start", "corr_start", "corr_kp", "kp_xy", "intr", "kp_image"):
        assert arrays[0][name].dtype == arrays[1][name].dtype and np.array_equal(arrays[0][name], arrays[1][name]), name
    assert len(arrays[0]["corr_kp"]) > 20000
    for a, b in zip(*logs):
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
    assert sum(len(o["type"]) for o in logs[0]) > 1000


def test_the_chain_from_a_store_to_the_track_engine(capsys):
    from numpy_scene import INVALID_POINT3D, correspondences_from_problem, scene_from_problem
    from mpsfm_amd.sfm.estimators.two_view_geometry import _pose_matrix
    from mpsfm_amd.sfm.mapper.triangulator import MpsfmTriangulator
    from mpsfm_amd.sfm.scene.correspondences import CorrespondenceStore, Correspondences
    from mpsfm_amd.synthetic import make_scene

    prob, truth = make_scene(6, 600, True, seed=81, perturb=False, outlier_frac=0.02)
    sc = scene_from_problem(prob, truth, seed=81, with_points=False)
    raw = correspondences_from_problem(sc, prob, false_matches=60, seed=81)  # the matches before verification
    name = {imid: f"im{imid}.jpg" for imid in sc.images}
    for imid, im in sc.images.items():
        im.name, im.has_pose = name[imid], False
    sc.cameras, sc.imid = sc.rec.cameras, {n: i for i, n in name.items()}.__getitem__

    def set_keypoints(image_id, xy):  # the scene contract of Correspondences: the stand-in keeps an image's keypoints in `kps`
        assert len(xy) == len(sc.images[image_id].kps)
        sc.images[image_id].kps = np.asarray(xy, np.float64).reshape(-1, 2)

    sc.set_keypoints = set_keypoints
    exact = {imid: im.kps.copy() for imid, im in sc.images.items()}
    rng = np.random.default_rng(81)
    store = CorrespondenceStore([(name[a], name[b]) for a, b in raw.matches], matcher_type="sparse")
    for imid, im in sc.images.items():
        store.set_sparse_keypoints(name[imid], (im.kps - 0.5).astype(np.float32))  # hloc's origin: gathering adds the half pixel
    for (a, b), m in raw.matches.items():
        store.set_sparse_matches(name[a], name[b], m, rng.uniform(0.1, 1, len(m)).astype(np.float16))
    c = Correspondences({"matches_mode": "sparse"}, sc, store)
    assert c.populate() is True
    assert "has no correspondences" not in capsys.readouterr().out
    # the scene's keypoints: the gathered float32 coordinates rounded to float16
    for imid, im in sc.images.items():
        assert np.array_equal(im.kps, c.keypoints_set[name[imid]].astype(np.float16).astype(np.float64))
        assert np.abs(im.kps - exact[imid]).max() <= 0.5 + 1e-3  # float16 resolves 1 pixel between 1024 and 2048
    # verification: inliers are rows of the pair's matches; both orientations of the geometry
    groups, n_in, n_all = [], 0, 0
    for (a, b), m in raw.matches.items():
        tvg, ok = c.two_view_geom(name[a], name[b])
        assert ok and tvg is c._two_view_geom[name[a], name[b]]
        rows = {tuple(r) for r in m.tolist()}
        assert all(tuple(r) in rows for r in tvg.inlier_matches.tolist())
        inv, ok = c.two_view_geom(name[b], name[a])
        assert ok and np.array_equal(inv.E, tvg.E.T) and np.array_equal(inv.F, tvg.F.T) and np.array_equal(inv.inlier_matches, tvg.inlier_matches[:, ::-1])
        assert np.allclose(_pose_matrix(inv.cam2_from_cam1)[:, :3], _pose_matrix(tvg.cam2_from_cam1)[:, :3].T, atol=1e-12)
        mask = np.array([tuple(r) in {tuple(q) for q in tvg.inlier_matches.tolist()} for r in m.tolist()], bool)
        scores = store.get_matches("sparse", name[a], name[b])[1]
        want = sum(scores[mask]) if len(tvg.inlier_matches) else 0  # the reference's expression
        got = c.inlier_match_scores[frozenset((name[a], name[b]))]
        assert got == want and type(got) is type(want)
        groups.append((a, b, tvg.inlier_matches))
        n_in, n_all = n_in + len(tvg.inlier_matches), n_all + len(m)
    assert c.two_view_geom("im1.jpg", "nowhere.jpg") == (None, False)
    print("inlier matches", n_in, "of", n_all)
    # the graph holds the inlier matches of every pair: the restatement over the same lists
    ids = sorted(sc.images)
    kp_start = np.concatenate([[0], np.cumsum([len(sc.images[i].kps) for i in ids])]).astype(np.int64)
    want = NG.build(kp_start, *NG.lists_of([(ids.index(a), ids.index(b), m) for a, b, m in groups]))
    csr = c.cg.csr()
    assert np.array_equal(csr["corr_start"], want["corr_start"]) and np.array_equal(csr["corr_kp"], want["corr_kp"]) and len(want["corr_kp"]) == 2 * n_in
    loop = [(i, j) for i in sc.images for j in sc.images if i < j and c.num_correspondences_between_images(i, j) > 0]  # the reference's loop
    assert c.image_pairs() == loop and len(loop) > 0
    assert np.array_equal(c.matches(*loop[0]), c.cg.find_correspondences_between_images(*loop[0]))
    # the track engine on correspondences.cg, as tests/test_gpu_triangulator.py::test_incremental_triangulation_recovers_the_scene
    tri = MpsfmTriangulator({"colmap_options": {"min_angle": 0.001, "ignore_two_view_tracks": False}, "lift_low_parallax": False}, sc, c.cg)
    tri._require_engine()
    n = 0
    for imid in ids:
        sc.images[imid].has_pose = True
        n += tri._triangulator.triangulate_image(tri.options, imid)
    assert n == sum(p.track.length() for p in sc.points3D.values())
    seen = set()
    for pid, p in sc.points3D.items():
        assert p.track.length() >= 2
        for e in p.track.elements:
            assert (e.image_id, e.point2D_idx) not in seen and sc.images[e.image_id].kp_point3D[e.point2D_idx] == pid
            seen.add((e.image_id, e.point2D_idx))
    assert sum(int((im.kp_point3D != INVALID_POINT3D).sum()) for im in sc.images.values()) == len(seen)
    first_obs = {(int(i), int(k)): o for o, (i, k) in enumerate(zip(sc._obs_image, sc._obs_point2D))}
    err = np.array([np.linalg.norm(p.xyz - truth["pts"][prob.obs_pt[first_obs[(p.track.elements[0].image_id, p.track.elements[0].point2D_idx)]]])
                    for p in sc.points3D.values()])
    print("triangulated", len(sc.points3D), "of", prob.n_pts, "points; median error", np.median(err), "share below 0.5:", np.mean(err < 0.5))
    # Every landmark is seen at least twice.  Against the full graph of the test this follows (bound 0.85), verification drops the
    # matches of pairs it finds no geometry for (fewer than 15 inliers) and of the 2 % corrupted observations, and the keypoints
    # are rounded to float16 (half a pixel at most, 4e-4 rad at a focal length above 1000 pixels): a tenth more may go.
    assert len(sc.points3D) > 0.75 * prob.n_pts
    assert np.median(err) < 0.05 and np.mean(err < 0.5) > 0.97


def test_the_methods_of_the_class_against_the_restatement():
    rng = np.random.default_rng(5)
    kp_start, li0, li1, lstart, m = random_case(rng, 6, 400, 900, 25)
    ids = [3, 8, 9, 20, 21, 40]  # image ids are not indices
    want = NG.build(kp_start, li0, li1, lstart, m)
    g = HipCorrespondenceGraph()
    for i, imid in enumerate(ids):
        g.add_image(imid, int(kp_start[i + 1] - kp_start[i]))
    for l in range(len(li0)):
        g.add_correspondences(ids[li0[l]], ids[li1[l]], m[lstart[l]:lstart[l + 1]].astype(np.uint32) if l % 2 else m[lstart[l]:lstart[l + 1]])
    assert g.num_correspondences_for_image(ids[0]) == want["image_num_correspondences"][0]  # a query before finalize builds
    g.finalize()
    with pytest.raises(RuntimeError):
        g.add_image(99, 3)
    with pytest.raises(RuntimeError):
        g.add_correspondences(3, 8, [[0, 0]])
    assert np.array_equal(np.concatenate(g.match_status()), want["match_status"])
    n = np.bincount(want["match_status"], minlength=4)
    assert g.rejected() == {"invalid": n[1], "self_pair": n[2], "duplicate": n[3]}
    assert g.num_image_pairs() == len(want["pair_image0"]) and g.num_images() == int((want["image_num_correspondences"] > 0).sum())
    assert g.image_pairs() == [(ids[a], ids[b]) for a, b in zip(want["pair_image0"], want["pair_image1"])]
    all_pairs = g.num_correspondences_between_all_images()
    for p, (a, b) in enumerate(zip(want["pair_image0"], want["pair_image1"])):
        rows = want["pair_matches"][want["pair_start"][p]:want["pair_start"][p + 1]]
        assert np.array_equal(g.find_correspondences_between_images(ids[a], ids[b]), rows)
        assert np.array_equal(g.find_correspondences_between_images(ids[b], ids[a]), rows[:, ::-1])
        assert g.num_correspondences_between_images(ids[b], ids[a]) == len(rows) == all_pairs[2147483647 * ids[a] + ids[b]]
    assert len(all_pairs) == len(want["pair_image0"])
    assert g.num_correspondences_between_images(3, 77) == 0 and len(g.find_correspondences_between_images(77, 3)) == 0
    for i, imid in enumerate(ids):
        if want["image_num_correspondences"][i] == 0:
            assert not g.exists_image(imid)
            continue
        assert g.exists_image(imid)
        assert g.num_correspondences_for_image(imid) == want["image_num_correspondences"][i]
        assert g.num_observations_for_image(imid) == want["image_num_observations"][i]
        for idx in range(int(kp_start[i + 1] - kp_start[i])):
            k = kp_start[i] + idx
            row = want["corr_kp"][want["corr_start"][k]:want["corr_start"][k + 1]]
            assert g.has_correspondences(imid, idx) == (len(row) > 0)
            assert g.is_two_view_observation(imid, idx) == bool(want["kp_two_view"][k])
            im = np.searchsorted(kp_start, row, side="right") - 1
            assert g.extract_correspondences(imid, idx) == [(ids[a], int(r - kp_start[a])) for a, r in zip(im, row)]
    assert not g.exists_image(77)
    csr = g.csr()
    assert csr["image_ids"] == ids and np.array_equal(csr["corr_start"], want["corr_start"]) and np.array_equal(csr["corr_kp"], want["corr_kp"])


def test_cached_blocks_and_pool_streams_come_back():
    cases = [random_case(np.random.default_rng(s), 5 + s, 300 * (s + 1), 500 * (s + 1) + 1, 9 + s) for s in range(3)]

    def body():
        for c in cases:
            capi.corr_graph_build(*c)
        capi.corr_graph_build(np.zeros(3, np.int64), *NG.lists_of([(0, 1, [[0, 0]])]))  # no device needed
        with pytest.raises(capi.MpsfmHipError):
            capi.corr_graph_build(np.array([0, 5, 3], np.int64), *NG.lists_of([(0, 1, [[0, 0]])]))

    body()
    before = capi.debug_resources()
    body()
    after = capi.debug_resources()
    print("blocks, bytes, streams, events, pinned:", before, "->", after)
    assert after == before
