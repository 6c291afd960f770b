"""Wall time of one global filter_bundle through BundleFilter (one mpsfm_filter_scene call) and through the sequence it replaces
(tests/mapper_replay.py over HipObservationManager: five walks over the tracks, five mpsfm_filter_tracks launches), on the NumPy
scene at two shapes: make_scene(40, 30000) of DESIGN.md section 4u and a C3-shaped scene (200 images, 150 k points), both at the
unperturbed state (at the perturbed start every observation is beyond 4 px and a filter deletes the scene).  Then the
call alone, its device time split into track lists and k_scene_filter, and the angle launch of mpsfm_filter_tracks on the same
tracks (a mpsfm_lift_tracks call with threshold 0 ends after that launch, so its info.ms is the launch alone).

"fresh": every run on its own deep copy of the scene as built (outliers and all: the filter deletes).  "steady": the scene after one
filter, on which a further filter finds nothing, so the runs need no copies and both paths do the same (empty) bookkeeping.
Median of 5 after 2 warm-ups throughout (the deep copies are outside the timed region)."""
import copy, json, sys, time
sys.path.insert(0, '.')
sys.path.insert(0, 'tests')
import numpy as np
from mpsfm_amd import capi
from mpsfm_amd.synthetic import make_scene
from mpsfm_amd.sfm.mapper.filtering import BundleFilter
from mpsfm_amd.sfm.mapper.triangulator import tracks_from_scene
from mpsfm_amd.sfm.scene.scene_queries import SceneQueries
from mapper_replay import MapperReplay
from numpy_scene import NumpyCorrespondenceGraph, scene_from_problem


def drop_in(sc):
    cg = NumpyCorrespondenceGraph()
    for imid, im in sc.images.items():
        cg.add_image(imid, len(im.kps))
    return BundleFilter({}, sc, SceneQueries(sc, cg))


def timed(fn, runs, warm):
    ts = []
    for i in range(warm + runs):
        t0 = time.perf_counter(); r = fn(); t = 1e3 * (time.perf_counter() - t0)
        if i >= warm:
            ts.append(t)
    return round(float(np.median(ts)), 2), r


def once(sc, new):
    s = copy.deepcopy(sc)
    f = drop_in(s) if new else MapperReplay(s, None)
    t0 = time.perf_counter(); r = f.filter_bundle(f.find_global_bundle()); t = 1e3 * (time.perf_counter() - t0)
    return t, r, s


out = {}
for name, (n_cams, n_pts), fresh_runs in (("40x30000", (40, 30000), (5, 2)), ("200x150000", (200, 150000), (5, 2))):
    prob, truth = make_scene(n_cams, n_pts, True, seed=5, perturb=False)  # as after a bundle adjustment: 5 % outlier observations to find
    sc = scene_from_problem(prob, truth, seed=1)
    row = {"points": len(sc.points3D), "elements": int(sum(len(p.track.elements) for p in sc.points3D.values()))}
    for label, new in (("bundle_filter", True), ("parent_path", False)):
        ts, r = [], None
        for i in range(sum(fresh_runs)):
            t, r, _ = once(sc, new)
            if i >= fresh_runs[1]:
                ts.append(t)
        row[label + "_fresh_ms"] = round(float(np.median(ts)), 2)
        row[label + "_fresh_returned"] = [int(r[0]), sorted(r[1])]
    _, _, steady = once(sc, True)
    bf, replay = drop_in(steady), MapperReplay(steady, None)
    bundle = bf.find_global_bundle()
    row["bundle_filter_steady_ms"], r_new = timed(lambda: bf.filter_bundle(bundle), 5, 2)
    row["info"] = bf.last_info
    row["parent_path_steady_ms"], r_old = timed(lambda: replay.filter_bundle(bundle), 5, 2)
    row["steady_returned"] = [int(r_new[0]), int(r_old[0])]
    # the call alone, on the arrays of the steady scene
    st, point_ids = bf._state()
    in_bundle, flags = bf._invalid_depth_flags(bundle["optim_ids"], st)
    call = lambda: capi.filter_scene(bf.sq.kp_start, bf.sq.kp_xy, bf.sq.intr, st["registered"], st["cam_quat_xyzw"], st["cam_t"], st["kp_point"], st["xyz"],
                                     float(bf._max_err()), 0.001, 1.5, in_bundle=in_bundle, kp_invalid_depth=flags, point_sel=np.ones(len(point_ids), np.uint8))
    row["call_wall_ms"], r = timed(call, 5, 2)
    infos = [call()["info"] for _ in range(5)]
    row["device_ms"] = round(float(np.median([i["ms"] for i in infos])), 4)
    row["device_tracks_ms"] = round(float(np.median([i["ms_tracks"] for i in infos])), 4)
    row["device_kernel_ms"] = round(float(np.median([i["ms"] - i["ms_tracks"] for i in infos])), 4)
    t0 = time.perf_counter(); _ = [bf._state() for _ in range(3)]; row["state_arrays_ms"] = round(1e3 * (time.perf_counter() - t0) / 3, 2)
    t0 = time.perf_counter(); bf._invalid_depth_flags(bundle["optim_ids"], st); row["depth_flags_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
    # the angle launch of mpsfm_filter_tracks on the same tracks
    ids = sorted(steady.points3D)
    t0 = time.perf_counter(); tr, imids = tracks_from_scene(steady, ids); row["one_walk_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
    im = [steady.images[i] for i in imids]
    args = ([True] * len(im), [i.depth.data for i in im], [i.depth.valid for i in im], [steady.rec.cameras[i.camera_id].sx for i in im],
            [steady.rec.cameras[i.camera_id].sy for i in im])
    xyz = steady.point3D_coordinates(ids)
    row["filter_tracks_angle_launch_ms"] = round(float(np.median([capi.lift_tracks(tr, xyz, *args, 0.0)["info"]["ms"] for _ in range(5)])), 4)
    out[name] = row
    print(json.dumps({name: row}), flush=True)
print(json.dumps(out))
