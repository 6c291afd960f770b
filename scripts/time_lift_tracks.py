"""Wall time of MpsfmTriangulator.lift_low_parallax over all points of the NumPy scene (40 cameras / 30 k landmarks) with
lift="loop" and lift="batch", and the device-time split of mpsfm_lift_tracks: a call with threshold 0 ends after the angle
launch, so its info.ms is the angle launch alone and the difference to a full call is the lift launch."""
import copy, json, sys, time
sys.path.insert(0, '.')
sys.path.insert(0, 'tests')
import numpy as np
from mpsfm_amd import capi
from mpsfm_amd.synthetic import make_scene
from mpsfm_amd.sfm.mapper.triangulator import MpsfmTriangulator, track_quality, tracks_from_scene
from numpy_scene import scene_from_problem

prob, truth = make_scene(40, 30000, True, seed=5)
sc = scene_from_problem(prob, truth, seed=1)
ids = sorted(sc.points3D)
ang = track_quality(sc, ids)[0]
out = {"points": len(ids), "elements": int(sum(len(p.track.elements) for p in sc.points3D.values()))}
for name, thr in (("retri_min_angle", 1.5), ("median_angle", float(np.rad2deg(np.median(ang))))):
    row = {"threshold_deg": thr, "risky": int((ang < np.deg2rad(thr)).sum())}
    for mode in ("loop", "batch"):
        ts = []
        for _ in range(3):
            s = copy.deepcopy(sc)
            tri = MpsfmTriangulator({"colmap_options": {}}, s, None, lift=mode)
            t0 = time.perf_counter(); new = tri.lift_low_parallax(ids, thr); ts.append(1e3 * (time.perf_counter() - t0))
        row[mode + "_wall_ms"] = [round(t, 1) for t in ts]
        row[mode + "_new_points"] = len(new)
        if mode == "batch":
            row["info"] = tri.last_lift_info
    out[name] = row
    # the call alone, without gathering the tracks from the scene and without applying the result
    tr, imids = tracks_from_scene(sc, ids)
    im = [sc.images[i] for i in imids]
    args = ([True] * len(im), [i.depth.data for i in im], [i.depth.valid for i in im], [sc.rec.cameras[i.camera_id].sx for i in im],
            [sc.rec.cameras[i.camera_id].sy for i in im])
    xyz = sc.point3D_coordinates(ids)
    for label, t in (("angle_only", 0.0), ("full", thr)):
        ms, wall = [], []
        for _ in range(5):
            t0 = time.perf_counter(); r = capi.lift_tracks(tr, xyz, *args, t); wall.append(1e3 * (time.perf_counter() - t0)); ms.append(r["info"]["ms"])
        row[label + "_device_ms"] = round(float(np.median(ms)), 4)
        row[label + "_call_wall_ms"] = round(float(np.median(wall)), 2)
print(json.dumps(out))
