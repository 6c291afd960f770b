"""The filter behind a bundle adjustment, and the bundles it works on, over libmpsfm_hip.

``BundleFilter(conf, mpsfm_rec, scene_queries)`` carries the methods of the reference's ``MpsfmMapper`` that filter a scene and find
its bundles (mpsfm/sfm/mapper/base.py:686-826), with their names, arguments and return shapes:

    filter_all()  filter_bundle(bundle, filter_ims=True)  filter_images()
    filter_local_points3D(local_bundle, max_err, min_angle)  filter_all_points3D(max_err, min_angle)
    find_invalid_depth_points(imids)
    find_local_bundle(refimid, num_images=None, return_points=True)  find_global_bundle()  find_subset_bundle(bundle)

The reference runs a ``filter_bundle`` as five filters of ``ObservationManager``, one after the other.  Every decision of that sequence
about a point depends on the point's own track only, so here it is ONE ``mpsfm_filter_scene`` call on the flat arrays a
``SceneQueries`` keeps (keypoints, intrinsics) and ``state_arrays`` gathers per call (poses, keypoint -> point): no walk over the
elements of the tracks.  The answer is applied through the scene's own manager, ``obs.delete_point3D`` for every point that died and
``obs.delete_observation`` for the marked keypoints of the points that live on, so the scene object keeps its bookkeeping.
"""

from __future__ import annotations

import numpy as np

from .track_engine import state_arrays

RISKY_MIN_TRI_ANGLE = 1.5  # degrees: COLMAP's default, which the reference passes for the risky set (mapper/base.py:786-790)
_DEFAULTS = dict(filter_max_reproj_error=4.0, filter_min_tri_angle=0.001, min_focal_length_ratio=0.1, max_focal_length_ratio=10.0,
                 max_extra_param=1.0)  # COLMAP's, with the mapper's filter_min_tri_angle (mapper/base.py:35-40)


class BundleFilter:
    def __init__(self, conf, mpsfm_rec, scene_queries, backend=None):
        """`conf`: the mapper's conf (its `colmap_options` are read) or the options themselves, as a mapping or an object; fields that
        are missing take COLMAP's defaults.  `scene_queries`: the SceneQueries of the scene; its keypoint arrays are reused.
        `backend`: a callable with capi.filter_scene's signature and return value, used instead of the library (tests without a GPU)."""
        self.conf, self.rec, self.sq, self.backend = conf, mpsfm_rec, scene_queries, backend
        self.device = getattr(scene_queries, "device", 0)
        self.last_info = None
        self.last_result = None

    # -- options ---------------------------------------------------------------------------------------------------------------------
    def _option(self, name):
        conf = self.conf
        options = conf.get("colmap_options") if hasattr(conf, "get") else getattr(conf, "colmap_options", None)
        for src in (options, conf):
            if src is None:
                continue
            v = src.get(name) if hasattr(src, "get") else getattr(src, name, None)
            if v is not None:
                return v
        return _DEFAULTS[name]

    def _max_err(self):
        return self._option("filter_max_reproj_error") * np.median([image.kp_std for image in self.rec.images.values()])

    # -- the call ----------------------------------------------------------------------------------------------------------------------
    def _state(self):
        sq = self.sq
        st, point_ids = state_arrays(self.rec, sq.image_ids, sq.kp_start)
        stray = (st["kp_point"] >= 0) & (st["registered"][sq.kp_image] == 0)
        if stray.any():
            imid = sq.image_ids[int(sq.kp_image[int(np.flatnonzero(stray)[0])])]
            raise ValueError(f"image {imid} is not registered but its keypoints have 3-D points")
        return st, point_ids

    def _invalid_depth_flags(self, imids, st):
        """in_bundle [n_images] and kp_invalid_depth [n_kp]: the keypoints with a point of the given images whose prior depth is not valid."""
        sq = self.sq
        in_bundle, flags = np.zeros(len(sq.image_ids), np.uint8), np.zeros(len(st["kp_point"]), np.uint8)
        for imid in imids:
            i = sq.im_index[imid]
            in_bundle[i] = 1
            image = self.rec.images[imid]
            idx = np.flatnonzero(st["kp_point"][sq.kp_start[i]:sq.kp_start[i + 1]] >= 0)
            if len(idx):
                valid = np.asarray(image.depth.valid_at_kps(image.keypoint_coordinates(idx)), bool)
                flags[sq.kp_start[i] + idx[~valid]] = 1
        return in_bundle, flags

    def _filter(self, bundle, points, max_err, min_angle, negative_depth):
        """One mpsfm_filter_scene call and its application.  `bundle`: the image ids of the risky set or None; `points`: the point ids
        of the second pass or None for all."""
        sq = self.sq
        st, point_ids = self._state()
        in_bundle = flags = sel = None
        if bundle is not None:
            in_bundle, flags = self._invalid_depth_flags(bundle, st)
        if points is not None:
            sel = np.isin(point_ids, np.fromiter((int(p) for p in points), np.int64, len(points))).astype(np.uint8)
        call = self.backend
        if call is None:
            from ... import capi

            call = capi.filter_scene
        out = call(sq.kp_start, sq.kp_xy, sq.intr, st["registered"], st["cam_quat_xyzw"], st["cam_t"], st["kp_point"], st["xyz"], float(max_err),
                   float(min_angle), RISKY_MIN_TRI_ANGLE, in_bundle=in_bundle, kp_invalid_depth=flags, point_sel=sel,
                   negative_depth=negative_depth, device=self.device)
        self.last_info, self.last_result = out["info"], out
        self._apply(out, st, point_ids, in_bundle is not None, sel)
        return out["info"]

    def _apply(self, out, st, point_ids, with_bundle, sel):
        sq, rec, obs = self.sq, self.rec, self.rec.obs
        fate, deleted, kp_point = out["point_fate"], out["kp_deleted"], st["kp_point"]
        for pid in point_ids[fate >= 2].tolist():
            obs.delete_point3D(pid)
        kps = np.flatnonzero(deleted != 0)
        kps = kps[fate[kp_point[kps]] < 2]
        images = sq.kp_image[kps]
        for imid, idx in zip(np.asarray(sq.image_ids)[images].tolist(), (kps - sq.kp_start[images]).tolist()):
            obs.delete_observation(imid, idx)
        # Point3D.error of the points a pass looked at and left standing: the mean error of what is left of their tracks
        passed = fate < 2
        if sel is not None:
            passed &= (sel != 0) | ((out["point_risky"] != 0) if with_bundle else False)
        if out["kp_sq_err"] is None or not passed.any() or not hasattr(rec.points3D[int(point_ids[np.flatnonzero(passed)[0]])], "error"):
            return
        left = (kp_point >= 0) & (deleted == 0)
        total = np.bincount(kp_point[left], weights=np.sqrt(out["kp_sq_err"][left]), minlength=len(point_ids))
        count = np.bincount(kp_point[left], minlength=len(point_ids))
        points3D = rec.points3D
        for pid, err in zip(point_ids[passed].tolist(), (total[passed] / np.maximum(count[passed], 1)).tolist()):
            points3D[pid].error = err

    # -- the reference's filters -----------------------------------------------------------------------------------------------------
    def filter_all(self):
        """Filters all points and images"""
        info = self._filter(None, None, self._max_err(), self._option("filter_min_tri_angle"), True)
        return info["num_changed_b"], self.filter_images()

    def filter_bundle(self, bundle, filter_ims=True):
        """Filters 3D points and images in bundle"""
        pts3d = bundle["pts3D"]
        if "constpoints" in bundle:
            pts3d = pts3d.union(bundle["constpoints"])
        info = self._filter(bundle["optim_ids"], pts3d, self._max_err(), self._option("filter_min_tri_angle"), True)
        return info["num_changed_a"] + info["num_changed_b"], (self.filter_images() if filter_ims else None)

    def filter_images(self):
        rec, obs = self.rec, self.rec.obs
        before = set(rec.registered_images.keys())
        obs.filter_images(self._option("min_focal_length_ratio"), self._option("max_focal_length_ratio"), self._option("max_extra_param"))
        for imid, image in list(rec.registered_images.items()):
            if image.num_points3D == 0:
                obs.deregister_image(imid)
        return before - set(rec.registered_images.keys())

    def filter_local_points3D(self, local_bundle, filter_max_reproj_error, filter_min_tri_angle):
        """Filters 3D points in local bundle"""
        pts3d = local_bundle["pts3D"]
        if "constpoints" in local_bundle:
            pts3d = pts3d.union(local_bundle["constpoints"])
        info = self._filter(local_bundle["optim_ids"], pts3d, filter_max_reproj_error, filter_min_tri_angle, False)
        return info["num_changed_a"] + info["num_changed_b"]

    def filter_all_points3D(self, filter_max_reproj_error, filter_min_tri_angle):
        """Filters all 3D points"""
        return self._filter(None, None, filter_max_reproj_error, filter_min_tri_angle, False)["num_changed_b"], True

    def find_invalid_depth_points(self, imids):
        """Finds invalid depth points for given image ids"""
        st, point_ids = self._state()
        _, flags = self._invalid_depth_flags(imids, st)
        sq, out = self.sq, []
        for imid in imids:
            i = sq.im_index[imid]
            row = slice(sq.kp_start[i], sq.kp_start[i + 1])
            out.append(set(point_ids[st["kp_point"][row][flags[row] != 0]].tolist()))
        return out

    # -- the reference's bundles -----------------------------------------------------------------------------------------------------
    def _points_of(self, imids, st, point_ids):
        """One boolean mark per point: seen by a keypoint of the given images."""
        sq = self.sq
        chosen = np.zeros(len(sq.image_ids), bool)
        chosen[[sq.im_index[i] for i in imids]] = True
        seen = np.zeros(len(point_ids), bool)
        kp = (st["kp_point"] >= 0) & chosen[sq.kp_image]
        seen[st["kp_point"][kp]] = True
        return seen

    def find_local_bundle(self, refimid, num_images=None, return_points=True):
        """Finds local bundle around image. image -1 is the reference image"""
        if num_images == 0 and not return_points:
            return {"optim_ids": set([refimid])}
        optim_imids = set(self.sq.find_local_bundle_ids(refimid, num_images)) | {refimid}
        out = {"ref_id": refimid, "optim_ids": optim_imids}
        if return_points:
            st, point_ids = self._state()
            mine = self._points_of([refimid], st, point_ids)
            out["pts3D"] = set(point_ids[mine].tolist())
            out["constpoints"] = set(point_ids[self._points_of(optim_imids, st, point_ids) & ~mine].tolist())
        return out

    def find_global_bundle(self):
        """Get global bundle"""
        rec = self.rec
        return {"optim_ids": set(imid for imid, image in rec.images.items() if image.has_pose), "pts3D": set(rec.points3D.keys()),
                "constpoints": set()}

    def find_subset_bundle(self, bundle):
        """Get subset bundle"""
        sq = self.sq
        imids = bundle["optim_ids"]
        st, point_ids = self._state()
        seen = self._points_of(imids, st, point_ids)
        kp = st["kp_point"] >= 0
        kp[kp] = seen[st["kp_point"][kp]]
        sees = np.zeros(len(sq.image_ids), bool)
        sees[sq.kp_image[kp]] = True  # images with a keypoint on a seen point
        optim_ids = set(imids) | {imid for imid, s, r in zip(sq.image_ids, sees.tolist(), st["registered"].tolist()) if s and r}
        return {"optim_ids": optim_ids, "pts3D": set(point_ids[seen].tolist())}
