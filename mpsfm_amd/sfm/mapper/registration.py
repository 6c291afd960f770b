"""Drop-in ``MpsfmRegistration`` over libmpsfm_hip.

Host-side mirror of reference ``mpsfm/sfm/mapper/registration.py`` (class MpsfmRegistration, :11-441): same configuration,
constructor, attributes and public methods.  The decisions (which rows go to the estimator, inlier-mask remapping, the
parallax branch, the merge of lifted and triangulated candidates, which points are added) stay host Python and follow the
reference; the per-match arithmetic runs in ``csrc/registration.hip``:

  register_next_image                  one ``mpsfm_registration_pairs`` launch for all reference images (gather of the
                                       triangulated points, depth sample + lift of the others), then ``AbsolutePose``
  register_and_triangulate_init_pair   ``RelativePose``, one ``mpsfm_init_pair_candidates`` launch (two-view triangulation,
                                       lifted points, angles, cheirality of every match), ``AbsolutePose`` on the lifted
                                       points, then a second launch for the chosen branch (the median rescale of the
                                       high-parallax branch is one ``np.median`` on the host between the two)

The scene is read through bulk accessors where it has them (``mpsfm_rec.keypoints``, ``point3D_coordinates``,
``image.point3D_ids(idxs)``), with the per-object walk as the fallback for real pycolmap objects.

Kept quirks of the reference: the triangulation angle is ``calculate_triangulation_angle`` of
mpsfm/utils/geometry.py, which works on plain lengths where its names say squared lengths; risky points are lifted, not
dropped; both images of an init pair are registered before the candidates are counted; in the merge the i-th common
candidate is judged by the i-th angle of the WHOLE triangulated list and the two common lists pair up by position.
Deviations: when the relative pose fails the reference raises TypeError, here ``register_and_triangulate_init_pair`` returns
False and leaves the scene untouched; an init pair without any lifted candidate returns the triangulated ones where the
reference raises KeyError.  There is no CPU fallback: without a device the calls raise ``MpsfmHipError``.
"""

from __future__ import annotations

from collections import defaultdict

import numpy as np

from ... import capi
from ...baseclass import BaseClass
from .bundle_adjustment import pinhole_params

_INVALID_POINT3D = np.uint64(18446744073709551615)  # pycolmap's kInvalidPoint3DId
_KEYS = ("pt2d_id_1", "pt2d_id_2", "tri_angle", "posdepth1", "posdepth2", "xyz")


def _identity():
    from ..estimators.absolute_pose import make_rigid3d  # not at module level: the estimators import this package

    return make_rigid3d([0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0])


def merge_candidates(lifted: dict, triangulated: dict, thresh: float) -> dict:
    """The reference's combination of lifted and triangulated init candidates (:309-339), vectorised, with its output
    order: the common ids in the order of the lifted list, then the lifted-only candidates with an angle below `thresh`,
    then the triangulated-only ones at or above it.  As there, the k-th common candidate pairs the k-th common lifted row
    with the k-th common triangulated row (by position, not by id) and is judged by the k-th angle of the whole
    triangulated list.  Inputs and output: dicts of equal-length arrays with the keys of _KEYS."""
    ids1, ids2 = np.asarray(lifted["pt2d_id_1"], np.int64), np.asarray(triangulated["pt2d_id_1"], np.int64)
    in2, in1 = np.isin(ids1, ids2), np.isin(ids2, ids1)
    cl, ct = np.flatnonzero(in2), np.flatnonzero(in1)
    m = min(len(cl), len(ct), len(ids2))
    ang_l, ang_t = np.asarray(lifted["tri_angle"], np.float64), np.asarray(triangulated["tri_angle"], np.float64)
    take_lifted = ang_t[:m] < thresh
    only_l = np.flatnonzero(~in2)
    only_l = only_l[ang_l[only_l] < thresh]
    only_t = np.flatnonzero(~in1)
    only_t = only_t[ang_t[only_t] >= thresh]
    out = {}
    for k in _KEYS:
        a, b = np.asarray(lifted[k]), np.asarray(triangulated[k])
        sel = take_lifted.reshape((-1,) + (1,) * (a.ndim - 1))
        out[k] = np.concatenate([np.where(sel, a[cl[:m]], b[ct[:m]]), a[only_l], b[only_t]])
    return out


class MpsfmRegistration(BaseClass):
    """MP-SfM Registration class. This class is used to register images and triangulate points."""

    default_conf = {
        "lifted_registration": True,  # important for ablation but can be removed
        "absolute_pose": {},
        "relative_pose": {},
        "reduce_min_inliers_at_failure": 6,  # release
        # dev
        "parallax_thresh": 1.5,  # exploration
        "combined_triangle_thresh": 1.5,
        "robust_triangles": 1,
        "resample_bunlde": False,  # exploration,
        "colmap_options": "<--->",
        "verbose": 0,
    }

    def _init(self, mpsfm_rec, correspondences, triangulator, device: int = 0, backend=None, **kwargs):
        self.mpsfm_rec = mpsfm_rec
        self.correspondences = correspondences
        self.triangulator = triangulator
        self.device = device
        # the two per-match calls; anything with capi's registration_pairs / init_pair_candidates (tests: the NumPy restatement)
        self.backend = capi if backend is None else backend
        from ..estimators import AbsolutePose, RelativePose  # not at module level: the estimators import this package

        self.relative_pose_estimator = RelativePose(self.conf.relative_pose, device=device)
        self.absolute_pose_estimator = AbsolutePose(self.conf.absolute_pose, device=device)

        self.half_ap_min_inliers = 0
        self.registration_cache = defaultdict(dict)

    # -- scene access: bulk where the scene offers it -------------------------------------------------------------------
    def _keypoints(self, imid):
        rec = self.mpsfm_rec
        if hasattr(rec, "keypoints"):
            return np.asarray(rec.keypoints(imid), np.float64).reshape(-1, 2)
        return np.array([p.xy for p in rec.images[imid].points2D], np.float64).reshape(-1, 2)

    @staticmethod
    def _point3D_ids(image, idxs):
        """uint64 ids of the 3-D points of keypoints `idxs` (the invalid id where there is none)"""
        idxs = np.asarray(idxs, np.int64)
        if hasattr(image, "point3D_ids"):
            return np.asarray(image.point3D_ids(idxs), dtype=np.uint64)
        p2 = image.points2D
        return np.array([p2[int(i)].point3D_id if p2[int(i)].has_point3D() else _INVALID_POINT3D for i in idxs], dtype=np.uint64)

    def _point3D_xyz(self, ids):
        rec = self.mpsfm_rec
        if len(ids) == 0:
            return np.zeros((0, 3))
        if hasattr(rec, "point3D_coordinates"):
            return np.asarray(rec.point3D_coordinates(ids), np.float64).reshape(-1, 3)
        return np.array([rec.points3D[int(p)].xyz for p in ids], np.float64).reshape(-1, 3)

    def _pose_arrays(self, image):
        pose = image.cam_from_world
        return np.asarray(pose.rotation.quat, np.float64), np.asarray(pose.translation, np.float64)

    # -- next image ----------------------------------------------------------------------------------------------------------
    def _gather_2D3D_pairs(self, imid, ref_imids):
        """The rows of the reference's pair2D3D for all reference images at once (:68-94, :341-373, :393-413): returns
        (points2D, points3D, stack_order, lifted_mask, ids3d, ref_match_sizes) in sorted(ref ids) order."""
        rec, conf = self.mpsfm_rec, self.conf
        image = rec.images[imid]
        stack_order = sorted(set(ref_imids))
        kps_qry = None
        refs, m_ref, m_xy, m_qry, m_pid = [], [], [], [], []
        for k, ref_id in enumerate(stack_order):
            image_ref = rec.images[ref_id]
            camera_ref = rec.rec.cameras[image_ref.camera_id]
            q, t = self._pose_arrays(image_ref)
            refs.append(dict(depth_map=image_ref.depth.data if conf.lifted_registration else None, sx=camera_ref.sx, sy=camera_ref.sy,
                             intr=pinhole_params(camera_ref), quat_xyzw=q, t=t))
            corr = np.asarray(self.correspondences.matches(ref_id, imid))
            if ref_id in image.ignore_matches_AP:
                corr = corr[~image.ignore_matches_AP[ref_id]]
            if len(corr) == 0:
                continue
            if kps_qry is None:
                kps_qry = self._keypoints(imid)
            ids_ref, ids_qry = corr[:, 0].astype(np.int64), corr[:, 1].astype(np.int64)
            m_ref.append(np.full(len(corr), k, np.int32))
            m_xy.append(self._keypoints(ref_id)[ids_ref])
            m_qry.append(kps_qry[ids_qry])
            m_pid.append(self._point3D_ids(image_ref, ids_ref))
        n_refs = len(stack_order)
        if not m_ref:
            return np.zeros((0, 2)), np.zeros((0, 3)), stack_order, np.zeros(0, bool), np.zeros(0, int), [0] * n_refs
        m_ref, m_xy, m_qry, m_pid = np.concatenate(m_ref), np.concatenate(m_xy), np.concatenate(m_qry), np.concatenate(m_pid)
        has = m_pid != _INVALID_POINT3D
        uids, inv = np.unique(m_pid[has], return_inverse=True)
        match_pt = np.full(len(m_pid), -1, np.int32)
        match_pt[has] = inv
        risky = None
        if conf.robust_triangles is not None and conf.lifted_registration and len(uids):
            # per point, so one call for the union of all reference images' ids gives what the reference's call per image does
            risky = np.asarray(rec.find_points3D_with_small_triangulation_angle(min_angle=conf.robust_triangles, point3D_ids=uids), bool)
        xyz, kind = self.backend.registration_pairs(refs, m_ref, m_xy, match_pt, self._point3D_xyz(uids), pt_risky=risky,
                                                    lifted_registration=bool(conf.lifted_registration), device=self.device)
        keep = kind != capi.REG_DROPPED  # without lifted_registration only the triangulated rows remain
        lifted = kind[keep] == capi.REG_LIFTED
        sizes = np.bincount(m_ref[keep], minlength=n_refs).tolist()
        ids3d = m_pid[kind == capi.REG_TRIANGULATED].astype(np.int64)
        return m_qry[keep], xyz[keep], stack_order, lifted, ids3d, sizes

    def register_next_image(self, imid, ref_imids=None, **kwargs):
        """Register next image and triangulate points."""
        rec = self.mpsfm_rec
        image = rec.images[imid]
        camera = rec.rec.cameras[image.camera_id]

        if ref_imids is None:
            ref_imids = rec.registered_images.keys()

        self.registration_cache[imid]["store_matches"] = {}
        ref_imids = list(ref_imids)
        ap_min_num_inliers = self.conf.colmap_options.abs_pose_min_num_inliers
        if self.half_ap_min_inliers:
            ap_min_num_inliers = int(ap_min_num_inliers / (1.2**self.half_ap_min_inliers))
        force_registration = self.half_ap_min_inliers >= self.conf.reduce_min_inliers_at_failure

        while True:
            points2D, points3D, stack_order, lifted_mask, ids3d, ref_match_sizes = self._gather_2D3D_pairs(imid, ref_imids)

            unique_ids3d, unique_indices, el_to_unique_index = np.unique(ids3d, return_index=True, return_inverse=True)
            triangpts3D = points3D[~lifted_mask][unique_indices]
            triangpts2D = points2D[~lifted_mask][unique_indices]
            points2D = np.concatenate([triangpts2D, points2D[lifted_mask]])
            points3D = np.concatenate([triangpts3D, points3D[lifted_mask]])

            if len(points2D) < 3:
                self.log(f"\nImage {imid} has less than 3 points to triangulate. Not registered")
                return False

            AP_info = self.absolute_pose_estimator(points2D, points3D, camera)
            if AP_info is None:
                self.log("\nAP estim No inliers found")
                return False

            if AP_info["num_inliers"] < ap_min_num_inliers and not force_registration:
                self.log(f"\nAP estim Not enough inliers: {ap_min_num_inliers}")
                return False

            inlier_mask = np.asarray(AP_info["inlier_mask"], bool)
            split_indices = np.cumsum(ref_match_sizes)[:-1]
            # mapping back masks to correspondences
            t_mask = inlier_mask[: len(triangpts3D)]
            l_mask = inlier_mask[len(triangpts3D):]
            remapped_inl_mask = np.ones(len(lifted_mask), dtype=bool)
            remapped_inl_mask[lifted_mask] = l_mask
            remapped_inl_mask[~lifted_mask] = t_mask[el_to_unique_index.reshape(-1)]

            split_mask = dict(zip(stack_order, np.split(remapped_inl_mask, split_indices)))
            rec.last_ap_inlier_masks = split_mask

            if self.conf.resample_bunlde:
                best_id = rec.best_next_ref_imid
                compare_ids = set(stack_order)
                compare_ids.remove(best_id)
                compare_ids = list(compare_ids)
                with np.errstate(invalid="ignore", divide="ignore"):
                    best_ratio = split_mask[best_id].sum() / len(split_mask[best_id])
                    other_ratios = [split_mask[im_ref_id].sum() / len(split_mask[im_ref_id]) for im_ref_id in compare_ids]
                self.log("Best:", best_id, "other:", compare_ids, "ratios:", best_ratio, "vs", other_ratios, level=1)
                if best_ratio < 0.1 and np.nanmax(other_ratios) > 0.2:
                    ignore = rec.images[imid].ignore_matches_AP
                    for ref_id in split_mask:
                        if len(split_mask[ref_id]) > 0:
                            if ref_id in ignore:
                                used = ~ignore[ref_id]
                                ignore[ref_id][used] |= split_mask[ref_id]
                            else:
                                ignore[ref_id] = split_mask[ref_id]
                    continue
            break

        rec.images[imid].cam_from_world = AP_info["cam_from_world"]
        rec.rec.register_image(imid)

        return True

    def register_and_triangulate_next_image(self, imid, ref_imids=None):
        """Register next image and triangulate points."""
        if not self.register_next_image(imid, ref_imids=ref_imids):
            return False

        return self.triangulate_image(imid)

    def triangulate_image(self, imid, **kwargs):
        """Triangulate points for the given image id."""
        return self.triangulator.triangulate_image(imid, **kwargs)

    # -- init pair -----------------------------------------------------------------------------------------------------------
    def _track_type(self):
        if hasattr(self.mpsfm_rec, "Track"):
            return self.mpsfm_rec.Track
        import pycolmap

        return pycolmap.Track

    def register_and_triangulate_init_pair(self, imid1, imid2):
        """Register initial image pair and triangulate it's points."""
        rec = self.mpsfm_rec
        kwargs = {
            "imid1": imid1,
            "imid2": imid2,
            "matches": np.asarray(self.correspondences.matches(imid1, imid2)),
            "kps1": self._keypoints(imid1),
            "kps2": self._keypoints(imid2),
            "camera1": rec.camera(imid1),
            "camera2": rec.camera(imid2),
        }
        out = self._init_pair_points_and_pose(**kwargs)
        if out is None:  # no relative pose: the reference raises TypeError here; the mapper moves to the next ranked pair
            self.log(f"Init pair {imid1} and {imid2}: no relative pose. Not registered")
            return False
        candidate_points, cam_from_world2 = out
        rec.images[imid1].cam_from_world = _identity()
        rec.images[imid2].cam_from_world = cam_from_world2
        rec.register_image(imid1)
        rec.register_image(imid2)
        if len(candidate_points["xyz"]) < 3:
            self.log(f"Init pair {imid1} and {imid2} has less than 3 points to triangulate. Not registered")
            return False
        id1 = np.asarray(candidate_points["pt2d_id_1"], np.int64)
        id2 = np.asarray(candidate_points["pt2d_id_2"], np.int64)
        passes = (self.conf.colmap_options.init_min_tri_angle < np.asarray(candidate_points["tri_angle"], np.float64)) \
            & np.asarray(candidate_points["posdepth1"], bool) & np.asarray(candidate_points["posdepth2"], bool)
        # keypoints that carry a point already; a point added below claims its two keypoints for the later candidates
        taken1 = set(id1[self._point3D_ids(rec.images[imid1], id1) != _INVALID_POINT3D].tolist())
        taken2 = set(id2[self._point3D_ids(rec.images[imid2], id2) != _INVALID_POINT3D].tolist())
        Track = self._track_type()
        for i in np.flatnonzero(passes):
            a, b = int(id1[i]), int(id2[i])
            if a in taken1 or b in taken2:
                continue
            track = Track()
            track.add_element(imid1, a)
            track.add_element(imid2, b)
            rec.obs.add_point3D(candidate_points["xyz"][i], track)
            taken1.add(a)
            taken2.add(b)
        return not len(rec.points3D) < 3

    @staticmethod
    def _rows(matches, cand, rows, kind):
        """candidate arrays (keys of _KEYS) of the match rows `rows` for kind "tri" or "lift" """
        return {"pt2d_id_1": matches[rows, 0], "pt2d_id_2": matches[rows, 1], "tri_angle": cand[f"{kind}_angle_deg"][rows],
                "posdepth1": cand[f"{kind}_posdepth1"][rows], "posdepth2": cand[f"{kind}_posdepth2"][rows], "xyz": cand[f"{kind}_xyz"][rows]}

    def _init_pair_points_and_pose(self, imid1, imid2, kps1, kps2, matches, camera1, camera2):
        conf = self.conf
        matches = np.asarray(matches, np.int64).reshape(-1, 2)
        kps1, kps2 = np.asarray(kps1, np.float64), np.asarray(kps2, np.float64)
        xy1, xy2 = kps1[matches[:, 0]], kps2[matches[:, 1]]
        E_info = self.relative_pose_estimator(xy1, xy2, camera1, camera2)
        if E_info is None:
            return None
        e_mask = np.asarray(E_info["inlier_mask"], bool)
        depth1 = self.mpsfm_rec.images[imid1].depth
        common = dict(xy1=xy1, xy2=xy2, intr1=pinhole_params(camera1), intr2=pinhole_params(camera2), prior_map=depth1.data_prior,
                      valid_map=depth1.valid, sx=camera1.sx, sy=camera1.sy, device=self.device)
        both = capi.INIT_TRIANGULATE | capi.INIT_LIFT

        # first launch, every match: triangulated under the relative pose, lifted from the prior depth of image 1
        first = self.backend.init_pair_candidates(cam2_from_cam1=E_info["cam2_from_cam1"].matrix(), rescale=1.0, what=both, **common)
        tri_rows = np.flatnonzero(e_mask & first["tri_ok"])
        valid_rows = np.flatnonzero(first["valid"])
        AP_info = self.absolute_pose_estimator(xy2[valid_rows], first["lift_xyz"][valid_rows], camera2)
        triangles = first["tri_angle_deg"][tri_rows]
        if AP_info is None:
            high_parallax = True
        else:
            high_parallax = (triangles > conf.parallax_thresh).sum() > AP_info["num_inliers"]
        self.log(f" -- INIT INFO --\n\t        num E inliers: {triangles.shape[0]}\n\tnum E w/ triangle>{conf.combined_triangle_thresh}: "
                 f"{(triangles > conf.combined_triangle_thresh).sum()}", level=2)
        if AP_info is not None:
            self.log(f"\t       num AP inliers: {AP_info['num_inliers']}", level=2)

        if high_parallax:
            cam_from_world2 = E_info["cam2_from_cam1"]
            if len(tri_rows) == 0:
                raise ValueError("init pair: no triangulated inlier to scale the prior depth with")  # reference: np.vstack([])
            with np.errstate(invalid="ignore", divide="ignore"):
                rescale = np.median(first["tri_xyz"][tri_rows, 2] / first["d_prior"][tri_rows])
            lift_rows = np.flatnonzero(e_mask & first["valid"])
            select = np.zeros(len(matches), np.uint8)
            select[lift_rows] = 1
            second = self.backend.init_pair_candidates(cam2_from_cam1=cam_from_world2.matrix(), rescale=float(rescale), select=select,
                                                       what=capi.INIT_LIFT, **common)
            points_lifted = self._rows(matches, second, lift_rows, "lift")
            points_triangulated = self._rows(matches, first, tri_rows, "tri")
        else:
            cam_from_world2 = AP_info["cam_from_world"]
            rows = valid_rows[np.asarray(AP_info["inlier_mask"], bool)]
            select = np.zeros(len(matches), np.uint8)
            select[rows] = 1
            second = self.backend.init_pair_candidates(cam2_from_cam1=cam_from_world2.matrix(), rescale=1.0, select=select, what=both,
                                                       **common)
            points_lifted = self._rows(matches, second, rows, "lift")
            points_triangulated = self._rows(matches, second, rows[second["tri_ok"][rows]], "tri")

        merged = merge_candidates(points_lifted, points_triangulated, conf.combined_triangle_thresh)
        return {k: list(v) for k, v in merged.items()}, cam_from_world2
