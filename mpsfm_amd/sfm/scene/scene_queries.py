"""What the incremental loop asks of a scene between two registrations, over libmpsfm_hip.

``SceneQueries(mpsfm_rec, correspondence_graph)`` answers, each in ONE native call over the flat arrays the track engine already
gathers (``graph_arrays`` / ``state_arrays`` of sfm/mapper/track_engine.py):

* ``visibility()``: COLMAP's per-image statistics ``num_visible_points3D``, ``point3D_visibility_score`` and ``num_observations``
  of ALL images, which the reference asks of ``pycolmap.ObservationManager`` once per image (mpsfm/sfm/mapper/image_selection.py:78-88);
* ``find_local_bundle_ids(refimid, num_images=None)``: the reference's ``MpsfmReconstruction.find_local_bundle_ids``
  (mpsfm/sfm/scene/reconstruction/base.py:147-156, ``pycolmap.IncrementalMapperImpl.find_local_bundle``), with its signature and its
  ``colmap_options`` lookup;
* ``find_local_bundles(ref_ids, num_images)``: the same for many images at once, for the loop over the "risky" images of
  ``MpsfmTriangulator.retriangulate``.

The keypoints and the correspondence graph are gathered once, when the object is made; poses, registration flags and the
keypoint -> point assignment are read from the scene at every call, so nothing has to be kept up to date between calls.
"""

from __future__ import annotations

import numpy as np

from ... import capi
from ..mapper.track_engine import graph_arrays, state_arrays

NUM_VISIBILITY_LEVELS = 6        # COLMAP's Image::kNumPoint3DVisibilityPyramidLevels
LOCAL_BA_NUM_IMAGES = 6          # IncrementalMapperOptions.local_ba_num_images
LOCAL_BA_MIN_TRI_ANGLE = 6.0     # IncrementalMapperOptions.local_ba_min_tri_angle, degrees


class SceneQueries:
    def __init__(self, mpsfm_rec, correspondence_graph, device: int = 0):
        self.rec, self.cg, self.device = mpsfm_rec, correspondence_graph, device
        for k, v in graph_arrays(correspondence_graph, mpsfm_rec).items():
            setattr(self, k, v)
        cams = [mpsfm_rec.rec.cameras[mpsfm_rec.images[i].camera_id] for i in self.image_ids]
        self.image_size = np.array([[int(c.width), int(c.height)] for c in cams], np.int32).reshape(-1, 2)
        below = np.concatenate([[0], np.cumsum(np.diff(self.corr_start) > 0)])  # keypoints with a correspondence below keypoint k
        self.num_observations = below[self.kp_start[1:]] - below[self.kp_start[:-1]]  # Image.num_observations
        self.last_info = None

    def _state(self):
        st, _ = state_arrays(self.rec, self.image_ids, self.kp_start)
        return st

    # -- which image to register next ----------------------------------------------------------------------------------------------
    def visibility(self, num_levels: int = NUM_VISIBILITY_LEVELS) -> dict:
        """{image id: {"num_visible_points3D", "point3D_visibility_score", "num_observations"}} of every image of the scene."""
        st = self._state()
        out = capi.visibility_scores(self.kp_start, self.kp_xy, self.corr_start, self.corr_kp, st["kp_point"], self.image_size,
                                     num_levels=num_levels, device=self.device, return_kp_visible=False)
        self.last_info = out["info"]
        return {imid: {"num_visible_points3D": int(out["num_visible"][i]), "point3D_visibility_score": int(out["score"][i]),
                       "num_observations": int(self.num_observations[i])} for i, imid in enumerate(self.image_ids)}

    # -- the local bundle ----------------------------------------------------------------------------------------------------------
    def _local_ba_options(self, num_images=None):
        """(local_ba_num_images, local_ba_min_tri_angle) as the reference looks them up: mpsfm_rec.conf.colmap_options where the scene
        has one (a mapping; the "<--->" placeholder of an unfilled conf counts as empty), COLMAP's defaults otherwise."""
        options = getattr(getattr(self.rec, "conf", None), "colmap_options", None)
        confs = {k: v for k, v in (options.items() if hasattr(options, "items") else ()) if k in {"local_ba_min_tri_angle", "local_ba_num_images"}}
        if num_images is not None:
            confs["local_ba_num_images"] = num_images
        return int(confs.get("local_ba_num_images", LOCAL_BA_NUM_IMAGES)), float(confs.get("local_ba_min_tri_angle", LOCAL_BA_MIN_TRI_ANGLE))

    def find_local_bundles(self, ref_ids, num_images=None) -> list:
        """The local bundle (image ids, best first) of every image id of `ref_ids`: one call for all of them."""
        ref_ids = list(ref_ids)
        num_images, min_tri_angle = self._local_ba_options(num_images)
        st = self._state()
        out = capi.local_bundles(self.kp_start, st["registered"], st["cam_quat_xyzw"], st["cam_t"], st["kp_point"], st["xyz"],
                                 [self.im_index[i] for i in ref_ids], num_images, min_tri_angle, device=self.device)
        self.last_info = out["info"]
        return [[self.image_ids[j] for j in row[:n]] for row, n in zip(out["bundle"], out["bundle_len"])]

    def find_local_bundle_ids(self, refimid, num_images=None) -> list:
        return self.find_local_bundles([refimid], num_images)[0]
