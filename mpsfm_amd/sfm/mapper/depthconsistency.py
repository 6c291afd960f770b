"""Drop-in ``DepthConsistencyChecker`` over libmpsfm_hip.

Host-side mirror of reference ``mpsfm/sfm/mapper/depthconsistency.py`` (class DepthConsistencyChecker, :6-246): same
configuration, constructor, attributes and methods.  The bookkeeping (thresholds, failure counters, flags on the images)
stays host Python and follows the reference line by line; the per-pixel work of ``check_depth_consistency`` and
``check_bundle_depth_concistency`` (reprojection, z-buffer, lifted covariances, classification) runs in
``csrc/depth_consistency.hip`` through ``mpsfm_depth_consistency``.  The reference's quirks are kept: the z-buffer keeps
the last writer in raster order (``find_min_buffer`` compares against an all-inf buffer), the depth maps of both images
of every pair are clamped in place (``<= 0 -> 0.1``), and the test value uses the winner's depth at the target pixel.
There is no CPU fallback: without a device the calls raise ``MpsfmHipError``.
"""

from __future__ import annotations

import numpy as np

from ...baseclass import BaseClass
from .bundle_adjustment import pinhole_params

_KEYS = ("in", "surface", "occl", "invalid")


class DepthConsistencyChecker(BaseClass):
    """Class to check depth consistency of an image."""

    default_conf = {
        "depth_cons_valid_thresh": 0.6,
        "depth_cons_thresh": 0.15,
        "init_depth_cons_thresh": 0.09,
        "init_valid_thresh": 0.8,
        "depth_consistency_resample": False,  # exploration
        "verbose": 0,
    }

    def _init(self, mpsfm_rec, correspondences, device: int = 0):
        self.mpsfm_rec = mpsfm_rec
        self.correspondences = correspondences
        self.device = device

        self.depth_cons_thresh = self.conf.depth_cons_thresh
        self.reg_batch_dc_times_failed = 0
        self.cons_thresh_times_increased = 0
        self.skip_dc_check = False

    # -- host bookkeeping (reference :26-51, :174-244) ---------------------------------------------------------------
    def at_registration_success(self):
        """Reset depth consistency variables after successful registration."""
        self.log("Resetting depth consistency variables", level=2)
        self.cons_thresh_times_increased = 0
        self.depth_cons_thresh = self.conf.depth_cons_thresh
        self.reg_batch_dc_times_failed = 0
        for imid in self.mpsfm_rec.images:
            self.mpsfm_rec.images[imid].ignore_matches_AP = {}
            self.mpsfm_rec.images[imid].failed_dc_check = False
        self.skip_dc_check = False

    def relax_thresholds(self):
        """Relax depth consistency thresholds after failed registration."""
        self.log("Relaxing depth consistency thresholds", level=1)
        self.depth_cons_thresh *= 1.3
        self.cons_thresh_times_increased += 1
        self.reg_batch_dc_times_failed = 0
        for imid in self.mpsfm_rec.images:
            self.mpsfm_rec.images[imid].ignore_matches_AP = {}
            self.mpsfm_rec.images[imid].failed_dc_check = False
        self.log(f"\tNew depth consistency threshold: {self.depth_cons_thresh}", level=1)
        self.log(f"\tCons thresh times increased: {self.cons_thresh_times_increased}", level=1)
        self.log(f"\tDepth consistency failed {self.reg_batch_dc_times_failed} times", level=1)

    def find_min_buffer(self, Dab, Pab, buffer_shapes):
        """Find the minimum distance buffer for depth consistency check (reference host function, kept for API
        completeness; the device path implements its effective semantics: the last writer per target pixel)."""
        min_dabs_out = np.full(buffer_shapes, np.inf)
        Pab_x, Pab_y = np.array(Pab).T

        mask = Dab < min_dabs_out[Pab_y, Pab_x]
        min_dabs_out[Pab_y[mask], Pab_x[mask]] = Dab[mask]

        return min_dabs_out, mask

    def init_pair(self, init_pair):
        """Check if the initial pair of images is valid based on depth consistency."""
        ref_imid = list(init_pair)[0]
        score_thresh = self.conf.init_valid_thresh
        out = self.check_bundle_depth_concistency(ref_imid, {"optim_ids": init_pair}, score_thresh=score_thresh)
        success = out[0] <= self.conf.init_depth_cons_thresh
        return success

    def pre_fail(self, imid):
        """Check if the image should be failed before registration based on previous depth consistency."""
        last_dc_score = self.mpsfm_rec.images[imid].last_dc_score
        if last_dc_score is None:
            return False

        times_inliers_resampled = self.mpsfm_rec.images[imid].dc_times_inliers_resampled
        if self.conf.depth_consistency_resample and times_inliers_resampled == 0:
            return False

        if self.skip_dc_check:
            return False

        # the reference stops here (its decision below this line is unreachable)
        raise NotImplementedError("This should be implemented")

    def at_failure(self, imid):
        """Handle failure of depth consistency check."""
        image = self.mpsfm_rec.images[imid]
        image.failed_dc_check = True
        if self.conf.depth_consistency_resample:  # exploration
            image.dc_times_inliers_resampled += 1
            print(f"Removing inliers for AP for im {imid}")
            for ref_id, inlier_mask in self.mpsfm_rec.last_ap_inlier_masks.items():
                if len(inlier_mask) > 0:
                    if ref_id in self.mpsfm_rec.images[imid].ignore_matches_AP:
                        used = ~self.mpsfm_rec.images[imid].ignore_matches_AP[ref_id]
                        self.mpsfm_rec.images[imid].ignore_matches_AP[ref_id][used] |= inlier_mask
                    else:
                        self.mpsfm_rec.images[imid].ignore_matches_AP[ref_id] = inlier_mask
            self.reg_batch_dc_times_failed += 1
        else:
            self.reg_batch_dc_times_failed += 1

    def check_image(self, imid, bundle):
        """Check depth consistency of an image in local bundle."""
        score, _ = self.check_bundle_depth_concistency(imid, bundle)

        if score > self.depth_cons_thresh:
            print(f"\nDepth consistency failed for {imid}: {score}!!!")
            self.at_failure(imid)
            return False
        self.log(f"Depth consistency passed for {imid}: {score}", level=1)
        return True

    # -- device-backed ------------------------------------------------------------------------------------------------
    def _image_entry(self, imid):
        """The image's row of the C image table.  depth.data is handed over in place (the clamp lands in it); a map that
        is not a writable C-contiguous float64 array goes through a copy that is written back after the call."""
        image = self.mpsfm_rec.images[imid]
        camera = self.mpsfm_rec.camera(imid)
        fx, fy, cx, cy = pinhole_params(camera)
        sx, sy = float(camera.sx), float(camera.sy)
        data = image.depth.data
        ok = isinstance(data, np.ndarray) and data.dtype == np.float64 and data.flags.c_contiguous and data.flags.writeable
        depth = data if ok else np.ascontiguousarray(data, np.float64).copy()
        entry = dict(depth=depth, variance=image.depth.uncertainty, prior_std_multiplier=image.depth.conf.prior_std_multiplier,
                     intr_scaled=(fx * sx, fy * sy, cx * sx, cy * sy), intr=(fx, fy, cx, cy),
                     cam_from_world=np.asarray(image.cam_from_world.matrix(), np.float64))
        return entry, (None if ok else data)

    def _run(self, imid, ref_ids, c, score_thresh, return_codes):
        from ... import capi

        ids = [imid] + [r for r in ref_ids if r != imid]
        entries, writeback = [], []
        for i in ids:
            e, orig = self._image_entry(i)
            entries.append(e)
            writeback.append(orig)
        pairs = [(0, k) for k in range(1, len(ids))]
        try:
            return capi.depth_consistency(entries, pairs, c=c, score_thresh=score_thresh, device=self.device,
                                          return_codes=return_codes)
        finally:
            for e, orig in zip(entries, writeback):
                if orig is not None:
                    orig[...] = e["depth"]

    def check_depth_consistency(self, imid1, imid2, c=15, score_thresh=None):
        """Check depth consistency between two images: the reference's ten H x W masks, rebuilt from the per-pixel codes
        of one device call."""
        if score_thresh is None:
            score_thresh = self.conf.depth_cons_valid_thresh
        from ...capi import DC_IN, DC_INVALID, DC_OCCL, DC_SURFACE

        _, _, codes = self._run(imid1, [imid2], c, score_thresh, True)
        c1, c2 = codes[0]
        out = {}
        for tag, code in (("1", c1), ("2", c2)):
            out["valid" + tag] = (code & (DC_SURFACE | DC_OCCL)) != 0
            out["occl" + tag] = (code & DC_OCCL) != 0
            out["invalid" + tag] = (code & DC_INVALID) != 0
            out["surface" + tag] = (code & DC_SURFACE) != 0
            out[f"valid{tag}_mask"] = (code & DC_IN) != 0
        keys = ["valid1", "valid2", "occl1", "occl2", "invalid1", "invalid2", "surface1", "surface2", "valid1_mask", "valid2_mask"]
        return {k: out[k] for k in keys}

    def check_bundle_depth_concistency(self, imid, bundle, score_thresh=None):
        """Check depth consistency of a bundle of images: one device call for every pair, counts transferred only.
        Returns (max of the reference and query not-valid ratios, (query pixels in canvas, reference pixels in canvas))."""
        self.log(f"Checking depth consistency of {imid}: {self.mpsfm_rec.images[imid].name}...", level=2)
        if score_thresh is None:
            score_thresh = self.conf.depth_cons_valid_thresh
        optim_ids = list(set(bundle["optim_ids"]) - {imid})
        if not optim_ids:
            return np.max([0.0, 0.0]), (0, 0)
        counts, _ = self._run(imid, optim_ids, 15, score_thresh, False)
        tot = counts.sum(axis=0)  # [leg][in, surface, occl, invalid]; leg 0: query -> ref, 1: ref -> query
        q_in, q_surf, q_occl = (int(v) for v in tot[0, :3])
        r_in, r_surf, r_occl = (int(v) for v in tot[1, :3])
        tot_ref_im_ratios = (r_in - r_surf - r_occl) / np.clip(r_in - r_occl, 0.1, None)
        tot_qry_im_ratios = (q_in - q_surf - q_occl) / np.clip(q_in - q_occl, 0.1, None)
        max_ratios = np.max([tot_ref_im_ratios, tot_qry_im_ratios])
        return max_ratios, (q_in, r_in)
