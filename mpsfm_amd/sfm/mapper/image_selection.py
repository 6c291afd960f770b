"""Which image to register next: drop-in for the reference's ``ImageSelection`` (mpsfm/sfm/mapper/image_selection.py:6-179).

The same ``default_conf``, the eight ranking methods under the reference's names, ``find_init_pairs``, ``next_image``, ``at_success``,
``at_failure``, ``freeze_imids``, ``candid``, ``registration_order`` and ``mpsfm_rec.best_next_ref_imid``, with the reference's values:
a fixture computed by the reference's own code pins them (tests/golden/reference_image_selection.npz).

The three methods that rest on COLMAP's per-image visibility statistics (MAX_VISIBLE_POINTS_NUM, MAX_VISIBLE_POINTS_RATIO,
MIN_UNCERTAINTY) take the statistics of ALL candidates from one ``SceneQueries.visibility()`` call per ``next_image`` (one native
call), where the reference asks ``mpsfm_rec.obs`` once per image.  The other five are host lookups in
``correspondences`` against every registered image, as in the reference.
"""

from __future__ import annotations

import numpy as np

from ...baseclass import BaseClass

VISIBILITY_METHODS = ("MAX_VISIBLE_POINTS_NUM", "MAX_VISIBLE_POINTS_RATIO", "MIN_UNCERTAINTY")
METHODS = {  # conf.image_selection_method -> the ranking method, the reference's table
    "MAX_VISIBLE_POINTS_NUM": "rank_next_image_max_visible_points_num",
    "MAX_VISIBLE_POINTS_RATIO": "rank_next_image_max_visible_points_ratio",
    "MIN_UNCERTAINTY": "rank_next_image_min_uncertainty",
    "MAX_NUM_CORRESPONDENCES": "rank_next_image_max_num_correspondences",
    "MAX_NUM_INLIER_CORRESPONDENCES": "rank_next_image_max_num_inlier_correspondences",
    "MAX_NUM_INLIER_CORRESPONDENCES_TOT": "rank_next_image_max_num_inlier_correspondences_tot",
    "MAX_NUM_INLIER_SCORES_TOT": "rank_next_image_max_num_inlier_matcher_scores_tot",
    "MAX_MATCHER_INLIER_SCORES": "rank_next_image_max_sum_inlier_matcher_scores",
}
NOT_VERIFIED = 1e-6  # what a pair without a verified geometry counts in find_init_pairs


def filtered_image_pairs(mpsfm_rec, two_view_geom, two_view_config=2) -> list:
    """The rule of the reference's MpsfmReconstruction.filtered_image_pairs (mpsfm/sfm/scene/reconstruction/base.py:103-114) for a
    scene object without that method: the pairs of scene images whose verified two-view geometry has the given config, as sorted
    tuples (imid1 < imid2) in ascending order.  A pair's geometry is read under the order of its ids in which a double loop over
    the scene's images first meets it, as in the reference."""
    ids = list(mpsfm_rec.images.keys())
    found = set()
    for first in ids:
        for second in ids:
            pair = (min(first, second), max(first, second))
            if first == second or pair in found:
                continue
            geom, verified = two_view_geom(mpsfm_rec.images[first].name, mpsfm_rec.images[second].name)
            if verified and geom.config == two_view_config:
                found.add(pair)
    return sorted(found)


class ImageSelection(BaseClass):
    default_conf = {"image_selection_method": "MAX_MATCHER_INLIER_SCORES", "colmap_options": "<--->", "verbose": 0}

    def _init(self, mpsfm_rec, correspondences, scene_queries=None, device: int = 0):
        """`scene_queries`: what answers visibility() (a SceneQueries; tests inject a restatement).  None: a SceneQueries over
        `correspondences.cg`, made when a visibility method first needs it."""
        self.mpsfm_rec, self.correspondences = mpsfm_rec, correspondences
        self.scene_queries, self.device = scene_queries, device
        self.freeze_imids = set()
        self.candid = None
        self.registration_order = []
        self._visibility = None  # the statistics of the next_image call in progress
        method = self.conf.image_selection_method
        if method not in METHODS:
            raise ValueError(f"Image selection method {method} not recognized")
        self.rank_image_func = getattr(self, METHODS[method])

    # -- the initial pair ------------------------------------------------------------------------------------------------------------
    def selection_method(self, num_inliers, **kwargs):
        """Positions by descending number of inliers (the reverse of an ascending argsort, as in the reference)."""
        return np.argsort(np.array(num_inliers))[::-1]

    def _pairs_with_config(self, two_view_config):
        if hasattr(self.mpsfm_rec, "filtered_image_pairs"):
            pairs = self.mpsfm_rec.filtered_image_pairs(self.correspondences.two_view_geom, two_view_config)
            return sorted(tuple(sorted(pair)) for pair in pairs)
        return filtered_image_pairs(self.mpsfm_rec, self.correspondences.two_view_geom, two_view_config)

    def find_init_pairs(self, exclude_init_pairs=None):
        """Candidate initial pairs, best first: the pairs of two-view config 2, then 3, ... 8, each group by descending number of
        inlier matches.  Pairs are sorted tuples (imid1 < imid2); `exclude_init_pairs` may hold them in any order or as sets."""
        excluded = {frozenset(pair) for pair in (exclude_init_pairs or [])}
        images = self.mpsfm_rec.images
        proposed = []
        for two_view_config in range(2, 9):
            pairs = [pair for pair in self._pairs_with_config(two_view_config) if frozenset(pair) not in excluded]
            if not pairs:
                continue
            num_inliers, tri_angles = [], []
            for imid1, imid2 in pairs:
                geom, verified = self.correspondences.two_view_geom(images[imid1].name, images[imid2].name)
                num_inliers.append(geom.inlier_matches.shape[0] if verified else NOT_VERIFIED)
                tri_angles.append(geom.tri_angle if verified else NOT_VERIFIED)
            proposed += [pairs[i] for i in self.selection_method(num_inliers=num_inliers, tri_angles=tri_angles)]
        return proposed

    # -- the three methods over COLMAP's visibility statistics: one call for all images ---------------------------------------------
    def _queries(self):
        if self.scene_queries is None:
            from ..scene.scene_queries import SceneQueries

            self.scene_queries = SceneQueries(self.mpsfm_rec, self.correspondences.cg, device=self.device)
        return self.scene_queries

    def _stats(self, imid):
        """The statistics of one image: of the next_image call in progress, or fetched for a direct call of a ranking method."""
        stats = self._visibility if self._visibility is not None else self._queries().visibility()
        return stats[imid]

    def rank_next_image_max_visible_points_num(self, imid):
        return {"score": self._stats(imid)["num_visible_points3D"]}

    def rank_next_image_max_visible_points_ratio(self, imid):
        stats = self._stats(imid)
        return {"score": stats["num_visible_points3D"] / stats["num_observations"]}

    def rank_next_image_min_uncertainty(self, imid):
        """COLMAP's default."""
        return {"score": self._stats(imid)["point3D_visibility_score"]}

    # -- the five host lookups against every registered image ------------------------------------------------------------------------
    def _against_registered(self, imid, value):
        """(registered images, [value(name of imid, registered image)]) in the order of mpsfm_rec.registered_images"""
        registered = list(self.mpsfm_rec.registered_images.values())
        name = self.mpsfm_rec.images[imid].name
        return registered, [value(name, image) for image in registered]

    def _num_inliers(self, name, image):
        geom, verified = self.correspondences.two_view_geom(name, image.name)
        return geom.inlier_matches.shape[0] if verified else 0

    def _matcher_score(self, name, image):
        return self.correspondences.inlier_match_scores.get(frozenset([name, image.name]), 0)

    @staticmethod
    def _best(registered, values, score):
        return {"score": score, "refid": registered[np.argmax(values)].image_id}

    def rank_next_image_max_num_correspondences(self, imid):
        count = self.correspondences.num_correspondences_between_images
        reg_imids = list(self.mpsfm_rec.registered_images.keys())
        counts = [count(imid, reg_imid) for reg_imid in reg_imids]
        best = np.argmax(counts)
        return {"score": counts[best], "refid": reg_imids[best]}

    def rank_next_image_max_num_inlier_correspondences(self, imid):
        registered, counts = self._against_registered(imid, self._num_inliers)
        return self._best(registered, counts, counts[np.argmax(counts)])

    def rank_next_image_max_num_inlier_correspondences_tot(self, imid):
        registered, counts = self._against_registered(imid, self._num_inliers)
        return self._best(registered, counts, np.sum(counts))

    def rank_next_image_max_num_inlier_matcher_scores_tot(self, imid):
        registered, scores = self._against_registered(imid, self._matcher_score)
        return self._best(registered, scores, np.sum(scores))

    def rank_next_image_max_sum_inlier_matcher_scores(self, imid):
        """The largest matcher-score sum against one registered image; a pair with ignored absolute-pose matches is weighted by
        kept / ignored, the reference's expression."""
        registered, scores = self._against_registered(imid, self._matcher_score)
        ignored = self.mpsfm_rec.images[imid].ignore_matches_AP
        for i, image in enumerate(registered):
            if image.imid in ignored:
                mask = ignored[image.imid]
                scores[i] *= (~mask).sum() / mask.sum()
        return self._best(registered, scores, scores[np.argmax(scores)])

    # -- the loop's interface ---------------------------------------------------------------------------------------------------------
    def next_image(self, qry_imids=None):
        """Sets `candid` (and mpsfm_rec.best_next_ref_imid) to the best unregistered, unfrozen image; False when there is none."""
        if qry_imids is None:
            qry_imids = [imid for imid, image in self.mpsfm_rec.images.items() if not image.has_pose and imid not in self.freeze_imids]
        if len(qry_imids) == 0:
            return False
        if self.conf.image_selection_method in VISIBILITY_METHODS:
            self._visibility = self._queries().visibility()  # all candidates in one call
        try:
            ranked = [self.rank_image_func(imid) for imid in qry_imids]
        finally:
            self._visibility = None
        best = np.argsort([out["score"] for out in ranked])[-1]  # the reference's choice among equal scores
        self.mpsfm_rec.best_next_ref_imid = ranked[best].get("refid")
        self.candid = qry_imids[best]
        return True

    def at_success(self):
        """The candidate was registered: it joins the order, and frozen images may be tried again."""
        self.freeze_imids = set()
        self.registration_order.append(self.candid)
        self.log(50 * "=" + f"\nImage {self.mpsfm_rec.images[self.candid].name} registered\n" + 50 * "=", level=2)

    def at_failure(self, imid):
        """Registration of imid failed: it is not proposed again until another image succeeds."""
        self.freeze_imids.add(imid)
