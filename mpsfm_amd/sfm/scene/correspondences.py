"""Correspondences of a scene over libmpsfm_hip: gathering, geometric verification, the correspondence graph.

Mirror of reference ``mpsfm/sfm/scene/correspondences/utils.py`` (``process_pair`` :13-32, ``geometric_verification``
:51-77, the gather functions :80-173) and ``correspondences/base.py`` (``Correspondences`` :21-139) with the reference's
signatures and options (max_num_trials 20000, min_inlier_ratio 0.1, compute_relative_pose).
By default each pair is one stateless call of ``mpsfm_two_view_geometry`` in a plain loop over the pairs in this process;
``batched=True`` gathers all pairs and makes one call of ``mpsfm_two_view_geometry_batch`` in place of the reference's process
pool, with the same result for every pair.
``Correspondences`` reads keypoints and matches from a ``CorrespondenceStore`` in memory where the reference reads the extractor's
HDF5 files, verifies all pairs in one batched call and fills a ``HipCorrespondenceGraph``, which one GPU call builds
(DESIGN.md section 4s).  HDF5 I/O stays with the reference; ``ImageSelection`` is sfm/mapper/image_selection.py.
"""

from __future__ import annotations

from collections import defaultdict
from copy import deepcopy
from itertools import chain

import numpy as np

from ...baseclass import BaseClass
from ..estimators.two_view_geometry import estimate_calibrated_two_view_geometry, estimate_calibrated_two_view_geometry_batch
from .correspondence_graph import HipCorrespondenceGraph


def pair_options(max_error) -> dict:
    """The options the reference passes for every pair."""
    return {
        "ransac": {"max_num_trials": 20000, "min_inlier_ratio": 0.1, "max_error": max_error},
        "compute_relative_pose": True,
    }


def process_pair(data, max_error, backend=None):
    """Estimates the two-view geometry of one gathered pair: (tvg, matches, name0, name1)."""
    tvg = estimate_calibrated_two_view_geometry(
        data["cam0"], data["kps0"], data["cam1"], data["kps1"], data["matches"], pair_options(max_error), backend=backend
    )
    return (tvg, data["matches"], data["name0"], data["name1"])


def gather_data(name0, name1, rec_name_to_id, reference, keypoints_cache, matches_cache):
    """The cameras, keypoints and matches of one pair."""
    out = {"name0": name0, "name1": name1}
    for k, name in (("0", name0), ("1", name1)):
        image = reference.images[rec_name_to_id[name]]
        cam = reference.cameras[image.camera_id]
        out["cam" + k] = cam.as_colmap() if hasattr(cam, "as_colmap") else cam
        out["kps" + k] = keypoints_cache[name]
    out["matches"] = matches_cache[name0, name1]
    return out


def geometric_verification(reference, pairs, max_error: float = 4.0, keypoints=None, matches=None, backend=None, batched: bool = False):
    """Geometric verification of `pairs` [(name0, name1)]: (inlier_masks, tvg_cache), both keyed (name0, name1).  `batched`: all
    pairs in one call of the batched estimator instead of one call per pair; the results are the same."""
    tvg_cache = {}
    inlier_masks = {}
    rec_name_to_id = {im.name: im.image_id for im in reference.images.values()}
    gathered = (gather_data(name0, name1, rec_name_to_id, reference, keypoints, matches) for name0, name1 in pairs)
    if batched:
        gathered = list(gathered)
        tvgs = estimate_calibrated_two_view_geometry_batch(
            [(d["cam0"], d["kps0"], d["cam1"], d["kps1"], d["matches"]) for d in gathered], pair_options(max_error), backend=backend
        )
        done = ((tvg, d["matches"], d["name0"], d["name1"]) for tvg, d in zip(tvgs, gathered))
    else:
        done = (process_pair(data, max_error, backend=backend) for data in gathered)
    for tvg, matches_, name0, name1 in done:
        tvg_cache[name0, name1] = tvg
        # the reference's expression: a match row is an inlier when an equal row is among the inlier matches, so every copy of
        # a duplicated row shares one answer
        mask = np.isin(
            matches_.view([("", matches_.dtype)] * 2), tvg.inlier_matches.view([("", tvg.inlier_matches.dtype)] * 2)
        )
        inlier_masks[(name0, name1)] = mask[:, 0]
    return inlier_masks, tvg_cache


# ---- keypoints and matches in memory ------------------------------------------------------------------------------------------------
def matches_from_matches0(matches0, matching_scores0):
    """The hloc layout the matchers of this package return (matches0 [n0] with -1, matching_scores0 [n0]) as the reference's
    get_matches reads it (mpsfm/utils/io.py:107-117): matches [n, 2], scores [n]."""
    matches0, scores0 = np.asarray(matches0), np.asarray(matching_scores0)
    idx = np.where(matches0 != -1)[0]
    return np.stack([idx, matches0[idx]], -1), scores0[idx]


class CorrespondenceStore:
    """What the reference's extractor keeps in HDF5 files, in memory: the pair list, the matcher type ("sparse" or "dense"), sparse
    keypoints per image, sparse (matches, scores) per pair, dense (kps0, kps1) and (matches, scores) per pair, and optionally the
    cached dense scores of the `cached_dense_scores` option.  A pair is found under either order of its names; read the other way
    round, its match columns are swapped (the reference's find_pair).  Every read is a copy: the gather functions modify what they
    read, as the reference's do with what h5py hands them."""

    def __init__(self, pairs, matcher_type="sparse"):
        self.pairs = [tuple(p) for p in pairs]
        self.matcher_type = matcher_type
        self.sparse_keypoints = {}
        self.matches = {"sparse": {}, "dense": {}, "cache": {}}
        self.dense_keypoints = {}

    @staticmethod
    def _pair_of(matches=None, scores=None, matches0=None, matching_scores0=None):
        if matches0 is not None:
            return matches_from_matches0(matches0, matching_scores0)
        return np.asarray(matches).reshape(-1, 2), np.asarray(scores).reshape(-1)

    def set_sparse_keypoints(self, name, keypoints):
        self.sparse_keypoints[name] = np.asarray(keypoints)

    def set_sparse_matches(self, name0, name1, matches=None, scores=None, matches0=None, matching_scores0=None):
        self.matches["sparse"][name0, name1] = self._pair_of(matches, scores, matches0, matching_scores0)

    def set_dense(self, name0, name1, kps0, kps1, matches=None, scores=None, matches0=None, matching_scores0=None):
        self.dense_keypoints[name0, name1] = (np.asarray(kps0), np.asarray(kps1))
        self.matches["dense"][name0, name1] = self._pair_of(matches, scores, matches0, matching_scores0)

    def set_cached_scores(self, name0, name1, matches=None, scores=None, matches0=None, matching_scores0=None):
        self.matches["cache"][name0, name1] = self._pair_of(matches, scores, matches0, matching_scores0)

    def get_keypoints(self, name):
        return np.array(self.sparse_keypoints[name])

    def _entry(self, table, name0, name1, what):
        """(entry, stored the other way round) of a pair in one of the tables"""
        if (name0, name1) in table:
            return table[name0, name1], False
        if (name1, name0) in table:
            return table[name1, name0], True
        raise ValueError(f"the store holds no {what} for the pair {(name0, name1)}, under either order of the names")

    def get_matches(self, kind, name0, name1):
        (m, s), swapped = self._entry(self.matches[kind], name0, name1, f"{kind} matches")
        return (np.flip(np.array(m), -1) if swapped else np.array(m)), np.array(s)

    def get_dense_2view_keypoints(self, name0, name1):
        (k0, k1), swapped = self._entry(self.dense_keypoints, name0, name1, "dense keypoints")
        return (np.array(k1), np.array(k0)) if swapped else (np.array(k0), np.array(k1))


def _pixel_centres(kps):
    """hloc's keypoints have the origin at the centre of the top-left pixel, COLMAP's at its corner.  The half pixel is added in the
    array's own precision and the result widened to float32 afterwards, which is the order the fixture pins."""
    return np.add(kps, 0.5, out=kps).astype(np.float32)


def gather_sparse_keypoints(store, ims):
    """{name: float32 [n, 2]} of the sparse keypoints of `ims`, in COLMAP's pixel convention (drop-in for reference utils.py:80-87)."""
    return {name: _pixel_centres(store.get_keypoints(name)) for name in ims}


def gather_sparse_matches(store, pairs):
    """({(name0, name1): matches [n, 2]}, {frozenset(pair): scores [n]}) of the sparse matches of `pairs`, as stored (drop-in for
    reference utils.py:90-98)."""
    read = [(tuple(pair), store.get_matches("sparse", *pair)) for pair in pairs]
    return {pair: m for pair, (m, _) in read}, {frozenset(pair): s for pair, (_, s) in read}


def gather_dense_2view(store, pairs, ims, matches_mode="dense"):
    """Keypoints, matches, scores and sparse masks of a dense matcher's output (drop-in for reference utils.py:101-173; values
    pinned by tests/golden/reference_correspondences.npz).  An image's keypoint array is a sequence of blocks: its sparse keypoints
    when the mode names "sparse" (as stored: no half-pixel shift on this path), then, when it names "dense", the dense keypoints of
    every pair the image is part of, in the order of `pairs`.  A dense match row is cut to the pair's dense keypoints and indexes the
    pair's blocks, so it is moved by what either image held when the blocks were appended.  A pair's rows are dense first, sparse
    second.  `sparse_im_masks[name]` is true on the sparse block."""
    with_sparse, with_dense = "sparse" in matches_mode, "dense" in matches_mode
    if not (with_sparse or with_dense):
        raise ValueError(f"matches_mode {matches_mode!r} names neither sparse nor dense")
    pairs = [tuple(pair) for pair in pairs]
    blocks, is_sparse, held = defaultdict(list), defaultdict(list), defaultdict(int)  # per image: arrays, flag per array, rows so far

    def append(name, kps, sparse):
        blocks[name].append(kps.astype(np.float32))
        is_sparse[name].append(sparse)
        held[name] += len(kps)

    rows, values = {pair: [] for pair in pairs}, {pair: [] for pair in pairs}
    if with_sparse:
        for name in ims:
            append(name, store.get_keypoints(name), True)
    if with_dense:
        for name0, name1 in pairs:
            m, s = store.get_matches("dense", name0, name1)
            kps0, kps1 = store.get_dense_2view_keypoints(name0, name1)
            offset = np.array([held[name0], held[name1]], dtype=np.int64)  # both read before either block is appended
            append(name0, kps0, False)
            append(name1, kps1, False)
            rows[name0, name1].append(m[:len(kps0)] + offset)
            values[name0, name1].append(s)
    if with_sparse:  # behind the dense rows of the pair
        for pair in pairs:
            m, s = store.get_matches("sparse", *pair)
            rows[pair].append(m)
            values[pair].append(s)
    keypoints = {name: np.concatenate(parts) for name, parts in blocks.items()}
    masks = {name: np.repeat(np.array(is_sparse[name], dtype=bool), [len(part) for part in parts]) for name, parts in blocks.items()}
    matches, scores = {}, {}
    for pair in pairs:
        m = np.concatenate(rows[pair])
        none = len(m) == 0  # a pair without a row has float32 scores whatever the store holds
        matches[pair] = np.empty((0, 2), dtype=np.int32) if none else m.astype(np.int32)
        scores[frozenset(pair)] = np.empty((0,), dtype=np.float32) if none else np.concatenate(values[pair])
    return keypoints, matches, scores, masks


def sequential_sum(x):
    """Python's sum() over the elements of a NumPy array, which is what the reference computes: a left-to-right sum in the array's
    own precision.  np.cumsum accumulates in that order; np.sum adds pairwise and differs in the last bits."""
    x = np.asarray(x)
    return 0 if len(x) == 0 else np.cumsum(x)[-1]


class CorrespondenceGraphWrapper:
    """Whatever the object does not define is the graph's: correspondences.num_correspondences_between_images(...) and the like."""

    def __getattr__(self, name):
        if name == "cg":  # not set yet: no recursion
            raise AttributeError(name)
        return getattr(self.cg, name)


class Correspondences(BaseClass, CorrespondenceGraphWrapper):
    """Drop-in for the reference's Correspondences (mpsfm/sfm/scene/correspondences/base.py:21-139) over a CorrespondenceStore and a
    HipCorrespondenceGraph: the same attribute names (cg, keypoints_set, matches_set, sparse_im_masks, inlier_match_scores,
    _two_view_geom), method names, arguments and values.  `mpsfm_rec` is the scene: images with `name`, `imid(name)`, and, unless it
    is the reference's pycolmap-backed object, `set_keypoints(image_id, xy)`."""

    default_conf = {"matches_mode": "<--->", "cached_dense_scores": False, "verbose": 0}  # the reference's keys and defaults

    def _init(self, mpsfm_rec=None, extractor=None, sfm_outputs_dir=None, device: int = 0, backend=None):
        self.mpsfm_rec, self.extractor, self.sfm_outputs_dir = mpsfm_rec, extractor, sfm_outputs_dir  # extractor: a CorrespondenceStore
        self.cg = HipCorrespondenceGraph(device=device)
        self.keypoints_set = self.matches_set = self.sparse_im_masks = self.inlier_match_scores = None
        self._two_view_geom = {}
        self._backend = backend  # of the two-view estimator (tests inject a restatement); None: libmpsfm_hip

    def two_view_geom(self, imname1, imname2):
        """(TwoViewGeometry of the pair, True), or (None, False) for a pair that was not verified.  A pair verified under the other
        order of its names gets an inverted COPY: what is stored stays as verification left it."""
        stored = self._two_view_geom.get((imname1, imname2))
        if stored is not None:
            return stored, True
        other_way = self._two_view_geom.get((imname2, imname1))
        if other_way is None:
            return None, False
        flipped = deepcopy(other_way)
        flipped.invert()
        return flipped, True

    def matches(self, imid1, imid2):
        """[n, 2] point2D indices of the graph's correspondences between two image ids"""
        return self.cg.find_correspondences_between_images(imid1, imid2)

    def image_pairs(self):
        """The pairs (imid1 < imid2) of scene images with a correspondence, in the order in which the reference's double loop over
        mpsfm_rec.images meets them; read from the graph's pair view, not asked pair by pair."""
        order = {imid: k for k, imid in enumerate(self.mpsfm_rec.images)}
        pairs = [p for p in self.cg.image_pairs() if p[0] in order and p[1] in order]
        return sorted(pairs, key=lambda p: (order[p[0]], order[p[1]]))

    def gather_correspondences(self, pairs, ims):
        """(keypoints, matches, scores, sparse_im_masks) of the store by its matcher type; the masks are None for a sparse matcher"""
        kind = self.extractor.matcher_type
        if kind == "dense":
            return gather_dense_2view(self.extractor, pairs, ims, matches_mode=self.conf.matches_mode)
        if kind != "sparse":
            raise ValueError(f"a store's matcher_type is 'sparse' or 'dense', not {kind!r}")
        return (gather_sparse_keypoints(self.extractor, ims), *gather_sparse_matches(self.extractor, pairs), None)

    def _pair_score(self, names, inlier_mask, scores, matches):
        """the score of one verified pair with inliers (values pinned by the fixture for both settings of cached_dense_scores)"""
        if not self.conf.cached_dense_scores:
            return sequential_sum(scores[frozenset(names)][inlier_mask])
        cached = self.extractor.get_matches("cache", *names)[1]
        mode = self.conf.matches_mode
        if "dense" in mode and "sparse" in mode:  # counted only when a match of the pair starts at a dense keypoint
            starts_sparse = self.sparse_im_masks[names[0]][matches[:, 0]]
            if starts_sparse.all():
                return 0
        return sequential_sum(cached)

    def gather_matches_scores(self, inlier_masks, scores, matches_set):
        """{frozenset(pair): score} over the verified pairs: 0 for a pair without inliers, otherwise the left-to-right sum of the
        inlier matches' scores, or of the store's cached scores with cached_dense_scores"""
        return {
            frozenset(names): self._pair_score(names, inlier_masks.get(names), scores, matches_set[names]) if len(tvg.inlier_matches) else 0
            for names, tvg in self._two_view_geom.items()
        }

    def process_and_verify_matches(self):
        """Gathers the store's pairs and verifies all of them in one batched call: fills keypoints_set, matches_set, sparse_im_masks,
        _two_view_geom and inlier_match_scores."""
        pairs = [tuple(p) for p in self.extractor.pairs]
        images = set(chain.from_iterable(pairs))
        self.keypoints_set, self.matches_set, scores, self.sparse_im_masks = self.gather_correspondences(pairs, images)
        inlier_masks, self._two_view_geom = geometric_verification(
            self.mpsfm_rec, pairs, keypoints=self.keypoints_set, matches=self.matches_set, backend=self._backend, batched=True
        )
        self.inlier_match_scores = self.gather_matches_scores(inlier_masks, scores, self.matches_set)

    def _set_keypoints(self, image_id, xy):
        """The scene contract: `mpsfm_rec.set_keypoints(image_id, xy)`.  A scene without it is the reference's pycolmap-backed
        object, whose keypoints are the images' points2D."""
        setter = getattr(self.mpsfm_rec, "set_keypoints", None)
        if setter is not None:
            setter(image_id, xy)
            return
        import pycolmap

        self.mpsfm_rec.images[image_id].points2D = [pycolmap.Point2D(xy=row) for row in xy]

    def populate(self, **kwargs):
        """Verifies the store's matches and fills the graph: every scene image with its keypoints, which the scene receives rounded
        to float16 as in the reference, and the inlier matches of every gathered pair; the graph is built and finalized here."""
        self.process_and_verify_matches()
        rec = self.mpsfm_rec
        for image_id, image in rec.images.items():
            xy = self.keypoints_set[image.name]
            self._set_keypoints(image_id, xy.astype(np.float16))
            self.cg.add_image(image_id, len(xy))
        for (name0, name1), gathered in self.matches_set.items():
            if gathered is not None:
                inliers = self.two_view_geom(name0, name1)[0].inlier_matches
                self.cg.add_correspondences(rec.imid(name0), rec.imid(name1), inliers.astype(np.uint32))
        for image_id in rec.images:  # asked before finalize(): afterwards such an image no longer exists in the graph
            if self.cg.num_correspondences_for_image(image_id) == 0:
                print(f"Image {image_id} has no correspondences")
        self.cg.finalize()
        return True
