"""``pycolmap.CorrespondenceGraph``-shaped graph built by one call of ``mpsfm_corr_graph_build``.

The reference fills a ``pycolmap.CorrespondenceGraph`` pair by pair (mpsfm/sfm/scene/correspondences/base.py:117-139) and the
mapper reads it through ``num_correspondences_between_images``, ``find_correspondences_between_images`` and the triangulator.
``HipCorrespondenceGraph`` has the same method names and return values.  ``add_image`` / ``add_correspondences`` only collect on the
host; the graph of all pairs is built on the GPU in one call, at the first query or at ``finalize()``, and a later ``add_*``
discards that build.  The rule is COLMAP 3.11's AddCorrespondences + Finalize as a set rule (include/mpsfm_hip.h): self pairs,
invalid indices and duplicates are refused and counted (``rejected()``), a keypoint may keep several partners in one image, and
images without correspondences stop existing at ``finalize()``.
"""

from __future__ import annotations

from collections import namedtuple

import numpy as np

from ... import capi

MAX_NUM_IMAGES = 2147483647  # COLMAP's kMaxNumImages: pair_id = kMaxNumImages * min(id1, id2) + max(id1, id2)

Correspondence = namedtuple("Correspondence", ["image_id", "point2D_idx"])


def image_pair_to_pair_id(image_id1: int, image_id2: int) -> int:
    a, b = (int(image_id1), int(image_id2)) if image_id1 <= image_id2 else (int(image_id2), int(image_id1))
    return MAX_NUM_IMAGES * a + b


def pair_id_to_image_pair(pair_id: int):
    return int(pair_id) // MAX_NUM_IMAGES, int(pair_id) % MAX_NUM_IMAGES


class HipCorrespondenceGraph:
    def __init__(self, device: int = 0):
        self.device = device
        self._num_kp = {}   # image id -> number of keypoints, as added
        self._lists = []    # (image id 1, image id 2, int32 [n, 2]) in the order of the calls
        self._g = None      # the build
        self._finalized = False

    # -- collecting ----------------------------------------------------------------------------------------------------------
    def _open(self):
        if self._finalized:
            raise RuntimeError("the correspondence graph is finalized: nothing can be added")
        self._g = None

    def add_image(self, image_id, num_points2D):
        self._open()
        if int(image_id) in self._num_kp:
            raise ValueError(f"image {image_id} was added before")
        if int(num_points2D) < 0:
            raise ValueError("negative number of keypoints")
        self._num_kp[int(image_id)] = int(num_points2D)

    def add_correspondences(self, image_id1, image_id2, matches):
        self._open()
        a, b = int(image_id1), int(image_id2)
        if a not in self._num_kp or b not in self._num_kp:
            raise KeyError(f"add_image comes before add_correspondences: {a if a not in self._num_kp else b}")
        m = np.asarray(matches).reshape(-1, 2).astype(np.int64)
        m = np.where((m < 0) | (m > np.iinfo(np.int32).max), -1, m).astype(np.int32)  # out of every range: an invalid index
        self._lists.append((a, b, np.ascontiguousarray(m)))

    def finalize(self):
        self._build()
        self._finalized = True

    # -- the build -----------------------------------------------------------------------------------------------------------
    def _build(self):
        if self._g is not None:
            return self._g
        ids = sorted(self._num_kp)
        index = {imid: i for i, imid in enumerate(ids)}
        kp_start = np.concatenate([[0], np.cumsum([self._num_kp[i] for i in ids], dtype=np.int64)]).astype(np.int64)
        li0 = np.array([index[a] for a, _, _ in self._lists], np.int32)
        li1 = np.array([index[b] for _, b, _ in self._lists], np.int32)
        lstart = np.concatenate([[0], np.cumsum([len(m) for _, _, m in self._lists], dtype=np.int64)]).astype(np.int64)
        matches = np.concatenate([m for _, _, m in self._lists]) if self._lists else np.zeros((0, 2), np.int32)
        g = capi.corr_graph_build(kp_start, li0, li1, lstart, matches, device=self.device)
        g.update(image_ids=ids, index=index, kp_start=kp_start, list_start=lstart, ids_arr=np.asarray(ids, np.int64),
                 pair_index={(int(a), int(b)): p for p, (a, b) in enumerate(zip(g["pair_image0"], g["pair_image1"]))})
        self._g = g
        return g

    def _image(self, image_id):
        g = self._build()
        i = g["index"].get(int(image_id))
        if i is None or (self._finalized and g["image_num_correspondences"][i] == 0):
            raise KeyError(f"image {image_id} does not exist in the correspondence graph")
        return g, i

    def _keypoint(self, image_id, point2D_idx):
        g, i = self._image(image_id)
        if not 0 <= int(point2D_idx) < self._num_kp[int(image_id)]:
            raise IndexError(f"image {image_id} has no keypoint {point2D_idx}")
        return g, int(g["kp_start"][i]) + int(point2D_idx)

    def _pair(self, image_id1, image_id2):
        g = self._build()
        i, j = g["index"].get(int(image_id1)), g["index"].get(int(image_id2))
        if i is None or j is None:
            return g, None, False
        return g, g["pair_index"].get((min(i, j), max(i, j))), i > j

    # -- pycolmap.CorrespondenceGraph's methods ----------------------------------------------------------------------------------
    def exists_image(self, image_id):
        g = self._build()
        i = g["index"].get(int(image_id))
        return i is not None and not (self._finalized and g["image_num_correspondences"][i] == 0)

    def num_images(self):
        g = self._build()
        return int((g["image_num_correspondences"] > 0).sum()) if self._finalized else len(g["image_ids"])

    def num_image_pairs(self):
        return len(self._build()["pair_image0"])

    def num_correspondences_for_image(self, image_id):
        g, i = self._image(image_id)
        return int(g["image_num_correspondences"][i])

    def num_observations_for_image(self, image_id):
        g, i = self._image(image_id)
        return int(g["image_num_observations"][i])

    def num_correspondences_between_images(self, image_id1, image_id2):
        g, p, _ = self._pair(image_id1, image_id2)
        return 0 if p is None else int(g["pair_start"][p + 1] - g["pair_start"][p])

    def num_correspondences_between_all_images(self):
        g = self._build()
        ids, n = g["image_ids"], np.diff(g["pair_start"])
        return {image_pair_to_pair_id(ids[a], ids[b]): int(c) for a, b, c in zip(g["pair_image0"], g["pair_image1"], n)}

    def find_correspondences_between_images(self, image_id1, image_id2):
        """uint32 [n, 2]: (point2D index in image_id1, point2D index in image_id2), ascending by the indices in the lower image id"""
        g, p, swapped = self._pair(image_id1, image_id2)
        if p is None:
            return np.zeros((0, 2), np.uint32)
        m = g["pair_matches"][g["pair_start"][p]:g["pair_start"][p + 1]].astype(np.uint32)
        return np.ascontiguousarray(m[:, ::-1]) if swapped else m

    def has_correspondences(self, image_id, point2D_idx):
        g, k = self._keypoint(image_id, point2D_idx)
        return bool(g["corr_start"][k + 1] > g["corr_start"][k])

    def is_two_view_observation(self, image_id, point2D_idx):
        g, k = self._keypoint(image_id, point2D_idx)
        return bool(g["kp_two_view"][k])

    def extract_correspondences(self, image_id, point2D_idx):
        g, k = self._keypoint(image_id, point2D_idx)
        kps = g["corr_kp"][g["corr_start"][k]:g["corr_start"][k + 1]]
        im = np.searchsorted(g["kp_start"], kps, side="right") - 1  # images without keypoints share their start: the last one holds it
        return [Correspondence(int(a), int(b)) for a, b in zip(g["ids_arr"][im], kps - g["kp_start"][im])]

    # -- what the track engine and the caller read beyond pycolmap's methods -----------------------------------------------------
    def image_pairs(self):
        """[(image_id1, image_id2)] with image_id1 < image_id2 of every pair with a correspondence, ascending"""
        g = self._build()
        ids = g["image_ids"]
        return [(ids[a], ids[b]) for a, b in zip(g["pair_image0"], g["pair_image1"])]

    def csr(self):
        """The graph as the arrays of `mpsfm_tri_graph`, images in the order of ascending image id (every added image, also after
        finalize(): an image without correspondences has empty rows)."""
        g = self._build()
        return dict(image_ids=list(g["image_ids"]), kp_start=g["kp_start"], corr_start=g["corr_start"], corr_kp=g["corr_kp"])

    def match_status(self):
        """uint8 per match, one array per add_correspondences call in the order of the calls: 0 added, 1 invalid, 2 self pair,
        3 duplicate"""
        g = self._build()
        return [g["match_status"][a:b] for a, b in zip(g["list_start"][:-1], g["list_start"][1:])]

    def rejected(self):
        """{"invalid": n, "self_pair": n, "duplicate": n} over everything that was added"""
        n = np.bincount(self._build()["match_status"], minlength=4)
        return {name: int(n[s]) for s, name in enumerate(capi.CORR_STATUS) if s > 0}
