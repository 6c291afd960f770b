"""Mutual nearest-neighbour descriptor matching with the reference's names (mpsfm/extraction/pairwise/models/
nearest_neighbor.py ``NearestNeighbor``), one call into libmpsfm_hip per pair (csrc/descriptor_matches.hip).

The reference forms the full ``n0 x n1`` float32 similarity matrix, a transposed copy and two ``topk`` passes.  Here the
similarities are fp64 dot products formed tile by tile on the matrix pipe and only a running top-2 per row is kept.  Equal
similarities go to the LOWEST index (in the reference that is an accident of the torch build); everything else is the
reference's ``find_nn`` / ``mutual_check`` in fp64.
"""

from __future__ import annotations

import numpy as np

from ... import capi


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _is_float64(x) -> bool:
    if _is_torch(x):
        import torch

        return x.dtype == torch.float64
    return np.dtype(x.dtype) == np.float64


def match_descriptors(desc0, desc1, ratio_threshold=None, distance_threshold=None, do_mutual_check=True):
    """desc0 ``[n0, dim]``, desc1 ``[n1, dim]`` (float16 / float32; NumPy, host or device tensors) -> ``matches0`` int64
    ``[n0]`` (-1: no match) and ``matching_scores0`` float64 ``[n0]``, NumPy.  A device tensor goes in as a device pointer."""
    return capi.match_descriptors(desc0, desc1, ratio_threshold, distance_threshold, do_mutual_check)


class NearestNeighbor:
    default_conf = {
        "ratio_threshold": None,
        "distance_threshold": None,
        "do_mutual_check": True,
        "require_download": False,
    }
    required_inputs = ["descriptors0", "descriptors1"]

    def __init__(self, conf=None):
        self.conf = {**self.default_conf, **dict(conf or {})}

    # a reference-style loader calls .eval().to(device) on what it builds: there is nothing to switch or to move
    def eval(self):
        return self

    def to(self, *args, **kwargs):
        return self

    def __call__(self, data):
        for key in self.required_inputs:
            assert key in data, f"Missing key {key} in data"
        d0, d1 = data["descriptors0"], data["descriptors1"]
        if d0.ndim != 3 or d1.ndim != 3 or d0.shape[0] != d1.shape[0] or d0.shape[1] != d1.shape[1]:
            raise ValueError("descriptors must be (b, D, N) and (b, D, M)")
        for d in (d0, d1):
            if _is_float64(d):
                raise TypeError("float64 descriptors are not supported: float16 and float32 are widened exactly")
        b, n0 = int(d0.shape[0]), int(d0.shape[2])
        matches, scores = np.full((b, n0), -1, np.int64), np.zeros((b, n0))
        for i in range(b):
            a = d0[i].T if not _is_torch(d0) else d0[i].transpose(0, 1)
            c = d1[i].T if not _is_torch(d1) else d1[i].transpose(0, 1)
            matches[i], scores[i] = match_descriptors(a, c, self.conf["ratio_threshold"], self.conf["distance_threshold"],
                                                      self.conf["do_mutual_check"])
        if _is_torch(d0):
            import torch

            return {"matches0": torch.from_numpy(matches).to(d0.device), "matching_scores0": torch.from_numpy(scores).to(d0.device)}
        return {"matches0": matches, "matching_scores0": scores}
