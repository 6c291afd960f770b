"""From a dense matcher's warp and certainty to match lists, with the reference's names and signatures
(mpsfm/extraction/pairwise/models/utils/warp.py ``simple_nms``, ``kpids_to_matches0``, ``assign_keypoints`` and the post-network
half of models/roma.py ``Roma._forward`` as ``warp_to_matches``).

The reference runs five ``max_pool2d`` passes, copies the whole warp to the host, queries two SciPy KD-trees with every row and
groups the rows in a Python loop.  Here each function is one call into libmpsfm_hip (csrc/warp_matches.hip), and device
tensors stay on the device.  All decisions are exact.

Ties.  Among equal scores the reference's ``get_unique_matches`` keeps whichever row an unstable ``np.argsort`` happens to put
first; here the LOWEST ROW wins (-0.0 counts as +0.0).

``to_pixel_coordinates`` is RoMa's (third-party, not part of the reference tree): ``W / 2 * (x + 1)`` in float32, taken as the
contract.
"""

from __future__ import annotations

import numpy as np

from ... import capi
from .utils import _np, assign_keypoints

__all__ = ["assign_keypoints", "kpids_to_matches0", "simple_nms", "to_pixel_coordinates", "warp_to_matches"]


def simple_nms(scores, nms_radius: int):
    """Non-maximum suppression of a 2-D score map over (2 r + 1)^2 windows, two rounds of recovery: bitwise the reference's.  A
    tensor gives a float32 tensor on the same device, an ndarray a float32 ndarray."""
    assert nms_radius >= 0
    if hasattr(scores, "detach"):
        import torch

        assert scores.dim() == 2
        if scores.is_cuda:
            return capi.simple_nms_map(scores.detach(), nms_radius)
        return torch.from_numpy(capi.simple_nms_map(scores.detach().numpy(), nms_radius))
    scores = np.asarray(scores)
    assert scores.ndim == 2
    return capi.simple_nms_map(scores, nms_radius)


def kpids_to_matches0(kpt_ids0, kpt_ids1, scores):
    """Rows (id0, id1, score) with both ids != -1, reduced to one-to-one matches: a row stays when it has the highest score of
    its id0 group and of its id1 group.  Returns ``(matches0 int32, scores0 float16)`` of length 1 + the largest matched id0, as
    the reference does; two empty arrays when nothing is valid."""
    m, s = capi.kpids_to_matches0_arrays(_np(kpt_ids0), _np(kpt_ids1), _np(scores))
    return m, s.astype(np.float16)


def to_pixel_coordinates(warp, H_A, W_A, H_B, W_B):
    """(kpts_A, kpts_B) in pixels from normalised [..., 4] coordinates, float32 with every operation rounded on its own."""
    if hasattr(warp, "detach"):
        import torch

        a, b = warp[..., :2], warp[..., 2:]
        return (torch.stack((W_A / 2 * (a[..., 0] + 1), H_A / 2 * (a[..., 1] + 1)), dim=-1),
                torch.stack((W_B / 2 * (b[..., 0] + 1), H_B / 2 * (b[..., 1] + 1)), dim=-1))
    w = np.asarray(warp, np.float32)
    one = np.float32(1)
    f = [np.float32(v / 2) for v in (W_A, H_A, W_B, H_B)]
    return (np.stack((f[0] * (w[..., 0] + one), f[1] * (w[..., 1] + one)), axis=-1),
            np.stack((f[2] * (w[..., 2] + one), f[3] * (w[..., 3] + one)), axis=-1))


def warp_to_matches(warp, certainty, sizes, mode="sparse", skpts0=None, skpts1=None, scale0=(1, 1), scale1=(1, 1), nms_radius=8,
                    sample_thresh=0.1, max_error=2):
    """The ``pred`` dict of ``Roma._forward`` from the network's ``warp`` [H, W, 4] and ``certainty`` [H, W] (tensors on any
    device, or arrays), ``sizes = (H_A, W_A, H_B, W_B)``.  ``"dense" in mode``: dkeypoints0, dkeypoints1, dscores (what
    ``thin_dense_matches`` takes next); ``"sparse" in mode``: smatches0, smatching_scores0 against the sparse keypoints
    ``skpts0`` / ``skpts1`` (pixels; the warp's pixel coordinates are multiplied by ``scale0`` / ``scale1`` first).  The defaults
    are the reference's ``default_conf``."""
    bits = (capi.WARP_DENSE if "dense" in mode else 0) | (capi.WARP_SPARSE if "sparse" in mode else 0)
    if not bits:
        return {}
    if bits & capi.WARP_SPARSE and (skpts0 is None or skpts1 is None):
        raise ValueError("the sparse leg needs skpts0 and skpts1")
    if hasattr(warp, "detach"):
        warp, certainty = warp.detach(), certainty.detach()
    pred = capi.warp_matches(warp, certainty, sizes, bits, _np(skpts0), _np(skpts1), _np(scale0), _np(scale1), nms_radius, sample_thresh,
                             max_error)
    if "smatching_scores0" in pred:
        pred["smatching_scores0"] = pred["smatching_scores0"].astype(np.float16)
    return pred
