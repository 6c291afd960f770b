"""All pairs (reference: mpsfm/extraction/pairs/hloc/pairs_from_exhaustive.py), host only."""

from __future__ import annotations

from .base import names_of, write_pairs


def main(output, image_list=None, features=None, ref_list=None, ref_features=None):
    """Every query image with every reference image; without references, every unordered pair of query images once, (i, j) with
    i < j in list order.  Returns the pairs as written to `output`."""
    names_q = names_of(image_list, features)
    if ref_list is not None or ref_features is not None:
        names_ref = names_of(ref_list, ref_features, "reference image list")
        pairs = [(a, b) for a in names_q for b in names_ref]
    else:
        pairs = [(a, b) for i, a in enumerate(names_q) for b in names_q[i + 1:]]
    write_pairs(output, pairs)
    return pairs
