"""Pairs of neighbours in an image sequence (reference: mpsfm/extraction/pairs/base.py), host only; and what the three pair
stages share: reading a list of names and writing the pairs file."""

from __future__ import annotations

from collections.abc import Iterable
from pathlib import Path

from ...utils.parsers import parse_image_lists


def names_of(image_list, features, what="image list"):
    """The names a stage works on: a list file (str / Path, may be a glob pattern), any iterable of names, or else the keys of the
    feature mapping."""
    if image_list is not None:
        if isinstance(image_list, (str, Path)):
            return parse_image_lists(image_list)
        if isinstance(image_list, Iterable):
            return list(image_list)
        raise ValueError(f"Unknown type for {what}: {image_list}")
    if features is not None:
        return list(features.keys())
    raise ValueError("Provide either a list of images or a feature mapping.")


def write_pairs(output, pairs):
    """`name0 name1` per line, no trailing newline: the reference's format.  output None: nothing is written."""
    if output is not None:
        with open(output, "w", encoding="utf-8") as f:
            f.write("\n".join(f"{a} {b}" for a, b in pairs))


def pairs_from_sequential(output, image_list=None, features=None, overlap=3, quadratic_overlap=True):
    """Image i with its next `overlap` images and, with `quadratic_overlap`, with the images 2^d ahead for every d <= overlap whose
    2^d exceeds `overlap`.  Returns the pairs, each ordered by name and the list sorted, as written to `output`."""
    names = names_of(image_list, features)
    n = len(names)
    pairs = []
    for i in range(n - 1):
        for d in range(1, min(overlap, n - 1 - i) + 1):
            pairs.append((names[i], names[i + d]))
            jump = 2 ** d
            if quadratic_overlap and jump > overlap and i + jump < n:
                pairs.append((names[i], names[i + jump]))
    pairs = sorted((min(a, b), max(a, b)) for a, b in pairs)
    write_pairs(output, pairs)
    return pairs
