"""Text files of image names and image pairs (reference: mpsfm/utils/parsers.py, adapted from hloc): one pair per line,
`name0 name1`, as the pair stages of mpsfm_amd/extraction/pairs write them."""

from __future__ import annotations

from pathlib import Path


def parse_image_list(path):
    """The names of an image list: the first word of every line that is neither empty nor a `#` comment.  (The reference's
    `with_intrinsics` branch builds pycolmap cameras and is not restated.)"""
    names = []
    with open(path) as f:
        for line in f:
            line = line.strip("\n")
            if line and line[0] != "#":
                names.append(line.split()[0])
    if not names:
        raise ValueError(f"no image name in {path}")
    return names


def parse_image_lists(paths):
    """`paths` is a path whose last component may be a glob pattern: the names of all files it matches, concatenated."""
    paths = Path(paths)
    files = sorted(paths.parent.glob(paths.name))
    if not files:
        raise ValueError(f"no image list matches {paths}")
    names = []
    for file in files:
        names += parse_image_list(file)
    return names


def parse_retrieval(path):
    """{query name: [db names in the order of the file]}; blank lines are skipped."""
    retrieval = {}
    with open(path) as f:
        for line in f.read().rstrip("\n").split("\n"):
            if not line:
                continue
            q, r = line.split()
            retrieval.setdefault(q, []).append(r)
    return retrieval


def read_unique_pairs(path):
    """The pairs of a pairs file as sorted two-element lists, each unordered pair once: `a b` and `b a` are one pair.  Blank
    lines are skipped.

    The result is in order of first appearance.  The reference returns the elements of a Python `set` of frozensets, whose
    order is arbitrary and changes from run to run with string hashing; the set of pairs is the same."""
    seen, pairs = set(), []
    with open(path) as f:
        for line in f:
            names = line.split()
            if not names:
                continue
            key = frozenset(names)
            if key not in seen:
                seen.add(key)
                pairs.append(sorted(key))
    return pairs
