"""tests/golden/reference_correspondences.npz: what the reference's own gather functions and score sums give on a small in-memory
data set (4 images, 5 pairs, one of them without a match, one stored under the other order of its names), for the three modes
sparse, dense and sparse+dense.

Loaded from /root/reference by AST extraction, as tests/golden/make_golden_reference.py does (this script only; nothing of the
reference travels, the fixture holds inputs and outputs, no source text):
  mpsfm/sfm/scene/correspondences/utils.py   gather_sparse_keypoints, gather_sparse_matches, gather_dense_2view
  mpsfm/sfm/scene/correspondences/base.py    Correspondences.gather_matches_scores
Their module-level readers of the extractor's HDF5 files (get_keypoints, get_matches, get_dense_2view_keypoints) are replaced by
stubs that hand out copies of the arrays below, a pair under either order of its names (read the other way round: columns swapped,
as the reference's find_pair has it).

Run in the build container:  python tests/golden/make_golden_correspondences.py
"""
import json
import os
from collections import defaultdict
from types import SimpleNamespace

import numpy as np

from make_golden_reference import extract_functions

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ["a.jpg", "b.jpg", "dir/c.jpg", "d.jpg"]
PAIRS = [("a.jpg", "b.jpg"), ("a.jpg", "dir/c.jpg"), ("b.jpg", "dir/c.jpg"), ("dir/c.jpg", "d.jpg"), ("a.jpg", "d.jpg")]
STORED = [("b.jpg", "a.jpg"), ("a.jpg", "dir/c.jpg"), ("b.jpg", "dir/c.jpg"), ("dir/c.jpg", "d.jpg"), ("a.jpg", "d.jpg")]  # pair 0 the other way
EMPTY = 4  # the pair without a match
MODES = {"sparse": ("sparse", "sparse"), "dense": ("dense", "dense"), "sparse+dense": ("dense", "sparse+dense")}  # matcher type, matches_mode


def make_inputs(rng):
    inp = {}
    nkp = {}
    for name in NAMES:
        nkp[name] = int(rng.integers(6, 11))
        inp[f"skp/{name}"] = (rng.uniform(0, 640, (nkp[name], 2)).astype(np.float16)).astype(np.float32)  # what hloc stores, read as float32
    for k, (n0, n1) in enumerate(STORED):
        n = 0 if k == EMPTY else int(rng.integers(3, min(nkp[n0], nkp[n1])))
        inp[f"sm/{k}"] = np.stack([rng.permutation(nkp[n0])[:n], rng.permutation(nkp[n1])[:n]], -1).astype(np.int64).reshape(-1, 2)
        inp[f"ss/{k}"] = rng.uniform(0.1, 1, n).astype(np.float16)
        nd = 0 if k == EMPTY else int(rng.integers(4, 9))
        inp[f"dk0/{k}"] = rng.uniform(0, 640, (nd, 2)).astype(np.float32)
        inp[f"dk1/{k}"] = rng.uniform(0, 640, (nd, 2)).astype(np.float32)
        extra = 0 if k == EMPTY else 2  # rows behind the keypoints: the reference cuts them off
        inp[f"dm/{k}"] = np.stack([np.arange(nd + extra), np.arange(nd + extra)], -1).astype(np.int64).reshape(-1, 2)
        inp[f"ds/{k}"] = rng.uniform(0.1, 1, nd).astype(np.float16)
        inp[f"cs/{k}"] = rng.uniform(0.1, 1, max(nd - 1, 0)).astype(np.float32)  # the cached dense scores
    return inp


def stubs(inp):
    def lookup(prefix, name0, name1):
        if (name0, name1) in STORED:
            return inp[f"{prefix}/{STORED.index((name0, name1))}"], False
        return inp[f"{prefix}/{STORED.index((name1, name0))}"], True

    def get_keypoints(path, name):
        assert path == "sfeats"
        return np.array(inp[f"skp/{name}"])

    def get_matches(path, name0, name1):
        m, reverse = lookup({"smatches": "sm", "dmatches": "dm", "cache_matches": "dm"}[path], name0, name1)
        s, _ = lookup({"smatches": "ss", "dmatches": "ds", "cache_matches": "cs"}[path], name0, name1)
        return (np.flip(np.array(m), -1) if reverse else np.array(m)), np.array(s)

    def get_dense_2view_keypoints(path, name0, name1):
        assert path == "dfeats"
        k0, reverse = lookup("dk0", name0, name1)
        k1, _ = lookup("dk1", name0, name1)
        return (np.array(k1), np.array(k0)) if reverse else (np.array(k0), np.array(k1))

    return dict(get_keypoints=get_keypoints, get_matches=get_matches, get_dense_2view_keypoints=get_dense_2view_keypoints)


def main():
    rng = np.random.default_rng(20)
    inp = make_inputs(rng)
    out = {f"in/{k}": v for k, v in inp.items()}
    rel = "mpsfm/sfm/scene/correspondences/"
    ns = extract_functions(rel + "utils.py", ("gather_sparse_keypoints", "gather_sparse_matches", "gather_dense_2view"))
    ns.update(stubs(inp), defaultdict=defaultdict)
    base = extract_functions(rel + "base.py", cls="Correspondences", method_names=("gather_matches_scores",))
    base.update(stubs(inp))
    extractor = SimpleNamespace(match_dirs={k: k for k in ("sfeats", "smatches", "dfeats", "dmatches", "cache_matches")})
    ims = set(NAMES)
    for mode, (matcher, matches_mode) in MODES.items():
        if matcher == "sparse":
            kps = ns["gather_sparse_keypoints"](extractor, ims)
            matches, scores = ns["gather_sparse_matches"](extractor, PAIRS)
            masks = None
        else:
            kps, matches, scores, masks = ns["gather_dense_2view"](extractor, PAIRS, ims, matches_mode=matches_mode)
        for name in NAMES:
            out[f"{mode}/kp/{name}"] = kps[name]
            if masks is not None:
                out[f"{mode}/mask/{name}"] = masks[name]
        tvgs, inlier = {}, {}
        for k, pair in enumerate(PAIRS):
            out[f"{mode}/m/{k}"] = matches[pair]
            out[f"{mode}/s/{k}"] = scores[frozenset(pair)]
            inl = rng.uniform(size=len(matches[pair])) < 0.7
            if k == 2:
                inl[:] = False  # a pair whose verification keeps nothing
            out[f"{mode}/inl/{k}"] = inl
            inlier[pair] = inl
            tvgs[pair] = SimpleNamespace(inlier_matches=matches[pair][inl])
        for cached in (False, True):
            if cached and matcher == "sparse":
                continue
            me = SimpleNamespace(_two_view_geom=tvgs, conf=SimpleNamespace(cached_dense_scores=cached, matches_mode=matches_mode),
                                 extractor=extractor, sparse_im_masks=masks)
            sums = base["Correspondences"].gather_matches_scores(me, inlier, scores, matches)
            for k, pair in enumerate(PAIRS):
                out[f"{mode}/sum{int(cached)}/{k}"] = np.asarray(sums[frozenset(pair)])
    out["meta"] = np.array(json.dumps(dict(names=NAMES, pairs=PAIRS, stored=STORED, empty=EMPTY, modes={k: list(v) for k, v in MODES.items()})))
    path = os.path.join(HERE, "reference_correspondences.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
