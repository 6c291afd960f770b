"""Fixture for the dense reciprocal matcher (tests/golden/reference_reciprocal_matches.npz).  `merge_corres` and
`extract_correspondences` are taken out of the reference's mpsfm/extraction/pairwise/models/mast3r.py by AST (the module's own
imports, MASt3R among them, cannot be satisfied) and run BY THE REFERENCE'S OWN CODE on CPU torch tensors;
`fast_reciprocal_NNs`, which is MASt3R's and not part of the reference tree, is the fp64 restatement
(tests/numpy_reciprocal_matches.py).

Cases: maps of one scene seen with a shift of (9.5, -6.25) pixels, plus noise, float32, C = 24, rows of norm < 1; smooth
confidences in [0.3, 0.9]; the two decoder passes differ in noise and confidences.
  small   37 x 45 against 40 x 48, subsample 2          large   72 x 80 against 72 x 80, subsample 8
Asserted here: every seed of every search is decided (gap above tau64 = 4 C 2^-53 on its whole trajectory); at least 5 % of
the converged seeds collapse onto a pair another seed also found (in the small case and over both); a pair occurs in both halves with different confidences;
a seed needs three iterations.

The four maps of the two cases are 725 000 float32 values, which no lossless coding brings under the 1 MiB a committed file
may have, let alone under 200 KB: the file stores the cases' PARAMETERS and the SHA-256 of the maps and confidences that
numpy_reciprocal_matches.fixture_inputs builds from them (integer hashes and correctly rounded IEEE operations only, so every
machine builds the same bits: the test compares the digests first), and the three outputs.  Data only.

Run in the build container:  python tests/golden/make_golden_reciprocal_matches.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_reference import ROOT, extract_functions  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy_reciprocal_matches as NR  # noqa: E402

RUNS = []


def fast_reciprocal_NNs(A, B, subsample_or_initxy1=8, ret_xy=True, device="cpu", dist="dot", block_size=None, **kw):
    assert not ret_xy and dist == "dot" and not kw
    r = NR.fast_reciprocal_nns(A.numpy(), B.numpy(), int(subsample_or_initxy1), 10)
    RUNS.append(r)
    return r["idx1"], r["idx2"]


def main():
    ns = extract_functions("mpsfm/extraction/pairwise/models/mast3r.py", ("merge_corres", "extract_correspondences"))
    ns.update(device="cpu", fast_reciprocal_NNs=fast_reciprocal_NNs)
    out, total = {}, [0, 0]
    for name in NR.FIXTURE_CASES:
        feats, qonfs, S = NR.fixture_inputs(name)
        C = feats[0].shape[2]
        for f in feats:
            assert f.dtype == np.float32 and np.linalg.norm(f.astype(np.float64), axis=2).max() < 1
        for q in qonfs:
            assert q.dtype == np.float32 and q.min() >= 0.3 and q.max() <= 0.9
        del RUNS[:]
        xy1, xy2, scores = ns["extract_correspondences"]([torch.from_numpy(f) for f in feats], [torch.from_numpy(q) for q in qonfs], subsample=S)
        assert xy1.dtype == np.int64 and xy2.dtype == np.int64 and scores.dtype == np.float32 and len(RUNS) == 4
        # the restatement's own extract_correspondences says the same
        rx1, rx2, rs = NR.extract_correspondences(feats, qonfs, S)
        assert np.array_equal(rx1, xy1) and np.array_equal(rx2, xy2) and np.array_equal(rs, scores)
        gaps = np.concatenate([r["gap"] for r in RUNS])
        conv = sum(r["n_converged"] for r in RUNS)
        uniq = sum(len(r["idx1"]) for r in RUNS)
        its = np.concatenate([r["iters_of_seed"][r["converged"]] for r in RUNS])
        print(name, "seeds", [r["n_seeds"] for r in RUNS], "converged", [r["n_converged"] for r in RUNS], "unique", [len(r["idx1"]) for r in RUNS],
              "iterations", np.bincount(its), "min gap", gaps.min(), "tau64", NR.tau64(C), "rows", len(xy1))
        assert gaps.min() > NR.tau64(C)  # every seed is decided
        # seeds that collapse onto a pair another seed found: where the seeds are 2 pixels apart, and over both cases (at 8 pixels a
        # seed's neighbour lies outside its basin: the large case alone has none)
        total[0] += conv
        total[1] += uniq
        assert conv - uniq >= 0.05 * conv or S > 2
        assert its.max() >= 3
        # a pair found in both halves with different confidences: the first occurrence decides
        halves = []
        for h, (QA, QB) in enumerate(((qonfs[0], qonfs[1]), (qonfs[3], qonfs[2]))):
            f, b = RUNS[2 * h], RUNS[2 * h + 1]
            i1, i2 = np.r_[f["idx1"], b["idx2"]].astype(np.int64), np.r_[f["idx2"], b["idx1"]].astype(np.int64)
            halves.append({(a, c): (QA.ravel()[a], QB.ravel()[c]) for a, c in zip(i1.tolist(), i2.tolist())})
        both = [k for k in halves[0] if k in halves[1] and halves[0][k] != halves[1][k]]
        print(name, "pairs in both halves with different confidences", len(both))
        assert both
        out.update({f"{name}_digest": np.array(NR.digest(*feats, *qonfs)), f"{name}_case": np.array(NR.FIXTURE_CASES[name][0:1] + NR.FIXTURE_CASES[name][1]
                    + NR.FIXTURE_CASES[name][2] + NR.FIXTURE_CASES[name][3:5] + NR.FIXTURE_CASES[name][5], np.int64),
                    f"{name}_xy1": xy1, f"{name}_xy2": xy2, f"{name}_scores": scores})
        for s, r in enumerate(RUNS):
            out.update({f"{name}_search{s}_idx1": r["idx1"], f"{name}_search{s}_idx2": r["idx2"],
                        f"{name}_search{s}_stats": np.array([r["n_seeds"], r["n_converged"], r["iterations"], r["nn_queries"]], np.int64)})
    assert total[0] - total[1] >= 0.05 * total[0]
    path = os.path.join(HERE, "reference_reciprocal_matches.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: (v.shape, str(v.dtype)) for k, v in out.items()})
    assert os.path.getsize(path) < 200000


if __name__ == "__main__":
    main()
