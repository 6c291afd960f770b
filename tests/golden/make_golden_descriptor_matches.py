"""Fixture for the descriptor matcher (tests/golden/reference_descriptor_matches.npz), computed BY THE REFERENCE'S OWN CODE,
loaded by file path:

  mpsfm/extraction/pairwise/models/nearest_neighbor.py     NearestNeighbor (find_nn, mutual_check)
  mpsfm/extraction/pairwise/models/utils/featuremap.py     NNs_sparse (grid_sample + NearestNeighbor)

BaseModel (which needs omegaconf) is replaced by a stub that merges the configuration and calls _forward, `.cuda()` returns
the tensor itself, torch runs on the CPU in float32.

Cases (every condition a case rests on is asserted here):
  desc0 / desc1       300 x 340 descriptors of length 128 stored as float16 (so float16, float32 and fp64 readers see the same
                      values), norm <= 1: 200 noisy copies of each other, the rest without counterpart.
  plain               mutual check only            ratio           ratio 0.8 (+ mutual check)
  ratio_distance      ratio 0.9 + distance 0.7     no_mutual       no test, no mutual check
  maps_*              NNs_sparse: 32 x 40 x 24 smooth unit maps of one scene seen with a shift, smooth confidences in
                      [0.3, 0.9], about 400 float64 keypoints per side, scores_thresh 0.85.
For every case: at least 20 % of the rows matched, at least 20 % rejected by each test the case exercises (the mutual check
counts where it is the only test: beside a ratio test it rejects almost nothing the ratio test has not), rows whose decision
margin (tests/numpy_descriptor_matches.py) is below tau32 = 4 D 2^-24 (sampled: 8 C 2^-24) are at most 1 %, outside those
rows the reference's matches equal the fp64 restatement's exactly, and the scores agree to tau32.  The file holds inputs
and outputs only.

Run in the build container:  python tests/golden/make_golden_descriptor_matches.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_reference import ROOT, load_by_path  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy_descriptor_matches as NM  # noqa: E402


class BaseModelStub:
    default_conf = {}
    required_inputs = []

    def __init__(self, conf):
        self.conf = {**self.default_conf, **dict(conf)}
        self._init(self.conf)

    def __call__(self, data):
        for key in self.required_inputs:
            assert key in data
        return self._forward(data)


def load_reference():
    stub = types.ModuleType("mpsfm.extraction.base_model")
    stub.BaseModel = BaseModelStub
    sys.modules["mpsfm.extraction.base_model"] = stub
    nn = load_by_path("mpsfm.extraction.pairwise.models.nearest_neighbor", "mpsfm/extraction/pairwise/models/nearest_neighbor.py")
    sys.modules["mpsfm.extraction.pairwise.models.nearest_neighbor"] = nn
    fm = load_by_path("ref_featuremap", "mpsfm/extraction/pairwise/models/utils/featuremap.py")
    torch.Tensor.cuda = lambda self, *a, **k: self
    return nn, fm


def rejected_fractions(d0, d1, ratio, distance, mutual, score_thr=None):
    """fractions of rows each test rejects, from the restatement's similarities"""
    sim = NM.similarities(d0, d1)
    v1, i1, v2 = NM.top2(sim)
    dist0, dist1 = 2.0 * (1.0 - v1), 2.0 * (1.0 - v2)
    out = {}
    if ratio:
        out["ratio"] = (dist0 > ratio * ratio * dist1).mean()
    if distance:
        out["distance"] = (dist0 > distance * distance).mean()
    if mutual and not ratio and not distance:  # beside another test the mutual check is not what the case is about
        fwd, _, _ = NM.match_similarities(sim, ratio, distance, False)
        both, _, _ = NM.match_similarities(sim, ratio, distance, True)
        out["mutual"] = ((fwd >= 0) & (both < 0)).mean()
    if score_thr:
        out["score"] = ((v1 + 1.0) / 2.0 < score_thr).mean()
    return out


def main():
    nn, fm = load_reference()
    rng = np.random.default_rng(20241018)
    out = {}

    n0, n1, D, m = 300, 340, 128, 200
    d1 = rng.normal(size=(n1, D))
    d1 /= np.linalg.norm(d1, axis=1, keepdims=True)
    d0 = rng.normal(size=(n0, D))
    cols = rng.permutation(n1)[:m]
    noise = rng.uniform(0.1, 0.9, m)[:, None]  # from clear matches to ones the ratio and distance tests reject
    d0[:m] = d1[cols] + noise * rng.normal(size=(m, D)) / np.sqrt(D)
    d0 /= np.linalg.norm(d0, axis=1, keepdims=True)
    perm = rng.permutation(n0)
    d0 = d0[perm]
    d0, d1 = (d0 * (1 - 2.0 ** -8)).astype(np.float16), (d1 * (1 - 2.0 ** -8)).astype(np.float16)
    assert np.linalg.norm(d0.astype(np.float64), axis=1).max() <= 1 and np.linalg.norm(d1.astype(np.float64), axis=1).max() <= 1
    out.update(desc0=d0, desc1=d1)
    t32 = NM.tau(D, NM.TAU32_EPS)
    t0, t1 = torch.from_numpy(d0.astype(np.float32).T.copy())[None], torch.from_numpy(d1.astype(np.float32).T.copy())[None]
    for case, ratio, distance, mutual in (("plain", None, None, True), ("ratio", 0.8, None, True), ("ratio_distance", 0.9, 0.7, True),
                                          ("no_mutual", None, None, False)):
        ref = nn.NearestNeighbor({"ratio_threshold": ratio, "distance_threshold": distance, "do_mutual_check": mutual})(
            {"descriptors0": t0, "descriptors1": t1})
        rm, rs = ref["matches0"][0].numpy().astype(np.int64), ref["matching_scores0"][0].numpy().astype(np.float64)
        m0, s0, margin = NM.match_descriptors(d0, d1, ratio, distance, mutual)
        sure = margin > t32
        frac = rejected_fractions(d0, d1, ratio, distance, mutual)
        print(case, "matched", (rm >= 0).mean(), "rejected", frac, "below tau32", (~sure).sum(), "score diff", np.abs(rs - s0)[sure].max())
        assert (rm >= 0).mean() >= 0.2 and all(f >= 0.2 for f in frac.values())
        assert (~sure).mean() <= 0.01
        assert np.array_equal(rm[sure], m0[sure]) and np.abs(rs - s0)[sure].max() <= t32
        out.update({f"{case}_ratio": np.array(ratio or 0.0), f"{case}_distance": np.array(distance or 0.0), f"{case}_mutual": np.array(mutual),
                    f"{case}_matches0": rm, f"{case}_scores0": rs})

    # one scene, two views: view 1 sees the scene point (x + 9.5, y - 6.25) at its pixel (x, y)
    H, W, C, shift = 32, 40, 24, np.array([9.5, -6.25])
    fx, fy, ph = rng.uniform(-0.6, 0.6, C), rng.uniform(-0.6, 0.6, C), rng.uniform(0, 2 * np.pi, C)

    def view(off):
        x, y = np.meshgrid(np.arange(W) + off[0], np.arange(H) + off[1])
        f = np.sin(fx * x[..., None] + fy * y[..., None] + ph)
        f /= np.linalg.norm(f, axis=2, keepdims=True)
        conf = 0.6 + 0.3 * np.sin(x / 7.0) * np.cos(y / 5.0)
        return (f * (1 - 2.0 ** -20)).astype(np.float32), conf.astype(np.float32)

    map0, conf0 = view(np.zeros(2))
    map1, conf1 = view(shift)
    assert conf0.min() >= 0.3 and conf0.max() <= 0.9 and conf1.min() >= 0.3 and conf1.max() <= 0.9
    assert np.linalg.norm(map0.astype(np.float64), axis=2).max() <= 1 and np.linalg.norm(map1.astype(np.float64), axis=2).max() <= 1
    nk = 400
    k0 = rng.random((nk, 2)) * [W - 1, H - 1]
    k1 = k0[:260] - shift + rng.normal(0, 0.03, (260, 2))
    k1 = k1[(k1[:, 0] > 0) & (k1[:, 0] < W - 1) & (k1[:, 1] > 0) & (k1[:, 1] < H - 1)]
    k1 = np.concatenate([k1, rng.random((nk - len(k1), 2)) * [W - 1, H - 1]])[rng.permutation(nk)]
    thr = 0.85
    rm, rs = fm.NNs_sparse(torch.from_numpy(map0), torch.from_numpy(map1), torch.from_numpy(conf0), torch.from_numpy(conf1), k0, k1, thr)
    rm, rs = np.asarray(rm, np.int64), np.asarray(rs, np.float64)
    m0, s0, margin = NM.nns_sparse(map0, map1, conf0, conf1, k0, k1, thr)
    t32s = 8.0 * C * NM.TAU32_EPS
    sure = margin > t32s
    frac = rejected_fractions(NM.sample_map(map0, k0), NM.sample_map(map1, k1), None, None, True, thr)
    print("maps matched", (rm >= 0).mean(), "rejected", frac, "below tau32", (~sure).sum(), "score diff", np.abs(rs - s0)[sure].max())
    assert (rm >= 0).mean() >= 0.2 and all(f >= 0.2 for f in frac.values())
    assert (~sure).mean() <= 0.01
    assert np.array_equal(rm[sure], m0[sure]) and np.abs(rs - s0)[sure].max() <= t32s
    out.update(maps_map0=map0, maps_map1=map1, maps_conf0=conf0, maps_conf1=conf1, maps_kps0=k0, maps_kps1=k1, maps_scores_thresh=np.array(thr),
               maps_matches0=rm, maps_scores0=rs)

    path = os.path.join(HERE, "reference_descriptor_matches.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: (v.shape, str(v.dtype)) for k, v in out.items()})
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
