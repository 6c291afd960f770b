"""tests/golden/reference_image_selection.npz: what the reference's own ImageSelection chooses on a stub scene, for all eight
image_selection_methods, and the order of its find_init_pairs.

Loaded from the reference tree by AST extraction, as tests/golden/make_golden_correspondences.py does (this script only; nothing of
the reference travels, the fixture holds inputs and outputs, no source text):
  mpsfm/sfm/mapper/image_selection.py          every method of ImageSelection (its base class is cut off: conf is set by hand)
  mpsfm/sfm/scene/reconstruction/base.py       MpsfmReconstruction.filtered_image_pairs
The stub scene (7 images, 3 of them registered) is tables: per-image visibility statistics, correspondences per pair, verified
two-view geometries with inlier counts, triangulation angles and configs 2 .. 4, matcher-score sums, one ignore_matches_AP mask.
Every method's scores over the candidates are DISTINCT, and so are the inlier counts within a config: the reference orders equal
scores by an unstable argsort and pairs by set iteration, which no fixture can pin.  stub_scene() is shared with
tests/test_image_selection_cpu.py, which rebuilds the scene from the fixture's tables.

Run in the build container:  python tests/golden/make_golden_image_selection.py
"""
import ast
import json
import os
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
METHODS = ["MAX_VISIBLE_POINTS_NUM", "MAX_VISIBLE_POINTS_RATIO", "MIN_UNCERTAINTY", "MAX_NUM_CORRESPONDENCES", "MAX_NUM_INLIER_CORRESPONDENCES",
           "MAX_NUM_INLIER_CORRESPONDENCES_TOT", "MAX_NUM_INLIER_SCORES_TOT", "MAX_MATCHER_INLIER_SCORES"]
IMAGE_IDS = [3, 5, 8, 11, 12, 14, 17]
REGISTERED = [5, 11, 14]
EXCLUDE = [(5, 3), (11, 14)]  # the second run of find_init_pairs; the first pair is given the other way round


def make_tables(rng):
    n = len(IMAGE_IDS)
    t = {}
    t["num_visible"] = rng.permutation(np.arange(40, 40 + 7 * n, 7))[:n].astype(np.int64)
    t["num_observations"] = (t["num_visible"] + rng.permutation(np.arange(5, 5 + 11 * n, 11))[:n]).astype(np.int64)
    t["visibility_score"] = rng.permutation(np.arange(900, 900 + 131 * n, 131))[:n].astype(np.int64)
    pairs = [(a, b) for i, a in enumerate(IMAGE_IDS) for b in IMAGE_IDS[i + 1:]]
    t["pairs"] = np.array(pairs, np.int64)
    t["num_corr"] = rng.permutation(np.arange(20, 20 + 13 * len(pairs), 13)).astype(np.int64)
    t["verified"] = rng.uniform(size=len(pairs)) < 0.8
    t["num_inliers"] = rng.permutation(np.arange(15, 15 + 9 * len(pairs), 9)).astype(np.int64)
    t["tri_angle"] = rng.uniform(0.5, 20.0, len(pairs))
    t["config"] = rng.integers(2, 5, len(pairs)).astype(np.int64)
    t["has_score"] = t["verified"] & (rng.uniform(size=len(pairs)) < 0.85)
    t["score_sum"] = rng.uniform(1.0, 60.0, len(pairs))
    t["ignore_image"], t["ignore_ref"] = np.array(8), np.array(11)
    t["ignore_mask"] = rng.uniform(size=30) < 0.4
    return t


class StubObs:
    def __init__(self, t):
        self.row = {imid: i for i, imid in enumerate(IMAGE_IDS)}
        self.t = t

    def num_visible_points3D(self, imid):
        return int(self.t["num_visible"][self.row[imid]])

    def num_observations(self, imid):
        return int(self.t["num_observations"][self.row[imid]])

    def point3D_visibility_score(self, imid):
        return int(self.t["visibility_score"][self.row[imid]])


class StubCorrespondences:
    def __init__(self, t):
        self.pair_row = {(int(a), int(b)): k for k, (a, b) in enumerate(t["pairs"])}
        self.t = t
        self.name_to_id = {f"im{i}.jpg": i for i in IMAGE_IDS}
        self.inlier_match_scores = {frozenset([f"im{a}.jpg", f"im{b}.jpg"]): np.float64(t["score_sum"][k])
                                    for (a, b), k in self.pair_row.items() if t["has_score"][k]}

    def _row(self, a, b):
        return self.pair_row[(min(a, b), max(a, b))]

    def two_view_geom(self, name1, name2):
        k = self._row(self.name_to_id[name1], self.name_to_id[name2])
        if not self.t["verified"][k]:
            return None, False
        return SimpleNamespace(inlier_matches=np.zeros((int(self.t["num_inliers"][k]), 2), np.int32), tri_angle=float(self.t["tri_angle"][k]),
                               config=int(self.t["config"][k])), True

    def num_correspondences_between_images(self, a, b):
        return int(self.t["num_corr"][self._row(a, b)])


class StubScene:
    """images / registered_images / image_ids / obs as the reference's ImageSelection reads them"""

    def __init__(self, t, filtered_image_pairs=None):
        self.images = {}
        for imid in IMAGE_IDS:
            ignore = {int(t["ignore_ref"]): np.array(t["ignore_mask"], bool)} if imid == int(t["ignore_image"]) else {}
            self.images[imid] = SimpleNamespace(name=f"im{imid}.jpg", image_id=imid, imid=imid, has_pose=imid in REGISTERED, ignore_matches_AP=ignore)
        self.obs = StubObs(t)
        self.best_next_ref_imid = None
        if filtered_image_pairs is not None:  # the reference's own rule, bound to this object
            self.filtered_image_pairs = lambda tvg, config=2: filtered_image_pairs(self, tvg, config)

    image_ids = property(lambda s: list(s.images.keys()))
    registered_images = property(lambda s: {i: im for i, im in s.images.items() if im.has_pose})


def stub_scene(tables, filtered_image_pairs=None):
    return StubScene(tables, filtered_image_pairs), StubCorrespondences(tables)


def main():
    from make_golden_reference import REF, extract_functions

    rng = np.random.default_rng(21)
    t = make_tables(rng)
    out = {f"in/{k}": v for k, v in t.items()}
    src = ast.parse(open(os.path.join(REF, "mpsfm/sfm/mapper/image_selection.py")).read())
    names = tuple(n.name for c in src.body if isinstance(c, ast.ClassDef) and c.name == "ImageSelection" for n in c.body if isinstance(n, ast.FunctionDef))
    Ref = extract_functions("mpsfm/sfm/mapper/image_selection.py", cls="ImageSelection", method_names=names)["ImageSelection"]
    RefRec = extract_functions("mpsfm/sfm/scene/reconstruction/base.py", cls="MpsfmReconstruction", method_names=("filtered_image_pairs",))["MpsfmReconstruction"]
    for method in METHODS:
        scene, corr = stub_scene(t, RefRec.filtered_image_pairs)
        sel = Ref.__new__(Ref)
        sel.conf = SimpleNamespace(image_selection_method=method, verbose=0)
        sel._init(scene, corr)
        candidates = [i for i in IMAGE_IDS if i not in REGISTERED]
        scores = [sel.rank_image_func(i)["score"] for i in candidates]
        assert len(set(float(s) for s in scores)) == len(scores), f"{method}: equal scores, the reference's choice would be arbitrary"
        assert sel.next_image() is True
        out[f"{method}/candid"] = np.array(sel.candid)
        out[f"{method}/refid"] = np.array(-1 if scene.best_next_ref_imid is None else scene.best_next_ref_imid)
        out[f"{method}/scores"] = np.array(scores, np.float64)
        sel.at_failure(sel.candid)  # frozen: the second choice
        assert sel.next_image() is True
        out[f"{method}/candid_after_failure"] = np.array(sel.candid)
    scene, corr = stub_scene(t, RefRec.filtered_image_pairs)
    sel = Ref.__new__(Ref)
    sel.conf = SimpleNamespace(image_selection_method=METHODS[-1], verbose=0)
    sel._init(scene, corr)
    for config in range(2, 9):  # distinct counts within every config, or the order is arbitrary
        counts = [int(t["num_inliers"][k]) if t["verified"][k] else 1e-6 for k in range(len(t["pairs"])) if t["verified"][k] and t["config"][k] == config]
        assert len(set(counts)) == len(counts)
    out["init_pairs"] = np.array([sorted(p) for p in sel.find_init_pairs()], np.int64).reshape(-1, 2)
    out["init_pairs_excluding"] = np.array([sorted(p) for p in sel.find_init_pairs([frozenset(p) for p in EXCLUDE])], np.int64).reshape(-1, 2)
    out["meta"] = np.array(json.dumps(dict(methods=METHODS, image_ids=IMAGE_IDS, registered=REGISTERED, exclude=EXCLUDE)))
    path = os.path.join(HERE, "reference_image_selection.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")
    for method in METHODS:
        print(method, int(out[f"{method}/candid"]), int(out[f"{method}/refid"]), int(out[f"{method}/candid_after_failure"]))
    print(out["init_pairs"].tolist())


if __name__ == "__main__":
    main()
