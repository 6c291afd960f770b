"""ImageSelection (mpsfm_amd/sfm/mapper/image_selection.py) against what the reference's own class chose on the stub scene of
tests/golden/reference_image_selection.npz, for all eight methods; the visibility statistics come from an injected object, so no
device is needed."""
import importlib.util
import json
import os

import numpy as np
import pytest

from mpsfm_amd.sfm.mapper.image_selection import METHODS, ImageSelection, filtered_image_pairs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load_stub_module():
    spec = importlib.util.spec_from_file_location("make_golden_image_selection", os.path.join(GOLDEN, "make_golden_image_selection.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


STUB = _load_stub_module()


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(GOLDEN, "reference_image_selection.npz"))
    tables = {k[3:]: z[k] for k in z.files if k.startswith("in/")}
    return z, tables, json.loads(str(z["meta"]))


class TableQueries:
    """visibility() from the fixture's tables, counting its calls"""

    def __init__(self, tables, image_ids):
        self.tables, self.image_ids, self.calls = tables, image_ids, 0

    def visibility(self):
        self.calls += 1
        t = self.tables
        return {imid: {"num_visible_points3D": int(t["num_visible"][i]), "num_observations": int(t["num_observations"][i]),
                       "point3D_visibility_score": int(t["visibility_score"][i])} for i, imid in enumerate(self.image_ids)}


def test_the_fixture_names_the_eight_methods_of_the_class(golden):
    _, _, meta = golden
    assert meta["methods"] == list(METHODS) and len(METHODS) == 8
    assert ImageSelection.default_conf == {"image_selection_method": "MAX_MATCHER_INLIER_SCORES", "colmap_options": "<--->", "verbose": 0}
    with pytest.raises(ValueError):
        ImageSelection({"image_selection_method": "NO_SUCH_METHOD"}, None, None)


@pytest.mark.parametrize("method", list(METHODS))
def test_next_image_chooses_what_the_reference_chose(golden, method):
    z, tables, meta = golden
    scene, corr = STUB.stub_scene(tables)
    queries = TableQueries(tables, meta["image_ids"])
    sel = ImageSelection({"image_selection_method": method}, scene, corr, scene_queries=queries)
    candidates = [i for i in meta["image_ids"] if i not in meta["registered"]]
    scores = [sel.rank_image_func(i)["score"] for i in candidates]
    np.testing.assert_array_equal(np.array(scores, np.float64), z[f"{method}/scores"])  # the same expressions: bitwise
    calls = queries.calls
    assert sel.next_image() is True
    assert sel.candid == int(z[f"{method}/candid"])
    refid = int(z[f"{method}/refid"])
    assert scene.best_next_ref_imid == (None if refid < 0 else refid)
    visibility_method = method.startswith("MAX_VISIBLE") or method == "MIN_UNCERTAINTY"
    assert queries.calls - calls == (1 if visibility_method else 0)  # all candidates from ONE call, none for the host lookups
    sel.at_failure(sel.candid)
    assert sel.freeze_imids == {sel.candid}
    assert sel.next_image() is True and sel.candid == int(z[f"{method}/candid_after_failure"])
    sel.at_success()
    assert sel.freeze_imids == set() and sel.registration_order == [sel.candid]


def test_next_image_without_a_candidate_and_with_given_candidates(golden):
    z, tables, meta = golden
    scene, corr = STUB.stub_scene(tables)
    sel = ImageSelection({"image_selection_method": "MIN_UNCERTAINTY"}, scene, corr, scene_queries=TableQueries(tables, meta["image_ids"]))
    assert sel.next_image(qry_imids=[]) is False and sel.candid is None
    assert sel.next_image(qry_imids=[8]) is True and sel.candid == 8
    for imid in [i for i in meta["image_ids"] if i not in meta["registered"]]:
        sel.at_failure(imid)
    assert sel.next_image() is False  # every candidate frozen


def test_find_init_pairs_has_the_reference_s_order(golden):
    z, tables, meta = golden
    scene, corr = STUB.stub_scene(tables)  # no filtered_image_pairs on the scene: the helper's rule
    sel = ImageSelection({}, scene, corr)
    assert [list(p) for p in sel.find_init_pairs()] == z["init_pairs"].tolist()
    excluded = [tuple(p) for p in meta["exclude"]]
    assert [list(p) for p in sel.find_init_pairs(excluded)] == z["init_pairs_excluding"].tolist()
    assert [list(p) for p in sel.find_init_pairs([frozenset(p) for p in excluded])] == z["init_pairs_excluding"].tolist()
    assert all(isinstance(p, tuple) and p[0] < p[1] for p in sel.find_init_pairs())
    # a scene with the method: its pairs (sets there) are iterated as sorted tuples
    scene.filtered_image_pairs = lambda tvg, config=2: {frozenset(p) for p in filtered_image_pairs(scene, tvg, config)}
    assert [list(p) for p in sel.find_init_pairs()] == z["init_pairs"].tolist()


def test_filtered_image_pairs_by_hand(golden):
    _, tables, _ = golden
    scene, corr = STUB.stub_scene(tables)
    for config in (2, 3, 4, 5):
        want = sorted((int(a), int(b)) for k, (a, b) in enumerate(tables["pairs"]) if tables["verified"][k] and tables["config"][k] == config)
        assert filtered_image_pairs(scene, corr.two_view_geom, config) == want
    assert filtered_image_pairs(scene, corr.two_view_geom, 5) == []
