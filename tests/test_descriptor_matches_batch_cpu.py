"""mpsfm_match_descriptors_batch and mpsfm_amd/extraction/pairwise/match_sparse.py without a GPU: every argument check (all come
before any HIP call), what a batch does when no pair needs a device, the wrapper's return types, and the pair bookkeeping of
match_sparse.  With a device the same valid calls are computed: tests/test_gpu_descriptor_matches_batch.py."""

import ctypes as C

import numpy as np
import pytest

from mpsfm_amd import capi
from mpsfm_amd.extraction.pairwise import find_unique_new_pairs, match_pairs, names_to_pair, names_to_pair_old

EINVAL, ENODEVICE = -1, -2
P = lambda a: None if a is None else a.ctypes.data  # noqa: E731


class Batch:
    """a valid batch of three images (3, 2 and 0 descriptors, dim 4) and three pairs; call(**changes) replaces arguments"""

    def __init__(self):
        self.start = np.array([0, 3, 5, 5], np.int64)
        self.desc = np.ones((5, 4), np.float32)
        self.p0, self.p1 = np.array([0, 1, 0], np.int32), np.array([1, 0, 0], np.int32)
        self.mstart = np.array([0, 3, 5, 8], np.int64)
        self.m, self.s, self.cnt = np.full(8, 7, np.int32), np.full(8, 7.0), np.full(3, 7, np.int64)
        self.report = capi.CMatchBatchReport()

    def call(self, **kw):
        a = dict(num_images=3, start=self.start, dim=4, desc=self.desc, num_pairs=3, p0=self.p0, p1=self.p1, mstart=self.mstart, opts=None,
                 column_ranges=0, pairs_per_group=0, m=self.m, s=self.s, cnt=self.cnt, report=self.report)
        a.update(kw)
        return capi.lib().mpsfm_match_descriptors_batch(
            a["num_images"], P(a["start"]), a["dim"], P(a["desc"]), a["num_pairs"], P(a["p0"]), P(a["p1"]), P(a["mstart"]),
            None if a["opts"] is None else C.addressof(a["opts"]), a["column_ranges"], a["pairs_per_group"], 0, P(a["m"]), P(a["s"]),
            P(a["cnt"]), None if a["report"] is None else C.addressof(a["report"]))


def last_error():
    return capi.lib().mpsfm_last_error().decode()


def arr(values, dtype):
    return np.array(values, dtype)


@pytest.mark.parametrize("name,changes,names_it", [
    ("image_start NULL", dict(start=None), None),
    ("desc NULL", dict(desc=None), None),
    ("pair_image0 NULL", dict(p0=None), None),
    ("pair_image1 NULL", dict(p1=None), None),
    ("match_start NULL", dict(mstart=None), None),
    ("matches0 NULL", dict(m=None), None),
    ("scores0 NULL", dict(s=None), None),
    ("negative num_images", dict(num_images=-1), None),
    ("negative num_pairs", dict(num_pairs=-1), None),
    ("image_start[0] != 0", dict(start=arr([1, 3, 5, 5], np.int64)), None),
    ("a decreasing image offset", dict(start=arr([0, 3, 2, 5], np.int64)), "image 1"),
    ("an image of more than 2^24 descriptors", dict(start=arr([0, 3, 5, 5 + (1 << 24) + 1], np.int64)), "image 2"),
    ("dim 0", dict(dim=0), None),
    ("dim 1025", dict(dim=1025), None),
    ("a pair index below 0", dict(p1=arr([1, -1, 0], np.int32)), "pair 1"),
    ("a pair index beyond the images", dict(p0=arr([0, 1, 3], np.int32)), "pair 2"),
    ("match_start[0] != 0", dict(mstart=arr([1, 4, 6, 9], np.int64)), None),
    ("a slice that is not as long as its first image", dict(mstart=arr([0, 3, 6, 9], np.int64)), "pair 1"),
    ("negative column_ranges", dict(column_ranges=-1), None),
    ("negative pairs_per_group", dict(pairs_per_group=-1), None),
])
def test_every_argument_check_comes_before_any_device(name, changes, names_it):
    b = Batch()
    assert b.call(**changes) == EINVAL, name
    if names_it:
        assert names_it in last_error(), (name, last_error())
    assert b.m.tolist() == [7] * 8 and b.cnt.tolist() == [7] * 3  # nothing was written


def test_non_finite_thresholds_and_values_are_refused():
    b = Batch()
    for bad in (np.nan, np.inf, -np.inf):
        for field in ("ratio_threshold", "distance_threshold", "score_threshold"):
            o = capi._match_options(None, None, None, True)
            setattr(o, field, bad)
            assert b.call(opts=o) == EINVAL and "threshold" in last_error()
        x = b.desc.copy()
        x[4, 3] = bad
        assert b.call(desc=x) == EINVAL and "image 1" in last_error() and "non-finite" in last_error()
        assert b.call(desc=x, num_pairs=0) == EINVAL  # checked whether or not a pair reads it


def test_optional_pointers_and_an_empty_pair_list():
    b = Batch()
    assert b.call(num_pairs=0, p0=None, p1=None, mstart=np.zeros(1, np.int64), m=None, s=None, cnt=None, report=None) == 0
    assert b.call(num_pairs=0, mstart=np.zeros(1, np.int64)) == 0
    assert b.m.tolist() == [7] * 8 and b.report.num_launches == 0 and b.report.num_syncs == 0
    assert b.call(num_images=0, start=np.zeros(1, np.int64), desc=None, num_pairs=0, mstart=np.zeros(1, np.int64)) == 0


def test_pairs_with_an_empty_side_need_no_device():
    b = Batch()
    # (0, 2) and (1, 2): no columns, all -1 / 0.  (2, 0): no rows, an empty slice.
    p0, p1 = np.array([0, 2, 1], np.int32), np.array([2, 0, 2], np.int32)
    mstart = np.array([0, 3, 3, 5], np.int64)
    b.report.num_groups = 9
    assert b.call(p0=p0, p1=p1, mstart=mstart) == 0
    assert b.m[:5].tolist() == [-1] * 5 and b.s[:5].tolist() == [0.0] * 5 and b.m[5:].tolist() == [7] * 3
    assert b.cnt.tolist() == [0, 0, 0]
    r = b.report
    assert (r.num_matches, r.num_groups, r.num_launches, r.num_syncs, r.num_workgroups, r.ms) == (0, 0, 0, 0, 0, 0.0)
    assert b.call(p0=p0, p1=p1, mstart=mstart, cnt=None, report=None, opts=capi._match_options(0.8, 0.7, None, False)) == 0


def test_any_other_batch_needs_a_device():
    b = Batch()
    want = 0 if capi.device_count() > 0 else ENODEVICE
    assert b.call() == want
    assert b.call(opts=capi._match_options(0.8, 0.7, None, False), column_ranges=3, pairs_per_group=1) == want
    if want:
        assert "no HIP device" in last_error()
        with pytest.raises(capi.MpsfmHipError) as e:
            capi.match_descriptors_batch([np.ones((3, 4), np.float32), np.ones((2, 4), np.float16)], [(0, 1)])
        assert e.value.code == ENODEVICE
        feats = {"a": {"descriptors": np.ones((4, 3), np.float32)}, "b": {"descriptors": np.ones((4, 2), np.float32)}}
        for batched in (True, False):
            with pytest.raises(capi.MpsfmHipError) as e:
                match_pairs({}, [("a", "b")], feats, batched=batched)
            assert e.value.code == ENODEVICE


def test_wrapper_return_types_on_empty_input():
    import torch

    e, d = np.zeros((0, 8), np.float32), np.ones((3, 8), np.float16)
    m, s = capi.match_descriptors_batch([], [])
    assert m == [] and s == []
    m, s, info = capi.match_descriptors_batch([e, d], [(0, 1), (1, 0), (0, 0)], ratio_threshold=0.8, return_info=True)
    assert [x.tolist() for x in m] == [[], [-1, -1, -1], []] and [x.tolist() for x in s] == [[], [0.0, 0.0, 0.0], []]
    assert all(x.dtype == np.int64 for x in m) and all(x.dtype == np.float64 for x in s)
    assert info["pair_num_matches"].tolist() == [0, 0, 0] and info["pair_num_matches"].dtype == np.int64
    assert {k: v for k, v in info.items() if k != "pair_num_matches"} == dict(num_matches=0, num_groups=0, num_launches=0, num_syncs=0,
                                                                              num_workgroups=0, ms=0.0)
    m, s = capi.match_descriptors_batch([torch.zeros(0, 8), torch.ones(3, 8, dtype=torch.float16)], [(1, 0)])
    assert isinstance(m[0], np.ndarray) and m[0].tolist() == [-1, -1, -1]
    with pytest.raises(TypeError):
        capi.match_descriptors_batch([np.ones((3, 8)), np.ones((2, 8))], [(0, 1)])
    with pytest.raises(ValueError):
        capi.match_descriptors_batch([np.ones((3, 8), np.float32), np.ones((2, 7), np.float32)], [(0, 1)])
    with pytest.raises(ValueError):
        capi.match_descriptors_batch([np.ones((3, 8), np.float32)], [(0, 1)])
    with pytest.raises(ValueError):
        capi.match_descriptors_batch([np.ones(8, np.float32)], [(0, 0)])


# ---- match_sparse --------------------------------------------------------------------------------------------------------------
def test_names_to_pair_replaces_the_slash_in_a_name():
    assert names_to_pair("a.jpg", "b.jpg") == "a.jpg/b.jpg" and names_to_pair_old("a.jpg", "b.jpg") == "a.jpg_b.jpg"
    assert names_to_pair("seq/a.jpg", "seq/sub/b.jpg") == "seq-a.jpg/seq-sub-b.jpg"
    assert names_to_pair_old("seq/a.jpg", "b.jpg") == "seq-a.jpg_b.jpg"


def test_find_unique_new_pairs_keeps_the_first_appearance():
    pairs = [("c", "a"), ("a", "b"), ("b", "a"), ("a", "b"), ("b", "c"), ("a", "c"), ("d", "d"), ("c", "b"), ("d", "d")]
    assert find_unique_new_pairs(pairs) == [("c", "a"), ("a", "b"), ("b", "c"), ("d", "d")]  # in order of first appearance
    assert find_unique_new_pairs([]) == [] and find_unique_new_pairs(iter(pairs), set()) == find_unique_new_pairs(pairs)
    # `existing` holds a pair under either key form, in either order
    for key in (names_to_pair("a", "b"), names_to_pair("b", "a"), names_to_pair_old("a", "b"), names_to_pair_old("b", "a")):
        assert find_unique_new_pairs(pairs, {key}) == [("c", "a"), ("b", "c"), ("d", "d")], key
        assert find_unique_new_pairs(pairs, {key: None}) == [("c", "a"), ("b", "c"), ("d", "d")]  # anything that answers `in`
    assert find_unique_new_pairs(pairs, {"d/d", "c_b"}) == [("c", "a"), ("a", "b")]
    assert find_unique_new_pairs([("s/a", "s/b")], {"s-b/s-a"}) == []


def test_match_pairs_keys_layout_and_types_without_a_device():
    import torch

    feats = {"s/a": {"descriptors": np.ones((8, 3), np.float16)}, "s/b": {"descriptors": np.ones((8, 0), np.float16)}}
    pairs = [("s/a", "s/b"), ("s/b", "s/a"), ("s/b", "s/b")]
    for batched in (True, False):
        out = match_pairs({"ratio_threshold": 0.8}, pairs, feats, batched=batched)
        assert list(out) == ["s-a/s-b", "s-b/s-a", "s-b/s-b"]
        for key, n in zip(out, (3, 0, 0)):  # [D, N] in, [1, N] out, as NearestNeighbor returns it
            m, s = out[key]["matches0"], out[key]["matching_scores0"]
            assert isinstance(m, np.ndarray) and m.dtype == np.int64 and s.dtype == np.float64 and m.shape == s.shape == (1, n)
            assert (m == -1).all() and (s == 0).all()
        assert match_pairs(None, [], feats, batched=batched) == {}
    # the second name is looked up in features_ref when there is one: "s/a" is the empty image there
    ref = {"s/a": {"descriptors": torch.ones(8, 0)}}
    tf = {"s/a": {"descriptors": torch.ones(8, 3, dtype=torch.float16)}}
    for batched in (True, False):
        out = match_pairs({}, [("s/a", "s/a")], tf, ref, batched=batched)
        m, s = out["s-a/s-a"]["matches0"], out["s-a/s-a"]["matching_scores0"]
        assert isinstance(m, torch.Tensor) and m.dtype == torch.int64 and s.dtype == torch.float64 and m.tolist() == [[-1, -1, -1]]
        with pytest.raises(TypeError):
            match_pairs({}, [("x", "x")], {"x": {"descriptors": np.ones((8, 3))}}, batched=batched)
        with pytest.raises(KeyError):
            match_pairs({}, [("s/a", "s/b")], tf, ref, batched=batched)
