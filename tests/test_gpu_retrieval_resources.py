"""mpsfm_retrieve_topk gives back what it took from the process-wide caches (csrc/dev_resources.h: DeviceBlocks), read through the
counters tests/test_gpu_resource_balance.py reads: the hook mpsfm_debug_resources reports the live device blocks and their bytes
and the pooled streams, events and pinned blocks that are handed out.  The body, a series of calls with different shapes, runs once
to warm up (the pools fill on first use); the hook is read, the body runs again, and the five numbers must be the same, for calls
that succeed and for a call that is refused after its blocks exist."""

import numpy as np
import pytest

from mpsfm_amd import capi

pytestmark = pytest.mark.gpu


def assert_balanced(body):
    body()
    before = capi.debug_resources()
    body()
    after = capi.debug_resources()
    print("blocks, bytes, streams, events, pinned:", before, "->", after)
    assert after == before


def test_a_series_of_calls_with_different_shapes():
    import torch

    rng = np.random.default_rng(5)
    sets = [(rng.integers(-4, 5, (n, d)) / 8.0).astype(np.float32) for n, d in ((40, 16), (333, 7), (129, 64), (1, 1))]

    def body():
        for s in sets:
            k = min(len(s), 20)
            ids = np.arange(len(s), dtype=np.int32)
            idx, _, cnt = capi.retrieve_topk(s, s, k, None, ids, ids)
            assert idx.shape == (len(s), k) and (cnt == min(k, len(s) - 1)).all()
            capi.retrieve_topk(s, sets[0][:, :1].repeat(s.shape[1], 1), 3, column_ranges=2)
            capi.retrieve_topk(s, s[:0], 128)  # no device needed
        t = torch.from_numpy(sets[1]).cuda()
        torch.cuda.synchronize()
        assert capi.retrieve_topk(t, t, 128, min_score=None)[2].tolist() == [128] * len(t)

    assert_balanced(body)


def test_a_refused_device_input():
    import torch

    d, ok = torch.zeros(70, 8, device="cuda"), torch.ones(5, 8, device="cuda")
    d[69, 7] = float("nan")
    torch.cuda.synchronize()

    def body():
        with pytest.raises(capi.MpsfmHipError) as e:
            capi.retrieve_topk(d, ok, 3)
        assert e.value.code == -1

    assert_balanced(body)
