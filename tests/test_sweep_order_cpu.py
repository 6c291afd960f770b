"""The order table of the dense track sweep (SweepArgs::order, csrc/common.h): workgroup b of k_track_sweep_dense takes chunk
order[b], the chunks by descending dense_sweep_cost, ties by ascending index.  Device-free, through mpsfm_debug_host_build: code 35
is the table, 36 the cost of every dense chunk as the library computes it from the chunk header, 0 the headers.

The last test is a condition on the ORDER, not a timing: a list-scheduling model of the dispatcher (768 resident workgroups on
the MI355X — 256 CUs x 3 —, a freed slot takes the next workgroup of the launch 1 us later) over the chunk table of the benchmark
scene C3 with the committed cost function.  In table order the heavy chunks that start in the last round of workgroups end long after
the rest has drained; heaviest first, the makespan has to come within 15 % of the ideal sum / 768."""

import heapq

import numpy as np
import pytest

from build_table_cases import CASES, environment
from mpsfm_amd import capi
from mpsfm_amd.synthetic import make_config

HDR_WORDS = 12      # int32 words of a ChunkHdr: rec0 nrec pt0 npt cam0 ncam blk0 nblk ent0 nent dense slab0
SLOTS = 768         # resident workgroups of k_track_sweep_dense: 256 CUs x 3 (LDS)
CYCLES_PER_US = 41.2e3 / 19.2   # the calibration of dense_sweep_cost: a wave life of 41.2 k shader cycles is 19.2 us
GAP_US = 1.0        # a freed slot starts its next workgroup this much later


def _tables(case):
    make, env, _ = CASES[case]
    prob = make()
    with environment({"MPSFM_DEV_BUILD": "0", **env}):
        hdr = capi.host_build_table(prob, 0, np.int32).reshape(-1, HDR_WORDS)
        return hdr, capi.host_build_table(prob, 35, np.int32), capi.host_build_table(prob, 36, np.int32)


@pytest.mark.parametrize("case", ["b", "e", "g", "i"])
def test_the_table_orders_the_dense_chunks_by_descending_cost(case):
    hdr, order, cost = _tables(case)
    n_dense = int(np.sum(hdr[:, 10] == 1))
    assert np.all(hdr[:n_dense, 10] == 1) and np.all(hdr[n_dense:, 10] == 0), "dense chunks precede the general ones"
    if case == "g":
        assert 0 < n_dense < len(hdr), "case g is meant to hold general chunks beside the dense ones"
    if case == "e":
        assert n_dense >= 100, "MPSFM_CHUNK_RECORDS=64 is meant to give many chunks"
    assert len(order) == n_dense and len(cost) == n_dense
    assert np.array_equal(np.sort(order), np.arange(n_dense)), "a permutation of the dense chunk indices"
    along = cost[order].astype(np.int64)
    assert np.all(np.diff(along) <= 0), "cost is non-increasing along the table"
    tie = np.diff(along) == 0
    assert np.all(np.diff(order)[tie] > 0), "ties are in ascending chunk index"
    # the cost comes from (nrec, npt, ncam) alone ...
    by_key = {}
    for h, c in zip(hdr[:n_dense], cost):
        assert by_key.setdefault((int(h[1]), int(h[3]), int(h[5])), int(c)) == int(c)
    assert np.all(cost > 0)


def test_the_cost_grows_with_records_landmarks_and_cameras():
    hdr, _, cost = _tables("i")
    n = len(cost)
    key = hdr[:n, [1, 3, 5]].astype(np.int64)
    # every pair of chunks where one dominates the other in all three numbers (a sample of the table is enough)
    idx = np.arange(0, n, max(1, n // 200))
    a, b = key[idx][:, None, :], key[idx][None, :, :]
    dominated = np.all(a <= b, axis=2)
    ci, cj = np.nonzero(dominated)
    assert np.all(cost[idx][ci] <= cost[idx][cj])
    assert dominated.sum() > len(idx), "the sample holds comparable chunks"


def makespan_us(cost_cycles, slots=SLOTS, gap_us=GAP_US):
    """List scheduling: workgroups start in launch order, each in the slot that frees first; (makespan, ideal = sum / slots) in us."""
    life = np.asarray(cost_cycles, np.float64) / CYCLES_PER_US
    free = [0.0] * slots
    heapq.heapify(free)
    end = 0.0
    for i, t in enumerate(life):
        start = heapq.heappop(free)
        if i >= slots:
            start += gap_us
        heapq.heappush(free, start + t)
        end = max(end, start + t)
    return end, float(life.sum()) / slots


@pytest.fixture(scope="module")
def c3_tables():
    prob, _ = make_config("C3")
    with environment({"MPSFM_DEV_BUILD": "0"}):
        return capi.host_build_table(prob, 35, np.int32), capi.host_build_table(prob, 36, np.int32)


def test_heaviest_first_shortens_the_modelled_tail_at_c3(c3_tables):
    order, cost = c3_tables
    assert len(order) > 3 * SLOTS, "C3 takes several rounds of workgroups"
    in_table_order, ideal = makespan_us(cost)
    in_new_order, _ = makespan_us(cost[order])
    print(f"C3: {len(order)} dense chunks; modelled makespan {in_table_order:.1f} us in table order, {in_new_order:.1f} us heaviest first, ideal {ideal:.1f} us")
    assert in_table_order - in_new_order > 0.0
    assert in_new_order <= 1.15 * ideal
