"""The launch records of the level-scheduled Cholesky (csrc/chol_plan.h: LevelHead, code 14 of mpsfm_debug_plan_get) against
the tables of record they are built from (codes 6, 8 and 9: items, srcs, rows), device-free: for every graph of
graph_scenes.py, the camera graph of the benchmark's scene C3 and the star graphs of level_entry_scenes.py, every record
decodes to the type, tile, source list and row list of its item, the tail beyond the record read where the record says.
The stars are asserted to sit on the caps they are built for."""

import functools

import numpy as np
import pytest

import graph_scenes as G
import level_entry_scenes as LE
from mpsfm_amd.synthetic import make_config

K = LE.K_INLINE_SRC


def check_heads(P):
    assert len(P["heads"]) == len(P["items"]) == P["n_items"]
    for it, H in zip(P["items"], P["heads"]):
        assert (H["type"], H["ti"], H["tk"], H["nsrc"]) == (it["type"], it["ti"], it["tk"], it["nsrc"])
        assert LE.head_lists(P, H) == LE.item_lists(P, it)
        # what the record does not use is zero, so that the table is a function of the plan alone
        used_src = 0 if it["type"] == 2 else min(it["nsrc"], K)
        used_row = min(it["nsrc"], LE.K_HEAD_ROWS) if it["type"] == 2 else 0
        assert not any(H["src"][used_src:]) and not any(H["row"][used_row:]) and H["pad"] == 0
        assert H["over"] == (it["aux"] + LE.K_HEAD_ROWS if it["type"] == 2 else it["src"] + K)


@pytest.mark.parametrize("pinv", [True, False])
@pytest.mark.parametrize("name", sorted(G.CASES))
def test_heads_of_the_graph_scenes(name, pinv):
    kind, n, _, seed = G.CASES[name]
    P = LE.plan_with_heads(G.graph(kind, n, seed), pinv_max_tiles=64 if pinv else 0)
    check_heads(P)


@functools.lru_cache(maxsize=None)
def _c3_graph():
    return G.covisibility(make_config("C3")[0])


@pytest.mark.parametrize("pinv", [True, False])
def test_heads_of_the_benchmark_scene(pinv):
    P = LE.plan_with_heads(_c3_graph(), pinv_max_tiles=64 if pinv else 0)
    assert (P["nt"], P["nlevels"]) == (39, 14)
    check_heads(P)
    # no item of the benchmark's scene leaves its record, and the unrolled forms cover all of them but the trailing tail
    assert max(it["nsrc"] for it in P["items"] if it["type"] == 0) == 2
    assert max(it["nsrc"] for it in P["items"] if it["type"] == 1) <= 4
    assert max((it["nsrc"] for it in P["items"] if it["type"] == 2), default=0) <= 2


@pytest.mark.parametrize("pinv", [True, False])
@pytest.mark.parametrize("leaves", LE.STAR_LEAVES)
def test_heads_of_the_stars_sit_on_the_cap(leaves, pinv):
    P = LE.plan_with_heads(LE.star_adj(leaves), depth=-1, pinv_max_tiles=64 if pinv else 0)
    assert P["use_pinv"] == (1 if pinv and P["nt"] <= 64 else 0)
    check_heads(P)
    hub = 3 * leaves  # the first tile column of the hub
    assert P["nt"] == hub + 3
    panels = [it for it in P["items"] if it["type"] == 0 and it["tk"] == hub]
    # hub tiles that receive one level of all the leaves at once (a hub column reaches the later ones with a single source)
    trails = [it for it in P["items"] if it["type"] == 1 and it["tk"] >= hub and it["nsrc"] > 1]
    assert panels and all(it["nsrc"] == leaves for it in panels)
    assert trails and all(it["nsrc"] == leaves for it in trails)
    assert max(it["nsrc"] for it in P["items"] if it["type"] != 2) == leaves
    # the tail beyond the record is exercised exactly where the star is built for it
    over = [it for it in P["items"] if it["type"] != 2 and it["nsrc"] > K]
    assert bool(over) == (leaves > K)
    for it in panels + trails:
        src, _ = LE.item_lists(P, it)
        assert len({c & 0xffff for c in src}) == leaves  # one source per leaf


def test_role_rows_beyond_the_record_are_read_from_the_list():
    """More rows per role than a record holds (the kernels are built for fewer): the record keeps the first ones and points at the rest."""
    P = LE.plan_with_heads(LE.star_adj(2), depth=-1, inv_rows=LE.K_HEAD_ROWS + 2)
    assert any(it["type"] == 2 and it["nsrc"] > LE.K_HEAD_ROWS for it in P["items"])
    check_heads(P)
