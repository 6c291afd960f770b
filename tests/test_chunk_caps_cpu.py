"""The scenes of tests/chunk_cap_scenes.py reach the chunk caps they are named for: read from the device-free table build
(mpsfm_debug_host_build) under each scene's environment.  A change to the chunker that moves a scene off its cap fails here
instead of passing test_gpu_chunk_caps.py with less coverage."""

import numpy as np
import pytest

import chunk_cap_scenes as CS
from build_table_cases import environment, host_tables

# csrc/common.h
K_DENSE_CAMS, K_DENSE_PTS, K_OBS_MAX, K_PTS_MAX, K_TILE_CAMS, K_ITEM_PAIRS, K_ENT_STAGE = 16, 96, 252, 126, 16, 64, 1024


@pytest.fixture(scope="module")
def built():
    out = {}
    for name in CS.SCENES:
        with environment(CS.environment_of(name)):
            t = host_tables(CS.problem(name))
        out[name] = t, CS.shapes(t)
    return out


def count(rows, nrec=None, npt=None, ncam=None):
    return sum((nrec is None or r[0] == nrec) and (npt is None or r[1] == npt) and (ncam is None or r[2] == ncam) for r in rows)


@pytest.mark.parametrize("name", list(CS.SCENES))
def test_every_chunk_is_within_the_caps_and_of_the_expected_kind(built, name):
    _, s = built[name]
    for nrec, npt, ncam, nent in s["dense"]:
        assert nrec <= K_OBS_MAX and npt <= K_DENSE_PTS and ncam <= K_DENSE_CAMS and nent == 0
    for nrec, npt, ncam, nent in s["general"]:
        assert nrec <= K_OBS_MAX and npt <= K_PTS_MAX and nent > 0
    for items in s["items"]:
        assert items.min() >= 1 and items.max() <= K_ITEM_PAIRS
    assert (not s["general"] and not s["long"]) == (name in CS.ALL_DENSE)
    assert len(s["dense"]) > 0


def test_two_view(built):
    """96 landmarks x 2 records = 192 of 252 lanes, camera sets of 1, 2 and 3; without the switches the same problem stays at 64 records."""
    _, s = built["two_view"]
    assert len(s["dense"]) == 7 and count(s["dense"], nrec=192, npt=K_DENSE_PTS) == 6
    assert count(s["dense"], ncam=1) == 2 and count(s["dense"], nrec=192, npt=K_DENSE_PTS, ncam=1) == 1
    assert count(s["dense"], ncam=2) == 3 and count(s["dense"], ncam=3) == 2
    plain = CS.shapes(host_tables(CS.problem("two_view")))["dense"]
    assert max(r[0] for r in plain) == 64 and max(r[1] for r in plain) < K_DENSE_PTS


def test_pairs16(built):
    _, s = built["pairs16"]
    assert len(s["dense"]) == 6 and count(s["dense"], npt=K_DENSE_PTS) == 5
    assert count(s["dense"], nrec=192, npt=K_DENSE_PTS, ncam=K_DENSE_CAMS) == 1


def test_mixed16(built):
    t, s = built["mixed16"]
    assert len(s["dense"]) == 12 and count(s["dense"], nrec=K_OBS_MAX, ncam=K_DENSE_CAMS) == 2 and count(s["dense"], ncam=K_DENSE_CAMS) == 8
    assert count(s["dense"], nrec=240, npt=15, ncam=16) == 1               # the landmarks every camera sees
    assert np.bincount(t["pt_kv"][:-1])[16] >= 15 and set(t["pt_kv"][:-1].tolist()) == set(range(2, 17))


def test_one_var(built):
    """A single variable camera: every chunk has one local camera, every variable landmark one variable record, and the blocks of a
    constant camera on a constant landmark are on the fixed list."""
    t, s = built["one_var"]
    prob = CS.problem("one_var")
    assert len(s["dense"]) == 8 and count(s["dense"], ncam=1) == 8
    kv = t["pt_kv"][:prob.n_pts][prob.pt_const[t["order"]] == 0]
    assert len(kv) == 205 and (kv == 1).all()
    assert len(t["fx_cam"]) == 44 and (t["rec_meta"] & 0xff == 255).any()


def test_g17_40(built):
    """General chunks of 17 local cameras (one past the LDS tile) and of 40; pair entries on either side of the LDS stage."""
    _, s = built["g17_40"]
    assert len(s["general"]) == 5 and count(s["general"], ncam=K_TILE_CAMS + 1) == 2 and count(s["general"], ncam=40) == 3
    nent = sorted(r[3] for r in s["general"])
    assert nent == [820, 2142, 2142, 4406, 4920] and nent[0] < K_ENT_STAGE < nent[1]
    assert count(s["dense"], ncam=K_DENSE_CAMS) == 3 and s["split"] == 0


def test_dup_aab(built):
    """Two blocks of one camera and one of another: 84 landmarks x 3 records = kObsMax, blocks of 336, 168 and 84 pairs cut into
    work items of kItemPairs, all entries staged in LDS."""
    _, s = built["dup_aab"]
    assert s["general"] == [(K_OBS_MAX, 84, 2, 588), (K_OBS_MAX, 84, 2, 588), (96, 32, 2, 224)] and 588 < K_ENT_STAGE
    assert sorted(s["items"][0].tolist()) == sorted([64] * 5 + [16] + [64] * 2 + [40] + [64, 20])
    assert max(int(i.max()) for i in s["items"]) == K_ITEM_PAIRS and s["split"] == 17


def test_dup_aa(built):
    """Two blocks of one camera only: kPtsMax landmarks in a chunk of one local camera."""
    _, s = built["dup_aa"]
    assert s["general"] == [(K_OBS_MAX, K_PTS_MAX, 1, 504), (K_OBS_MAX, K_PTS_MAX, 1, 504), (96, 48, 1, 192)]
    assert max(int(i.max()) for i in s["items"]) == K_ITEM_PAIRS and s["split"] == 16


def test_r252_253(built):
    """A track of exactly kObsMax records stays chunked (one landmark, 252 local cameras, 252 * 253 / 2 blocks of one pair each); one
    more record makes a long track."""
    _, s = built["r252_253"]
    assert s["general"] == [(K_OBS_MAX, 1, 252, 252 * 253 // 2)] and s["items"][0].max() == 1
    assert s["long"] == [(253, 253), (255, 255)]
    assert len(s["dense"]) == 19
