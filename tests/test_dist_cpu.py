"""Landmark-sharded BA on CPU: world_size-2 gloo ranks run the sharded LM loop (oracle engine,
same mpsfm_allreduce_fn hook the HIP library takes) and must reproduce the single-rank result."""

import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from mpsfm_amd.dist import landmark_ranges, make_torch_allreduce, shard_problem
from mpsfm_amd.synthetic import make_scene


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, seed, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    os.environ["OMP_NUM_THREADS"] = "2"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from oracle import cpu_oracle as O

    prob, _ = make_scene(10, 800, True, seed=seed)
    shard, (lo, hi) = shard_problem(prob, rank, world)
    fn, keep = make_torch_allreduce()
    opts = O.default_options()
    opts.allreduce = fn
    s = O.solve(shard, opts)
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), lo=lo, hi=hi, pts=shard.pts, cam_quat=shard.cam_quat,
             cam_t=shard.cam_t, final_cost=s["final_cost"], initial_cost=s["initial_cost"], iters=s["num_iterations"],
             nblocks=s["num_residual_blocks"], trace=np.array(s["trace_cost"]))
    dist.barrier()
    dist.destroy_process_group()


def test_landmark_ranges_cover_and_balance():
    prob, _ = make_scene(10, 2000, True, seed=1)
    for world in (1, 2, 3, 8):
        r = landmark_ranges(prob, world)
        assert r[0][0] == 0 and r[-1][1] == prob.n_pts and all(r[i][1] == r[i + 1][0] for i in range(world - 1))
        loads = []
        for rank in range(world):
            sh, (lo, hi) = shard_problem(prob, rank, world)
            assert sh.n_pts == hi - lo and sh.n_cams == prob.n_cams
            loads.append(sh.n_obs + sh.n_dobs)
        assert sum(loads) == prob.n_obs + prob.n_dobs
        assert max(loads) <= 1.2 * (sum(loads) / world) + 50


@pytest.mark.timeout(300)
def test_two_rank_sharded_solve_matches_single_rank(tmp_path):
    from oracle import cpu_oracle as O

    seed, world = 31, 2
    ref, _ = make_scene(10, 800, True, seed=seed)
    s_ref = O.solve(ref)
    port = _free_port()
    mp.spawn(_worker, args=(world, port, seed, str(tmp_path)), nprocs=world, join=True)
    outs = [np.load(tmp_path / f"r{r}.npz") for r in range(world)]
    for o in outs:
        assert int(o["iters"]) == s_ref["num_iterations"]
        assert int(o["nblocks"]) == s_ref["num_residual_blocks"]
        assert float(o["initial_cost"]) == pytest.approx(s_ref["initial_cost"], rel=1e-12)
        assert float(o["final_cost"]) == pytest.approx(s_ref["final_cost"], rel=1e-9)
        np.testing.assert_allclose(o["cam_t"], ref.cam_t, atol=1e-7)       # replicated cameras agree
        np.testing.assert_allclose(o["pts"], ref.pts[int(o["lo"]):int(o["hi"])], atol=1e-7)
    np.testing.assert_allclose(outs[0]["cam_quat"], outs[1]["cam_quat"], atol=1e-12)


def test_strong_scaling_shards_reassemble_to_the_single_rank_problem():
    """bench.py --scaling strong: the configuration's own landmarks cut into N ranges — every residual block lands in exactly
    one shard with its values, landmark indices shift by the range start, cameras are replicated."""
    prob, _ = make_scene(14, 3000, True, seed=9)
    for world in (2, 4, 8):
        obs, dobs, pts = [], [], []
        for rank in range(world):
            sh, (lo, hi) = shard_problem(prob, rank, world)
            np.testing.assert_array_equal(sh.cam_quat, prob.cam_quat)
            np.testing.assert_array_equal(sh.pose_const, prob.pose_const)
            assert sh.gauge_axis_cam == prob.gauge_axis_cam and sh.depth_loss_type == prob.depth_loss_type
            assert sh.obs_pt.min() >= 0 and sh.obs_pt.max() < hi - lo
            obs.append(np.column_stack([sh.obs_cam, sh.obs_pt + lo, sh.obs_xy]))
            dobs.append(np.column_stack([sh.dobs_cam, sh.dobs_pt + lo, sh.dobs_depth, sh.dobs_magnitude, sh.dobs_param]))
            pts.append(sh.pts)
        np.testing.assert_array_equal(np.concatenate(pts), prob.pts)
        key = lambda a: a[np.lexsort((a[:, 0], a[:, 1]))]
        np.testing.assert_array_equal(key(np.concatenate(obs)), key(np.column_stack([prob.obs_cam, prob.obs_pt, prob.obs_xy])))
        np.testing.assert_array_equal(key(np.concatenate(dobs)),
                                      key(np.column_stack([prob.dobs_cam, prob.dobs_pt, prob.dobs_depth, prob.dobs_magnitude, prob.dobs_param])))


@pytest.mark.parametrize("world", [1, 2, 3, 5, 8, 64])
def test_camera_graph_union_through_the_sum_exchange(world):
    """What the ranks of a sharded run do at handle creation (build_host.hip pack_graph / unpack_graph, called by build_tables in ba_build.hip): adjacency indicators
    packed as base-(world+1) digits, summed, unpacked — equals the OR of the ranks' graphs, for every world size the summed
    digits stay exact."""
    import ctypes as C

    from mpsfm_amd import capi

    L = capi.lib()
    rng = np.random.default_rng(world)
    for n in (1, 7, 67, 130):
        adj = (rng.uniform(size=(world, n, n)) < 0.15).astype(np.uint8)
        adj = np.maximum(adj, adj.transpose(0, 2, 1))
        if world > 1:
            adj[0] = 0                     # a rank without landmarks
            adj[1][: n // 2, : n // 2] = 1  # ... and one dense corner, every rank's digit set somewhere
            adj[:, n - 1, n - 1] = 1       # the same edge on EVERY rank: the digit reaches `world`
        adj = np.ascontiguousarray(adj)
        out = np.zeros((n, n), np.uint8)
        E = L.mpsfm_debug_graph_union(adj.ctypes.data, world, n, out.ctypes.data)
        assert (world + 1) ** E * 1.0 <= 2.0**53 and E >= 1
        np.testing.assert_array_equal(out, adj.max(0))
