"""Every entry point gives back what it took from the process-wide caches (csrc/dev_resources.h: DeviceBlocks).  The hook
mpsfm_debug_resources reports the live device blocks and their bytes and the pooled streams, events and pinned blocks that are
handed out; each case runs its body once to warm up (the staging buffer and the pools fill on first use), reads the hook, runs
the body again and asserts the same five numbers — for calls that succeed, for calls that are refused after their blocks exist,
and for handles that are created and destroyed."""

import os

import numpy as np
import pytest

import chunk_cap_scenes
import numpy_mono_priors as NMP
import numpy_two_view_geometry as TV
from conftest import GOLDEN
from mpsfm_amd import capi
from mpsfm_amd.synthetic import make_scene
from mpsfm_amd.synthetic_maps import make_maps
from test_gpu_pt_handoff import chain_scene

pytestmark = pytest.mark.gpu

BUILD_SWITCHES = ("MPSFM_DEV_BUILD", "MPSFM_CHOL_NB", "MPSFM_SLAB_TABLES_HOST", "MPSFM_LOCAL_LM")


def assert_balanced(body):
    body()
    before = capi.debug_resources()
    body()
    after = capi.debug_resources()
    print("blocks, bytes, streams, events, pinned:", before, "->", after)
    assert after == before


def handle_round_trip(prob, monkeypatch, env=None):
    """create / solve / get_state / destroy under the given switches; returns what the handle's tables say of its path"""
    for k in BUILD_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    seen = {}

    def body():
        out = prob.copy()
        h = capi.BAHandle(prob.copy())
        s = h.solve()
        h.get_state(out)
        seen.update(iterations=s["num_iterations"], on_device=bool(np.frombuffer(table(h, 22), np.uint8)[0]),
                    general=int((np.frombuffer(table(h, 0), np.int32).reshape(-1, 12)[:, 10] == 0).sum()),
                    held=capi.debug_resources())
        h.close()

    assert_balanced(body)
    assert seen["iterations"] > 0
    assert seen["held"][0] > capi.debug_resources()[0] and seen["held"][3] >= capi.debug_resources()[3] + 8  # the hook sees a handle
    return seen


def table(h, which):
    L = capi.lib()
    n = L.mpsfm_debug_table(h._h, which, None, 0)
    assert n >= 0
    buf = np.zeros(max(int(n), 1), np.uint8)
    assert L.mpsfm_debug_table(h._h, which, buf.ctypes.data, int(n)) == n
    return buf[:n].tobytes()


# ---- bundle adjustment: create / solve / get_state / destroy ------------------------------------------------------------------------
def test_single_launch_handle(monkeypatch):
    seen = handle_round_trip(make_scene(6, 300, True, seed=2)[0], monkeypatch)
    assert seen["on_device"]


@pytest.mark.parametrize("env,on_device", [({}, True), ({"MPSFM_DEV_BUILD": "0"}, False), ({"MPSFM_CHOL_NB": "3"}, True),
                                            ({"MPSFM_SLAB_TABLES_HOST": "0"}, True)],
                         ids=["device_build", "host_build", "second_stream", "device_slab_tables"])
def test_launch_chain_handle(env, on_device, monkeypatch):
    seen = handle_round_trip(chain_scene()[0], monkeypatch, env)
    assert seen["on_device"] == on_device and seen["general"] == 0
    if "MPSFM_CHOL_NB" in env:
        assert seen["held"][2] >= capi.debug_resources()[2] + 2  # the handle's stream and the second one


def test_handle_with_general_chunks(monkeypatch):
    """A track longer than kDenseCams: a device build whose general chunks get their pair tables from the host."""
    seen = handle_round_trip(chunk_cap_scenes.problem("g17_40"), monkeypatch, chunk_cap_scenes.environment_of("g17_40"))
    assert seen["on_device"] and seen["general"] > 0


def test_with_statement_and_one_shot(monkeypatch):
    for k in BUILD_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    prob = make_scene(6, 300, True, seed=2)[0]

    def with_handle():
        with capi.BAHandle(prob.copy()) as h:
            assert h.solve()["num_iterations"] > 0

    assert_balanced(with_handle)
    assert_balanced(lambda: capi.ba_solve(prob.copy()))


# ---- bundle adjustment: a create that fails after device allocations ---------------------------------------------------------------
def nonpositive_depth():
    prob = chain_scene()[0].copy()
    prob.dobs_depth[len(prob.dobs_depth) // 2] = -1.0
    return prob, "depth prior must be positive"


def nonpositive_shifted_depth():
    prob = chain_scene()[0].copy()
    prob.shift_logscale = np.zeros((prob.n_cams, 2))
    prob.shift_logscale[int(prob.dobs_cam[0]), 0] = -1e3  # depth * exp(0) - 1000 <= 0
    assert (prob.dobs_depth > 0).all()
    return prob, "shifted/scaled depth prior must be positive"


@pytest.mark.parametrize("dev_build", ["1", "0"])
@pytest.mark.parametrize("case", [nonpositive_depth, nonpositive_shifted_depth])
def test_refused_create(case, dev_build, monkeypatch):
    for k in BUILD_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MPSFM_DEV_BUILD", dev_build)
    prob, text = case()

    def body():
        with pytest.raises(capi.MpsfmHipError) as e:
            capi.BAHandle(prob.copy())
        assert e.value.code == -1 and str(e.value).endswith(": " + text)

    assert_balanced(body)


# ---- stateless calls ------------------------------------------------------------------------------------------------------------------
def refused(call):
    def body():
        with pytest.raises(capi.MpsfmHipError) as e:
            call()
        assert e.value.code == -1

    return body


def test_refused_device_inputs():
    """One NaN in a device tensor: MPSFM_EINVAL after the call's blocks exist."""
    import torch

    desc, ok = torch.zeros(70, 8, device="cuda"), torch.ones(5, 8, device="cuda")
    desc[69, 7] = float("nan")
    warp, cert = torch.zeros(9, 70, 4, device="cuda"), torch.full((9, 70), 0.5, device="cuda")
    warp[8, 69, 3] = float("nan")
    k = np.ones((3, 2))
    A, B = torch.rand(12, 13, 8, device="cuda"), torch.rand(9, 17, 8, device="cuda")
    B[-1, -1, -1] = float("nan")
    torch.cuda.synchronize()
    assert_balanced(refused(lambda: capi.match_descriptors(desc, ok)))
    assert_balanced(refused(lambda: capi.warp_matches(warp, cert, (30, 40, 30, 40), 1, skpts0=k, skpts1=k)))
    assert_balanced(refused(lambda: capi.reciprocal_nns(A, B, 2)))


def integration_arguments():
    maps = make_maps(8, 8, seed=1, n_sparse=6)
    nu = maps["normals_uncertainty"]
    nvar = np.stack([nu[..., 0, 0], nu[..., 1, 1], nu[..., 2, 2]], -1)
    return maps, (maps["depth_prior"], maps["depth_uncertainty"], maps["valid"], maps["normals"], nvar, maps["depth_init"], maps["K"])


def test_integration_calls():
    maps, args = integration_arguments()

    def integrate():
        _, s, *_ = capi.integrate_depth(*args, maps["kps"], maps["depth3d"], maps["zvars3d"])
        assert s["irls_iterations"] > 0 and s["ms"] > 0

    def variances():
        v, s = capi.integration_variances(*args, np.array([[1, 2], [6, 5]]))
        assert s["converged"] and s["ms"] > 0 and (v > 0).all()

    assert_balanced(integrate)
    assert_balanced(variances)


def test_depth_priors_call():
    meta, item, _ = NMP.fixture_cases(np.load(os.path.join(GOLDEN, "reference_mono_priors.npz")), "depth")[0]
    assert_balanced(lambda: capi.depth_priors([item], dict(NMP.DEPTH_CONF, **meta["conf"])))


def test_match_descriptors_batch_call():
    rng = np.random.default_rng(5)
    descs = [rng.normal(size=(n, 16)).astype(np.float32) for n in (40, 33, 57)]
    descs = [d / np.linalg.norm(d, axis=1, keepdims=True) for d in descs]
    assert_balanced(lambda: capi.match_descriptors_batch(descs, [(0, 1), (1, 2), (0, 2)], pairs_per_group=2))


def test_two_view_geometry_call():
    s = TV.synthetic_pair("general", 50, 0.2, 0, 0.0)
    args = (s["points1"], s["points2"], s["intr1"], s["intr2"], s["size1"], s["size2"])
    assert_balanced(lambda: capi.two_view_geometry(*args, max_num_trials=100))


def test_debug_panel_factor_call():
    rng = np.random.default_rng(6)
    M = rng.normal(size=(32, 32))
    dx = np.concatenate([M @ M.T + 32 * np.eye(32), rng.normal(size=(32, 32))])
    assert_balanced(lambda: capi.debug_panel_factor(dx, 4))


# ---- the triangulator handle --------------------------------------------------------------------------------------------------------
def test_triangulator_handle():
    from mpsfm_amd.sfm.mapper.triangulator import MpsfmTriangulator
    from test_gpu_triangulator import OPTS, empty_scene, register_all

    def body():
        sc, cg, _, _ = empty_scene(4, 120, 71)
        tri = MpsfmTriangulator({"colmap_options": dict(OPTS), "lift_low_parallax": False}, sc, cg)
        assert register_all(sc, tri) > 0 and tri._triangulator.stats()["batch_candidates"] > 0
        tri._triangulator.close()

    assert_balanced(body)
