"""Times the two scene queries (mpsfm_visibility_scores, mpsfm_local_bundles: host arrays in, host arrays out) at the C3 shape
(200 images, 150 k points) and at a dense shape of about 2 M keypoints, against this project's own plain-Python restatement of the
two rules (tests/numpy_scene_queries.py) on the host.  The restatement is NOT pycolmap: it walks Python objects point by point, as
the reference's ObservationManager and FindLocalBundle do in C++, so the ratio says what the call saves over the only host
implementation this repository has, not over COLMAP.  Median of 5 after 2 warm-ups for the calls, one run for the restatement; the
results are compared (integers exactly, angle75 within 1e-12 rad).  DESIGN.md section 4t quotes the numbers.

    python scripts/time_scene_queries.py [--shape c3|dense|both] [--no-host]
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy_scene_queries as NQ  # noqa: E402 - the restatement IS the host path that is compared against
from mpsfm_amd import capi  # noqa: E402

SHAPES = {"c3": (200, 150_000), "dense": (300, 400_000)}  # images, points; tracks of length clip(2 + Poisson(3), 2, 30)


def scene_input(n_images, n_points, registered=0.6, triangulated=0.7, seed=0):
    """Tracks over windows of consecutive images, a fresh keypoint per observation, every pair of a track's observations a
    correspondence; the first `registered` of the images have poses, `triangulated` of the points exist.  Cameras along a line with
    identity rotation, the points in front of their windows."""
    rng = np.random.default_rng(seed)
    k = np.clip(2 + rng.poisson(3.0, n_points), 2, min(30, n_images))
    t0 = rng.integers(0, n_images, n_points)
    first = np.cumsum(k) - k
    within = np.arange(k.sum()) - np.repeat(first, k)
    obs_pt, obs_img = np.repeat(np.arange(n_points), k), (np.repeat(t0, k) + within) % n_images
    order = np.argsort(obs_img, kind="stable")
    nkp = np.bincount(obs_img, minlength=n_images)
    kp_start = np.concatenate([[0], np.cumsum(nkp)]).astype(np.int64)
    kp_of_obs = np.empty(len(obs_img), np.int64)
    kp_of_obs[order] = np.arange(len(obs_img))
    n_kp = len(obs_img)
    is_reg = np.arange(n_images) < registered * n_images
    exists = rng.uniform(size=n_points) < triangulated
    kp_point = np.full(n_kp, -1, np.int64)
    sel = is_reg[obs_img] & exists[obs_pt]
    kp_point[kp_of_obs[sel]] = obs_pt[sel]
    src, dst = [], []
    for L in np.unique(k):
        base = first[k == L]
        for i in range(L):
            for j in range(L):
                if i != j:
                    src.append(kp_of_obs[base + i]); dst.append(kp_of_obs[base + j])
    src, dst = np.concatenate(src), np.concatenate(dst)
    order = np.lexsort((dst, src))
    src, dst = src[order], dst[order]
    corr_start = np.searchsorted(src, np.arange(n_kp + 1)).astype(np.int64)
    xy = rng.uniform(0, 1, (n_kp, 2)) * np.array([1600.0, 1200.0])
    size = np.tile(np.array([[1600, 1200]], np.int32), (n_images, 1))
    quat = np.zeros((n_images, 4)); quat[:, 3] = 1.0
    centres = np.stack([0.5 * np.arange(n_images), np.zeros(n_images), np.zeros(n_images)], 1)
    xyz = np.stack([0.5 * t0 + rng.uniform(-3, 3, n_points), rng.uniform(-2, 2, n_points), rng.uniform(8, 30, n_points)], 1)
    return dict(kp_start=kp_start, kp_xy=xy, corr_start=corr_start, corr_kp=dst.astype(np.int64), kp_point=kp_point, image_size=size,
                registered=is_reg.astype(np.uint8), cam_quat_xyzw=quat, cam_t=-centres, xyz=xyz)


def median_ms(fn, warmup=2, runs=5):
    for _ in range(warmup):
        out = fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t)), out


def once_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def run(shape, host):
    n_images, n_points = SHAPES[shape]
    s = scene_input(n_images, n_points)
    vis_args = [s[k] for k in ("kp_start", "kp_xy", "corr_start", "corr_kp", "kp_point", "image_size")]
    lb_args = [s[k] for k in ("kp_start", "registered", "cam_quat_xyzw", "cam_t", "kp_point", "xyz")]
    refs = [int(r) for r in np.linspace(0, 0.6 * n_images - 1, 32).astype(int)]
    out = dict(shape=shape, images=n_images, points=n_points, keypoints=int(s["kp_start"][-1]), correspondences=len(s["corr_kp"]))
    ms, vis = median_ms(lambda: capi.visibility_scores(*vis_args, return_kp_visible=False))
    out.update(visibility_call_ms=round(ms, 2), visibility_device_ms=round(vis["info"]["ms"], 3))
    for n in (1, 32):
        ms, lb = median_ms(lambda: capi.local_bundles(*lb_args, refs[:n], 6, 6.0))
        out.update({f"local_bundles_{n}_call_ms": round(ms, 2), f"local_bundles_{n}_device_ms": round(lb["info"]["ms"], 3),
                    f"local_bundles_{n}_launches": lb["info"]["num_launches"], f"local_bundles_{n}_groups": lb["info"]["num_groups"],
                    f"local_bundles_{n}_syncs": lb["info"]["num_syncs"]})
    if host:
        ms, want = once_ms(lambda: NQ.visibility(*vis_args))
        same = bool(np.array_equal(want["num_visible"], vis["num_visible"]) and np.array_equal(want["score"], vis["score"]))
        out.update(host_visibility_ms=round(ms, 1), visibility_identical=same)
        ms, want = once_ms(lambda: NQ.local_bundle(*lb_args, refs[0], 6, 6.0))
        same = same and bool(np.array_equal(want["shared"], lb["shared"][0]) and np.abs(want["angle75"] - lb["angle75"][0]).max() <= 1e-12
                             and want["bundle"] == lb["bundle"][0][:lb["bundle_len"][0]].tolist())
        out.update(host_local_bundle_one_ref_ms=round(ms, 1), identical=same)
    print(json.dumps(out), flush=True)
    if host and not out["identical"]:
        raise SystemExit("the two paths disagree")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["c3", "dense", "both"])
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    for shape in (("c3", "dense") if args.shape == "both" else (args.shape,)):
        run(shape, not args.no_host)


if __name__ == "__main__":
    main()
