"""Times `prepare_mono_priors` (one mpsfm_depth_priors + one mpsfm_normal_priors call) for 1, 8 and 64 images of
518x692 source maps and a 290x387 target, in the default configuration and with flip_consistency, next to the NumPy
restatement of the tests (tests/numpy_mono_priors.py) on the same inputs.  Needs a gfx950 device.

Host wall time around the whole call (it ends with the download, so the device is idle when the clock stops), after a
warm-up call per shape; median and spread of `--repeats` calls.  The device time of the launches alone (HIP events) is
printed next to it.  The NumPy time is per image (after a warm-up call, the median over `--repeats` passes over
`--numpy-images` images, each call timed on its own) and scaled to the batch: the restatement loops over images.  No
comparison with the reference itself: it needs OpenCV.

  python scripts/time_mono_priors.py [--repeats 7] [--numpy-images 2] [--out FILE]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy_mono_priors as NMP  # noqa: E402
from mpsfm_amd import capi  # noqa: E402
from mpsfm_amd.sfm.scene.image import Depth, Normals, prepare_mono_priors  # noqa: E402

SRC, DST, IMAGE = (518, 692), (290, 387), (2900.0, 3870.0)


def draw(rng, n):
    """n distinct images: float32 maps as the extractors store them, 2000 keypoints each"""
    cam = types.SimpleNamespace(int_height=DST[0], int_width=DST[1], sx=DST[1] / IMAGE[1], sy=DST[0] / IMAGE[0])
    items = []
    for _ in range(n):
        d = {k: v.astype(np.float32) for k, v in NMP.depth_maps(rng, SRC).items()}
        m = NMP.normal_maps(rng, SRC, np.where(rng.uniform(size=SRC) < 0.5, 0.03, 0.35))
        items.append(dict(depth_dict=d, normals_dict={k: v.astype(np.float32) for k, v in m.items()}, camera=cam,
                          kps=rng.uniform(0, 1, (2000, 2)) * [IMAGE[1], IMAGE[0]], mask=rng.uniform(size=(1036, 1384)) > 0.05))
    return items


def numpy_once(it, dconf, nconf):
    cam = it["camera"]
    d = NMP.depth_priors(dict(it["depth_dict"], size=DST, kps=it["kps"], sx=cam.sx, sy=cam.sy, mask=it["mask"]), dconf)
    NMP.normal_priors(dict(it["normals_dict"], size=DST, mask=it["mask"], continuity_mask=d["continuity_mask"]), nconf)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--numpy-images", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("time_mono_priors.py needs a gfx950 device: there is no CPU path to time")
    rng = np.random.default_rng(1)
    items = draw(rng, 64)
    rows = []
    for tag, dconf, nconf in (("default", {}, {}), ("flip_consistency", dict(flip_consistency=True), dict(flip_consistency=True))):
        numpy_once(items[0], dconf, nconf)  # warm-up
        per_image = []
        for _ in range(a.repeats):
            for it in items[: a.numpy_images]:
                t0 = time.perf_counter()
                numpy_once(it, dconf, nconf)
                per_image.append(1e3 * (time.perf_counter() - t0))
        numpy_ms = statistics.median(per_image)
        for n in (1, 8, 64):
            batch = items[:n]
            prepare_mono_priors(batch, dconf, nconf)  # warm-up: code objects, allocator blocks of this size
            wall = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                prepare_mono_priors(batch, dconf, nconf)
                wall.append(1e3 * (time.perf_counter() - t0))
            dc, nc = Depth._merged_conf(dconf), Normals._merged_conf(nconf)
            dm, ds = capi.depth_priors([Depth.problem(it["depth_dict"], it["camera"], it["kps"], it["mask"]) for it in batch], dc, return_summary=True)
            _, ns = capi.normal_priors([Normals.problem(it["normals_dict"], it["camera"], it["mask"], m["continuity_mask"]) for it, m in zip(batch, dm)],
                                       nc, return_summary=True)
            row = dict(config=tag, images=n, wall_ms_median=statistics.median(wall), wall_ms_min=min(wall), wall_ms_max=max(wall),
                       kernels_ms=ds["ms"] + ns["ms"], numpy_ms=numpy_ms * n, numpy_ms_per_image_min=min(per_image),
                       numpy_ms_per_image_max=max(per_image), repeats=a.repeats)
            rows.append(row)
            print(json.dumps(row), flush=True)
    print("\n| configuration | images | GPU call, median ms (min - max) | of which kernels, ms | per image, ms | NumPy restatement, ms |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['config']} | {r['images']} | {r['wall_ms_median']:.1f} ({r['wall_ms_min']:.1f} - {r['wall_ms_max']:.1f}) | {r['kernels_ms']:.2f} | "
              f"{r['wall_ms_median'] / r['images']:.2f} | {r['numpy_ms']:.0f} |")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
