"""Times the batched descriptor matcher on two scenes:

  50 images x 2 048 x 256, 20 neighbours each       100 images x 4 096 x 256, 10 neighbours each

both deduplicated by find_unique_new_pairs (500 pairs each), from host arrays and from device tensors.  Yardsticks on the same
inputs: the loop of single match_descriptors calls, on this build and (--parent DIR: a directory that holds the mpsfm_amd package
of the parent commit with its built library) on the parent's, run in a child process of its own; and the reference's torch
expression per pair (scripts/time_descriptor_matches.py).  Medians of 7 calls after 2 warm-ups; wall time is the whole Python
call over all pairs ending in a device synchronise, device time the calls' own HIP-event time.  Every timed batch is compared
with the single calls, matches and scores bitwise: a mismatch voids the number and the script fails.

  python scripts/time_descriptor_matches_batch.py [--out FILE.json] [--quick] [--parent DIR]
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--quick", action="store_true", help="small scenes: a rehearsal of the script, not a measurement")
ap.add_argument("--parent", help="directory holding the parent commit's mpsfm_amd package with its built library")
ap.add_argument("--root", help=argparse.SUPPRESS)        # child: where mpsfm_amd is imported from
ap.add_argument("--loop-scene", type=int, help=argparse.SUPPRESS)  # child: time the loop of single calls on this scene only
ARGS = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(ARGS.root) if ARGS.root else ROOT)
import torch  # noqa: E402
from mpsfm_amd import capi  # noqa: E402

WARMUP, CALLS = 2, 7
RATIO = 0.9
SCENES = [(50, 2048, 256, 10), (100, 4096, 256, 5)]  # images, descriptors, dim, neighbours on each side
QUICK = [(12, 300, 32, 3), (8, 520, 64, 2)]


def find_unique_new_pairs(pairs_all):  # the rule of mpsfm_amd.extraction.pairwise.match_sparse, restated: the parent has no such module
    taken, pairs = set(), []
    for i, j in pairs_all:
        if (j, i) not in taken and (i, j) not in taken:
            taken.add((i, j))
            pairs.append((i, j))
    return pairs


def scene(k, quick):
    """views of one scene: every image holds noisy, shuffled copies of two thirds of a common set, the rest has no counterpart"""
    n_img, n, dim, nb = (QUICK if quick else SCENES)[k]
    rng = np.random.default_rng(4100 + k)
    base = rng.normal(size=(n, dim)).astype(np.float32)
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    descs, m = [], (2 * n) // 3
    for _ in range(n_img):
        x = rng.normal(size=(n, dim)).astype(np.float32)
        x[:m] = base[rng.permutation(n)[:m]] + np.float32(0.3 / np.sqrt(dim)) * rng.normal(size=(m, dim)).astype(np.float32)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        descs.append(x / np.float32(1.0 + 2.0 ** -20))
    pairs = find_unique_new_pairs([(i, (i + s) % n_img) for i in range(n_img) for s in range(-nb, nb + 1) if s])
    return descs, pairs


def digest(ms, ss):
    h = hashlib.sha256()
    for m, s in zip(ms, ss):
        h.update(np.ascontiguousarray(m, np.int64).tobytes())
        h.update(np.ascontiguousarray(s, np.float64).tobytes())
    return h.hexdigest()


def timed(fn):
    """fn() -> (matches, scores, device ms); medians of wall and device ms over CALLS calls"""
    wall, dev, res = [], [], None
    for it in range(WARMUP + CALLS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ms, ss, d = fn()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if it >= WARMUP:
            wall.append(1e3 * (t1 - t0))
            dev.append(d)
        res = (ms, ss)
    return res, statistics.median(wall), statistics.median(dev)


def loop(descs, pairs):
    ms, ss, dev = [], [], 0.0
    for i, j in pairs:
        m, s, info = capi.match_descriptors(descs[i], descs[j], RATIO, return_info=True)
        ms.append(m), ss.append(s)
        dev += info["ms"]
    return ms, ss, dev


def loop_rows(k, quick, build):
    descs, pairs = scene(k, quick)
    tens = [torch.from_numpy(d).cuda() for d in descs]
    rows = []
    for path, d in (("host arrays", descs), ("device tensors", tens)):
        (ms, ss), wall, dev = timed(lambda: loop(d, pairs))
        rows.append(dict(call=f"loop of match_descriptors, {build}", scene=k, pairs=len(pairs), path=path, wall_ms=wall, device_ms=dev,
                         matched=int(sum((m >= 0).sum() for m in ms)), digest=digest(ms, ss)))
    return rows


def torch_loop(tens, pairs):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from time_descriptor_matches import torch_match

    ms, ss = [], []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i, j in pairs:
        m, s = torch_match(tens[i], tens[j], RATIO)
        ms.append(m), ss.append(s)
    e1.record()
    torch.cuda.synchronize()
    return ms, ss, e0.elapsed_time(e1)  # left on the device, as scripts/time_descriptor_matches.py times the expression


def main():
    if not torch.cuda.is_available() or capi.device_count() < 1:
        raise SystemExit("no device: nothing here is measured without one")
    if ARGS.loop_scene is not None:  # the child of a --parent run
        print(json.dumps(loop_rows(ARGS.loop_scene, ARGS.quick, "parent build")), flush=True)
        return
    rows, void = [], False
    for k in range(2):
        descs, pairs = scene(k, ARGS.quick)
        tens = [torch.from_numpy(d).cuda() for d in descs]
        single = loop_rows(k, ARGS.quick, "this build")
        rows += single
        want = single[0]["digest"]
        assert single[1]["digest"] == want

        def ours(d):
            ms, ss, info = capi.match_descriptors_batch(d, pairs, RATIO, return_info=True)
            assert info["num_syncs"] == 1
            return ms, ss, info

        for path, d in (("host arrays", descs), ("device tensors", tens)):
            last = {}

            def fn():
                ms, ss, info = ours(d)
                last.update(info)
                return ms, ss, info["ms"]

            (ms, ss), wall, dev = timed(fn)
            same = digest(ms, ss) == want
            void = void or not same
            rows.append(dict(call="match_descriptors_batch", scene=k, pairs=len(pairs), path=path, wall_ms=wall, device_ms=dev,
                             matched=int(last["num_matches"]), groups=last["num_groups"], launches=last["num_launches"],
                             workgroups=last["num_workgroups"], equals_single_calls=same))
        (tm, _), wall, dev = timed(lambda: torch_loop(tens, pairs))
        ref = loop(descs, pairs)[0]
        rows.append(dict(call="loop of the torch expression", scene=k, pairs=len(pairs), path="device tensors", wall_ms=wall, device_ms=dev,
                         rows_that_differ_from_ours=int(sum((a.cpu().numpy() != b).sum() for a, b in zip(tm, ref)))))
        if ARGS.parent:
            cmd = [sys.executable, os.path.abspath(__file__), "--root", ARGS.parent, "--loop-scene", str(k)] + (["--quick"] if ARGS.quick else [])
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise SystemExit("the parent's loop failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
            parent = json.loads(r.stdout.strip().splitlines()[-1])
            for row in parent:
                row["equals_this_build"] = row["digest"] == want
                void = void or not row["equals_this_build"]
            rows += parent
        for row in rows:
            if row["scene"] == k and not row.get("printed"):
                row["printed"] = True
                print(json.dumps({a: b for a, b in row.items() if a not in ("digest", "printed")}), flush=True)
    for row in rows:
        row.pop("printed", None)
    if ARGS.out:
        os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
        with open(ARGS.out, "w") as f:
            json.dump(rows, f, indent=1)
    if void:
        raise SystemExit("a timed result differs from the single calls: the numbers are void")


if __name__ == "__main__":
    main()
