"""Golden vectors of the 3D-3D alignment produced BY THE REFERENCE'S OWN CODE (tests/golden/alignment.npz).

The reference's icp/main.py reads its dataset at import, so it cannot run.  What can is taken out of /root/reference/icp by AST, as
make_golden_reference.py:extract_functions does (this script only; nothing of the reference travels — the fixture holds
numeric inputs and outputs, no source text):

    icp/depth_to_3d.py   depth_to_3d
    icp/interpolate.py   interpolate
    icp/main.py          rigid_transform_3D, the function nested in the body of the RANSAC loop (:149-175)

Lifting: depth_to_3d + interpolate at 200 keypoints of a 37 x 53 and of a 5 x 4 map, all inside the maps (the reference indexes
out of range elsewhere).  Fit: rigid_transform_3D on 50 random triples, on sets of 4, 10, 100 and 1000 points with 1 % noise and
on one mirrored set (tgt = diag(1, 1, -1) src + noise) that takes the reference's reflection fix.

Run in the build container:  python tests/golden/make_golden_alignment.py
"""
import ast
import os

import numpy as np

from make_golden_reference import REF, extract_functions

HERE = os.path.dirname(os.path.abspath(__file__))


def extract_nested_function(rel, name):
    """One function defined anywhere inside a reference file (here: inside a loop body), compiled on its own with numpy only."""
    tree = ast.parse(open(os.path.join(REF, rel)).read())
    found = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == name]
    assert len(found) == 1, f"{name} occurs {len(found)} times in {rel}"
    mod = ast.Module(body=found, type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = {"np": np}
    exec(compile(mod, rel, "exec"), ns)
    return ns[name]


def random_rotation(rng):
    a = rng.normal(size=3)
    ang = rng.uniform(0.1, 3.0)
    k = a / np.linalg.norm(a)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx


def main():
    depth_to_3d = extract_functions("icp/depth_to_3d.py", ("depth_to_3d",))["depth_to_3d"]
    interpolate = extract_functions("icp/interpolate.py", ("interpolate",))["interpolate"]
    rigid_transform_3D = extract_nested_function("icp/main.py", "rigid_transform_3D")
    rng = np.random.default_rng(20240521)
    out = {}

    for tag, (H, W) in {"a": (37, 53), "b": (5, 4)}.items():
        depth = rng.uniform(0.5, 9.0, (H, W))
        intr = [0.9 * W, 0.85 * W, 0.5 * W - 0.3, 0.5 * H + 0.2]
        xy = np.c_[rng.uniform(0, W - 1, 200), rng.uniform(0, H - 1, 200)]
        xy[:4] = [[0.0, 0.0], [W - 2.0, H - 2.0], [1.0, 0.5], [0.25, 1.0]]  # integer coordinates: a zero weight
        pcd = depth_to_3d(depth, intr).reshape(H, W, 3)
        out[f"lift_{tag}_depth"], out[f"lift_{tag}_intr"], out[f"lift_{tag}_xy"] = depth, np.array(intr), xy
        out[f"lift_{tag}_xyz"] = np.array([interpolate(pcd, float(x), float(y)) for x, y in xy])

    def record(tag, P, Q):
        R, t = rigid_transform_3D(P, Q)
        out[f"fit_{tag}_src"], out[f"fit_{tag}_tgt"], out[f"fit_{tag}_R"], out[f"fit_{tag}_t"] = P, Q, R, t

    box_lo, box_hi = [-2.0, -1.5, 0.5], [2.0, 1.5, 6.0]
    triples = []
    for _ in range(50):
        P = rng.uniform(box_lo, box_hi, (3, 3))
        Q = P @ random_rotation(rng).T + rng.normal(size=3) + rng.normal(size=(3, 3)) * 0.01
        triples.append((P, Q, *rigid_transform_3D(P, Q)))
    for k, name in enumerate(("src", "tgt", "R", "t")):
        out[f"fit_triples_{name}"] = np.array([tr[k] for tr in triples])
    for n in (4, 10, 100, 1000):
        P = rng.uniform(box_lo, box_hi, (n, 3))
        record(str(n), P, P @ random_rotation(rng).T + rng.normal(size=3) + rng.normal(size=(n, 3)) * 0.01)
    P = rng.uniform(box_lo, box_hi, (100, 3))
    record("mirrored", P, P * [1.0, 1.0, -1.0] + rng.normal(size=(100, 3)) * 0.01)
    assert np.linalg.det(out["fit_mirrored_R"]) > 0

    path = os.path.join(HERE, "alignment.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
