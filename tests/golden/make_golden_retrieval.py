"""Fixture for the pair stages (tests/golden/reference_retrieval.npz), computed BY THE REFERENCE'S OWN CODE:

  mpsfm/extraction/pairs/hloc/pairs_from_retrieval.py    pairs_from_score_matrix, parse_names
  mpsfm/extraction/pairs/hloc/pairs_from_exhaustive.py   main
  mpsfm/extraction/pairs/base.py                         pairs_from_sequential

The functions are extracted by AST (their modules import h5py at the top), annotations dropped; the similarity is the
reference's torch.einsum("id,jd->ij", q.float(), db.float()) on the CPU.  What pairs_from_retrieval.main does around them (names of
the feature files, name2db, the self mask, names of the pairs, the text file) reads HDF5 and is repeated here on mappings.

Descriptors: a clustered scene of a few places, images of one place share a direction; stored as float16 (so float16, float32 and
fp64 readers see the same values) with norm <= 1.

Cases, query x db x D, num_matched:
  same20      150 x 150 x 64, 20, same names        the self mask
  same5       the same with 5
  disjoint    90 x 170 x 64, 20, disjoint names     no self mask
  clipped     40 x 40 x 32, 60, same names          k clips to 40; every row's list ends at the score test
  quirk       12 x 30 x 32, 20                      k = min(20, 12): the number of QUERY images
  names_*     name lists with a prefix, an explicit list, a tuple of prefixes and two db mappings sharing a name
For every case (asserted here): rows whose decision margin (tests/numpy_retrieval.py) is below tau32 = 4 D 2^-24 are at most 5 %;
on all other rows the reference's list equals the fp64 restatement's exactly, element for element and in order; the reference's
float32 scores agree to tau32.
  sequential  overlap 1 and 3, quadratic_overlap on and off, n = 1, 2, 9
  exhaustive  self-matching and ref_list, n = 1, 2, 9
The file holds inputs and outputs only.

Run in the build container:  python tests/golden/make_golden_retrieval.py
"""
import ast
import collections.abc
import json
import os
import sys
import tempfile
from pathlib import Path
from typing import Optional, Union

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_reference import REF, ROOT  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy_retrieval as NR  # noqa: E402


def extract(rel, names):
    """Selected top-level functions of one reference file, compiled without the module's imports and without annotations."""
    tree = ast.parse(open(os.path.join(REF, rel)).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert len(body) == len(names), (rel, names)
    for fn in body:
        fn.returns = None
        for a in fn.args.args + fn.args.kwonlyargs:
            a.annotation = None
    mod = ast.Module(body=body, type_ignores=[])
    ast.fix_missing_locations(mod)

    def no_files(*a, **k):
        raise AssertionError("the fixture passes lists, not files")

    ns = dict(np=np, torch=torch, Path=Path, collections=collections.abc, Iterable=collections.abc.Iterable, Optional=Optional, Union=Union,
              parse_image_lists=no_files, list_h5_names=no_files)
    exec(compile(mod, rel, "exec"), ns)
    return ns


def places(rng, sizes, D, spread):
    """unit descriptors of len(sizes) places: the images of a place share a direction; float16, norm <= 1; shuffled"""
    x = []
    for n in sizes:
        u = rng.normal(size=D)
        u /= np.linalg.norm(u)
        x.append(u + spread * rng.normal(size=(n, D)) / np.sqrt(D))
    x = np.concatenate(x)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x = (x[rng.permutation(len(x))] * (1 - 2.0 ** -8)).astype(np.float16)
    assert np.linalg.norm(x.astype(np.float64), axis=1).max() <= 1
    return x


def reference_pairs(ref, q, db, q_names, db_names, num_matched):
    """pairs_from_retrieval.main between get_descriptors and the text file: (pairs [n, 2], float32 scores of the pairs)"""
    sim = torch.einsum("id,jd->ij", torch.from_numpy(q).float(), torch.from_numpy(db).float())
    kept = sim.clone()
    self_mask = np.array(q_names)[:, None] == np.array(db_names)[None]
    pairs = ref["pairs_from_score_matrix"](sim, self_mask, num_matched, min_score=0)
    pairs = np.array([(int(i), int(j)) for i, j in pairs], np.int64).reshape(-1, 2)
    return pairs, kept.numpy()[pairs[:, 0], pairs[:, 1]]


def check_case(tag, q, db, q_names, db_names, num_matched, pairs, scores):
    """the conditions the fixture rests on"""
    D = q.shape[1]
    k = min(num_matched, len(q))
    qi, di = NR.name_ids(q_names, db_names)
    idx, val, cnt, margin = NR.retrieve_topk(q, db, k, 0.0, qi, di)
    t32 = NR.tau(D, NR.TAU32_EPS)
    sure = margin > t32
    worst = 0.0
    for i in range(len(q)):
        if not sure[i]:
            continue
        mine = pairs[pairs[:, 0] == i]
        assert mine[:, 1].tolist() == idx[i, :cnt[i]].tolist(), (tag, i)
        if len(mine):
            worst = max(worst, np.abs(scores[pairs[:, 0] == i].astype(np.float64) - val[i, :cnt[i]]).max())
    print(tag, "k", k, "pairs", len(pairs), "below tau32", (~sure).sum(), f"of {len(q)} ({(~sure).mean():.3%})", "score diff", worst, "tau32", t32,
          "counts", cnt.min(), cnt.max())
    assert (~sure).mean() <= 0.05 and worst <= t32
    return cnt


def text_of(pairs):
    return "\n".join(" ".join([a, b]) for a, b in pairs)


def main():
    ref = extract("mpsfm/extraction/pairs/hloc/pairs_from_retrieval.py", ("pairs_from_score_matrix", "parse_names"))
    exh = extract("mpsfm/extraction/pairs/hloc/pairs_from_exhaustive.py", ("main",))["main"]
    seq = extract("mpsfm/extraction/pairs/base.py", ("pairs_from_sequential",))["pairs_from_sequential"]
    rng = np.random.default_rng(20241101)
    out = {}

    def names(prefix, n):
        return [f"{prefix}{i:03d}.jpg" for i in range(n)]

    # ---- descriptor cases
    a = places(rng, [30] * 5, 64, 1.0)
    same = names("scene/im", 150)
    x = places(rng, [52] * 5, 64, 1.0)
    cq, cdb = x[:90], x[90:]
    c = places(rng, [8] * 5, 32, 1.0)
    e = places(rng, [14] * 3, 32, 1.0)
    cases = [("same20", a, a, same, same, 20), ("same5", a, a, same, same, 5),
             ("disjoint", cq, cdb, names("query/q", 90), names("db/d", 170), 20),
             ("clipped", c, c, names("im", 40), names("im", 40), 60),
             ("quirk", e[:12], e[12:], names("q", 12), names("d", 30), 20)]
    for tag, q, db, qn, dn, num in cases:
        pairs, scores = reference_pairs(ref, q, db, qn, dn, num)
        cnt = check_case(tag, q, db, qn, dn, num, pairs, scores)
        if tag == "same20":
            assert (cnt == 20).all()
        if tag == "clipped":  # every list ends at the score test: shorter than the 39 columns the self mask leaves
            assert min(num, len(q)) == 40 and cnt.max() < 39 and cnt.min() >= 1
        if tag == "quirk":
            assert (cnt == 12).all()
        out.update({f"{tag}_query": q, f"{tag}_db": db, f"{tag}_query_names": np.array(qn), f"{tag}_db_names": np.array(dn),
                    f"{tag}_num_matched": np.array(num), f"{tag}_pairs": pairs, f"{tag}_scores": scores})

    # ---- name cases: three mappings; "shared/s0" is in both db mappings with different descriptors, the last one wins
    y = places(rng, [13] * 4, 32, 1.0)
    maps = {"queries": names("query/q", 10) + names("db/a", 5) + ["other/x0.jpg"],
            "dbA": names("db/a", 20) + ["shared/s0.jpg"],
            "dbB": names("db/b", 14) + ["shared/s0.jpg"]}
    at = 0
    for m, nm in maps.items():
        out[f"map_{m}_names"], out[f"map_{m}_desc"] = np.array(nm), y[at:at + len(nm)]
        at += len(nm)
    assert at <= len(y)
    for i in range(5):  # the query mapping's copies of db images hold the db descriptors
        out["map_queries_desc"][10 + i] = out["map_dbA_desc"][i]
    name_cases = [dict(tag="names_prefix", num_matched=5, query_prefix="query", query_list=None, db_prefix=None, db_list=None, dbs=["dbA", "dbB"]),
                  dict(tag="names_list", num_matched=4, query_prefix=None, query_list=["db/a003.jpg", "query/q002.jpg", "db/a000.jpg", "other/x0.jpg"],
                       db_prefix=["db/a", "shared"], db_list=None, dbs=["dbA", "dbB"]),
                  dict(tag="names_all", num_matched=3, query_prefix=None, query_list=None, db_prefix=None, db_list=None, dbs=None),
                  dict(tag="names_db_list", num_matched=6, query_prefix=["query", "other"], query_list=None, db_prefix=None,
                       db_list=["db/b001.jpg", "shared/s0.jpg", "db/a002.jpg", "db/b007.jpg", "db/a010.jpg", "db/b003.jpg", "db/a019.jpg"], dbs=["dbB", "dbA"])]
    for case in name_cases:
        dbs = case["dbs"] or ["queries"]
        name2db = {n: i for i, m in enumerate(dbs) for n in maps[m]}
        db_names = ref["parse_names"](case["db_prefix"], case["db_list"], list(name2db.keys()))
        q_names = ref["parse_names"](case["query_prefix"], case["query_list"], list(maps["queries"]))
        desc_of = lambda m, n: out[f"map_{m}_desc"][maps[m].index(n)]  # noqa: E731
        db = np.stack([desc_of(dbs[name2db[n]], n) for n in db_names])
        q = np.stack([desc_of("queries", n) for n in q_names])
        pairs, scores = reference_pairs(ref, q, db, q_names, db_names, case["num_matched"])
        check_case(case["tag"], q, db, q_names, db_names, case["num_matched"], pairs, scores)
        named = [(q_names[i], db_names[j]) for i, j in pairs]
        assert all(a != b for a, b in named)
        case.update(query_names=q_names, db_names=db_names, pairs=named, text=text_of(named))
    shared = [c for c in name_cases if c["dbs"] and any(b == "shared/s0.jpg" for _, b in c["pairs"])]
    assert shared, "no case lists the shared name"
    out["name_cases"] = np.array(json.dumps(name_cases))

    # ---- host-only stages
    host = []
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "pairs.txt")
        for n in (1, 2, 9):
            nm = [f"f{(7 * i) % 10}_{i}.png" for i in range(n)]  # not in alphabetical order
            for overlap in (1, 3):
                for quad in (True, False):
                    pairs = seq(path, image_list=nm, overlap=overlap, quadratic_overlap=quad)
                    host.append(dict(kind="sequential", names=nm, overlap=overlap, quadratic_overlap=quad, pairs=[list(p) for p in pairs],
                                     text=open(path).read()))
            exh(path, image_list=nm)
            text = open(path).read()
            host.append(dict(kind="exhaustive", names=nm, ref=None, pairs=[p.split() for p in text.split("\n") if p], text=text))
            refs = [f"r{i}.png" for i in range(3)] + nm[:1]
            exh(path, image_list=nm, ref_list=refs)
            text = open(path).read()
            host.append(dict(kind="exhaustive", names=nm, ref=refs, pairs=[p.split() for p in text.split("\n") if p], text=text))
    seqs = [h for h in host if h["kind"] == "sequential"]  # the quadratic jumps add pairs somewhere
    assert any(h["quadratic_overlap"] and not g["quadratic_overlap"] and g["names"] == h["names"] and g["overlap"] == h["overlap"]
               and len(h["pairs"]) > len(g["pairs"]) for h in seqs for g in seqs)
    out["host_cases"] = np.array(json.dumps(host))

    path = os.path.join(HERE, "reference_retrieval.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: (v.shape, str(v.dtype)) for k, v in out.items()})
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
