"""The decision kernels of the trust-region loop (k_lm_decide, k_lm_reduce_decide: csrc/ba_kernels.hip, csrc/lm_decide.h) one launch at
a time through mpsfm_debug_lm_decide, on the table of tests/lm_control_cases.py: every row in three forms (the scalars given; cost, invalid
count and landmark gradient from the all-reduced tail; everything reduced from partial tables of 1 ... 5000 rows), against the row's
hand-written literals and, field by field, against the restatement.  Integers and doubles that are copies, halvings or sums of exact
inputs are compared exactly; the four quantities behind the device's sqrt, its division and 1 - u^3 (radius after an accepted step, x_norm,
last_step_norm, last_rel) in ulps of a 60-digit evaluation.  Then the reduction on random tables and the host copy's two sizes."""

import ctypes as C
import math

import numpy as np
import pytest

import lm_control_cases as LC
from mpsfm_amd import capi
from mpsfm_amd.abi import CDebugLmCtl, CDebugLmOpts

pytestmark = pytest.mark.gpu

K = capi.debug_lm_constants()  # (no device involved)
HEAD, CTL, SLOTS, THREADS = K["head_bytes"], K["ctl_bytes"], K["redsc_slots"], K["reduce_threads"]
REDUCE_ROWS = (1, 63, 64, 65, THREADS - 1, THREADS, THREADS + 1, 5000)
RANK0 = 8  # first rank slot of the tail (SC_RANK0)
FILL = 0xA5
PAD = 0x5A5A5A5A
ULP_FIELDS = ("radius", "x_norm", "last_step_norm", "last_rel")
# Largest distance from the 60-digit value measured over the table in all twelve forms on MI355X (every run prints it; DESIGN.md section
# 4b-1): last_rel 0.241 ulp and last_step_norm 0.5 ulp (one correctly rounded operation), x_norm 0.544 ulp (a rounded sum under the
# root), radius 1.094 ulp (five roundings behind the rounded gain ratio) - the distances of IEEE binary64 on the host for the same rows.
# The bound is twice the measured distance.
ULP_BOUND = {"radius": 2.188, "x_norm": 1.088, "last_step_norm": 1.0, "last_rel": 0.482}
MEASURED = {f: 0.0 for f in ULP_FIELDS}


def _ctl(block):
    c = CDebugLmCtl()
    for f in LC.HEAD_DOUBLES + LC.HEAD_INTS:
        setattr(c, f, block[f])
    c.pad_ = PAD
    for i in range(LC.MAX_TRACE):  # what a launch must leave alone where it writes no entry
        c.trace_cost[i], c.trace_radius[i], c.trace_accepted[i] = -1000.0 - i, -2000.0 - i, 100 + i
    return c


def _opts(o):
    c = CDebugLmOpts()
    for f, v in o.items():
        setattr(c, f, v)
    return c


def _scal(s):
    v = np.array([900.0 + i for i in range(16)])  # slots 12-15 are not a decision's
    for name, slot in LC.SCALAR_SLOTS.items():
        v[slot] = s[name]
    return v


def _bytes(c):
    return bytes(C.string_at(C.addressof(c), C.sizeof(c)))


def _same(a, b):
    return (a != a and b != b) or (a == b and math.copysign(1.0, a) == math.copysign(1.0, b))


def _split(v, rows, rng):
    """`rows` addends whose sum in any order is exactly v: halves of a finite value in two rows, zeros elsewhere."""
    col = np.zeros(rows)
    if rows >= 2 and math.isfinite(v) and abs(v) > 1e-290:
        i, j = rng.choice(rows, 2, replace=False)
        col[i] = col[j] = 0.5 * v
    else:
        col[rng.integers(rows)] = v
    return col


def _count(v, rows, rng):
    col = np.zeros(rows)
    for _ in range(int(v)):
        col[rng.integers(rows)] += 1.0
    return col


def _inputs(r, form, arg):
    """(scal, extra keyword arguments of debug_lm_decide, the scalars the decision must see, the slots of scal the launch writes)."""
    s = dict(r["scalars"])
    rng = np.random.default_rng(len(r["name"]) + 97 * int(arg or 0))
    gp = s["gmax_pts"]
    if form != "scalars":  # the maximum is folded from 0 with fmax: a NaN entry is ignored
        s["gmax_pts"] = 0.0 if gp != gp else max(0.0, gp)
    if form == "scalars":
        return _scal(s), {}, s, ()
    if form == "redsc":
        scal = _scal({**s, "x_cost": -777.0, "x_bad": 55.0, "gmax_pts": 1e300})  # the launch must replace them
        redsc = np.array([700.0 + i for i in range(SLOTS)])  # slots 3-7 are nobody's
        redsc[0], redsc[1], redsc[2] = s["x_cost"], s["x_bad"], 4e300  # (SC_GMAX_PTS itself is zero after k_gmax_to_slot and never read)
        redsc[RANK0:] = [0.5 * gp if (math.isfinite(gp) and gp > 0) else 0.0 for _ in range(SLOTS - RANK0)]
        redsc[RANK0 + arg] = gp
        return scal, dict(redsc=redsc), s, (8, 9, 10)
    rows = arg
    scal = _scal({**s, "x_cost": -777.0, "x_bad": 55.0, "gmax_pts": 1e300, "cand": -778.0, "bad": 56.0, "mcc": -779.0, "step_sq_pts": -780.0,
                  "xn_sq_pts": -781.0})
    part, part2 = np.zeros((rows, 4)), np.zeros((rows, 8))
    part[:, 0], part[:, 1] = _split(s["x_cost"], rows, rng), _count(s["x_bad"], rows, rng)
    part[:, 2] = 0.5 * gp if (math.isfinite(gp) and gp > 0) else 0.0
    part[rng.integers(rows), 2] = gp
    part[:, 3] = 1e305  # not a column of the reduction
    part2[:, 0], part2[:, 1], part2[:, 2] = _split(s["cand"], rows, rng), _count(s["bad"], rows, rng), _split(s["mcc"], rows, rng)
    part2[:, 3], part2[:, 4] = _split(s["step_sq_pts"], rows, rng), _split(s["xn_sq_pts"], rows, rng)
    part2[:, 5:] = 1e305
    return scal, dict(part=part, part2=part2), s, (8, 9, 10, 0, 1, 2, 3, 4)


def _check_row(r, form, arg):
    scal_in, extra, seen, written_slots = _inputs(r, form, arg)
    ctl_in = _ctl(r["block"])
    dev, host, scal_out = capi.debug_lm_decide(ctl_in, _opts(r["options"]), scal_in, form, fill=FILL, **extra)
    want, written = LC.lm_step(r["block"], seen, r["options"])
    exact = LC.exact_quantities({**r, "scalars": seen})
    literal = r["expected"] if all(_same(seen[k], r["scalars"][k]) for k in seen) else None
    name = (r["name"], form, arg)

    def close(field, got, ref):
        if field in ULP_FIELDS and exact[field] is not None and not _same(got, ref):
            d = LC.ulp_distance(got, exact[field])
            MEASURED[field] = max(MEASURED[field], d)
            assert d <= ULP_BOUND[field], (name, field, got, ref, d)
        else:
            if field in ULP_FIELDS and exact[field] is not None:
                MEASURED[field] = max(MEASURED[field], LC.ulp_distance(got, exact[field]))
            assert _same(got, ref), (name, field, got, ref)

    # ---- the block against the restatement, every field
    for f in LC.HEAD_INTS:
        assert getattr(dev, f) == want[f], (name, f, getattr(dev, f), want[f])
    for f in LC.HEAD_DOUBLES:
        close(f, getattr(dev, f), want[f])
    assert dev.pad_ == PAD
    new = {i: (c, rad, a) for i, c, rad, a in written}
    for i in range(LC.MAX_TRACE):
        if i in new:
            assert _same(dev.trace_cost[i], new[i][0]) and dev.trace_accepted[i] == new[i][2], (name, i)
            close("radius" if new[i][2] and i == max(new) and want["accepted"] else "", dev.trace_radius[i], new[i][1])
            if i == max(new):
                assert _same(dev.trace_radius[i], dev.radius), name  # the entry is the block's radius, bit for bit
        else:
            assert (dev.trace_cost[i], dev.trace_radius[i], dev.trace_accepted[i]) == (-1000.0 - i, -2000.0 - i, 100 + i), (name, i)
    # ---- the block against the row's literals
    if literal is not None:
        for f in LC.EXPECTED_FIELDS:
            if f == "trace":
                got = [(dev.trace_cost[i], dev.trace_radius[i], dev.trace_accepted[i]) for i in range(r["block"]["trace_len"], dev.trace_len)]
                assert len(got) == len(literal["trace"]), (name, got)
                for (gc, gr, ga), (wc, wr, wa) in zip(got, literal["trace"]):
                    assert _same(gc, wc) and ga == wa, (name, got)
                    close("radius" if wa and literal["accepted"] else "", gr, wr)
            elif isinstance(literal[f], float):
                close(f, getattr(dev, f), literal[f])
            else:
                assert getattr(dev, f) == literal[f], (name, f, getattr(dev, f), literal[f])
    # ---- the scalars: what the launch writes, and nothing else
    live = r["block"]["term"] == LC.RUNNING
    for slot in range(16):
        ref = scal_in[slot]
        if live and slot in written_slots:
            ref = seen[[k for k, v in LC.SCALAR_SLOTS.items() if v == slot][0]]
        assert _same(float(scal_out[slot]), float(ref)), (name, "scal", slot, scal_out[slot], ref)
    if r["unchanged"]:
        assert _bytes(dev) == _bytes(ctl_in), name
    # ---- the host copy: the head while the solve runs, the whole block with the decision that ends it
    hb, db = _bytes(host), _bytes(dev)
    assert len(hb) == CTL and HEAD == CDebugLmCtl.trace_cost.offset
    if dev.term == LC.RUNNING:
        assert hb[:HEAD] == db[:HEAD] and hb[HEAD:] == bytes([FILL]) * (CTL - HEAD), name
        assert hb[:HEAD] != bytes([FILL]) * HEAD
    else:
        assert hb == db, name


def _forms():
    out = [("scalars", None)] + [("redsc", p) for p in (0, 31, 63)] + [("reduce", n) for n in REDUCE_ROWS]
    return out, [f"{f}-{a}" if a is not None else f for f, a in out]


@pytest.mark.parametrize("form,arg", _forms()[0], ids=_forms()[1])
def test_every_row_in_every_form(form, arg):
    for r in LC.ROWS:
        _check_row(r, form, arg)
    print("ULP measured so far:", {f: round(v, 3) for f, v in MEASURED.items()})


def test_constants_are_the_kernels():
    assert (HEAD, CTL, SLOTS) == (136, C.sizeof(CDebugLmCtl), 72) and THREADS % 64 == 0 and THREADS >= 128


@pytest.mark.parametrize("rows", REDUCE_ROWS)
def test_reduction_of_random_tables(rows):
    """Mixed signs and sixteen decades: the five sums within rows * 2^-52 * sum |a| of math.fsum (the bound of any summation order),
    the maximum and the counts exactly, two launches bit for bit; the decision is the restatement's on the scalars the launch left."""
    rng = np.random.default_rng(rows)
    part = rng.choice([-1.0, 1.0], (rows, 4)) * 10.0 ** rng.uniform(-8, 8, (rows, 4))
    part2 = rng.choice([-1.0, 1.0], (rows, 8)) * 10.0 ** rng.uniform(-8, 8, (rows, 8))
    part[:, 1], part2[:, 1] = rng.integers(0, 4, rows), rng.integers(0, 4, rows)
    block, opts = dict(LC.MID), dict(LC.OPTIONS)
    scal_in = _scal(LC.SCALARS)
    outs = [capi.debug_lm_decide(_ctl(block), _opts(opts), scal_in, "reduce", part=part, part2=part2, fill=FILL) for _ in range(2)]
    (dev, host, scal), (dev2, host2, scal2) = outs
    assert _bytes(dev) == _bytes(dev2) and _bytes(host) == _bytes(host2) and scal.tobytes() == scal2.tobytes()
    for slot, col in ((8, part[:, 0]), (0, part2[:, 0]), (2, part2[:, 2]), (3, part2[:, 3]), (4, part2[:, 4])):
        bound = rows * 2.0 ** -52 * math.fsum(abs(x) for x in col)
        assert abs(scal[slot] - math.fsum(col)) <= bound, (slot, scal[slot], math.fsum(col), bound)
    assert scal[10] == max(0.0, part[:, 2].max()) and scal[9] == part[:, 1].sum() and scal[1] == part2[:, 1].sum()
    for slot in (5, 6, 7, 11, 12, 13, 14, 15):
        assert scal[slot] == scal_in[slot]
    seen = {name: float(scal[slot]) for name, slot in LC.SCALAR_SLOTS.items()}
    want, _ = LC.lm_step(block, seen, opts)
    for f in LC.HEAD_INTS:
        assert getattr(dev, f) == want[f], f
    for f in LC.HEAD_DOUBLES:
        if f not in ULP_FIELDS:
            assert _same(getattr(dev, f), want[f]), f


def test_no_rows_leaves_the_scalars_to_the_caller():
    """rows == 0 (a problem without chunks): nothing is reduced, the decision reads the scalars as they are."""
    r = LC.ROWS[[x["name"] for x in LC.ROWS].index("gain_ratio_half_keeps_the_radius")]
    dev, _, scal = capi.debug_lm_decide(_ctl(r["block"]), _opts(r["options"]), _scal(r["scalars"]), "reduce", part=np.zeros((0, 4)), part2=np.zeros((0, 8)))
    assert scal.tobytes() == _scal(r["scalars"]).tobytes()
    for f in ("term", "accepted", "iter", "n_success"):
        assert getattr(dev, f) == r["expected"][f]


def test_bad_arguments_are_refused():
    with pytest.raises(capi.MpsfmHipError):
        capi.debug_lm_decide(_ctl({**LC.MID, "trace_len": 65}), _opts(LC.OPTIONS), _scal(LC.SCALARS))
    with pytest.raises(capi.MpsfmHipError):
        capi.debug_lm_decide(_ctl({**LC.MID, "trace_len": -1}), _opts(LC.OPTIONS), _scal(LC.SCALARS))
