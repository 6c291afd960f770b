"""mpsfm_triangulate_tracks, mpsfm_filter_tracks, mpsfm_point_covs, mpsfm_tri_estimate_batch and
mpsfm_init_pair_candidates against the exact reference of
tests/exact_geometry.py (mpmath, 60 digits; validated on the CPU by tests/test_exact_geometry_cpu.py), at the shapes and
edges where the kernels can go wrong.  The case sets and the comparison functions live in exact_geometry.py; the same
functions ran the C oracle with one arithmetic step altered at a time, and every alteration that can change an output
was flagged.

Criteria (eps = 2^-52; every form comes from rounding analysis, every constant is measured)

  triangulation, backward   v = (X, 1) / |(X, 1)|:  |A v - (v'Av) v| <= C_t eps |A|_F  and  v'Av <= lambda_min + C_t eps |A|_F
  triangulation, forward    |X - X_ref| <= C_t eps |A|_F / (lambda_2 - lambda_1) (1 + |X|) sqrt(1 + |X|^2), asserted where
                            that bound is at most 1e-6 (1 + |X_ref|) ("informative")
  angle                     |ang - ang_ref| <= C_a eps kappa per camera pair
  squared error             |e - e_ref| <= C_e eps (e_ref + s)
  covariance                |cov - cov_ref|_F <= C_p eps cond(H) |cov_ref|_F; NaN only where C_p eps cond(H) >= 1
  front, short tracks, landmarks with fewer than two observations: exact

Informative (forward bound asserted): every friendly track (2, 3, 5, 64, 200 views, shuffled cameras, both intrinsics
rows, the block-edge launches), the large rotations, the 1e-2 low-parallax pair with and without noise; as it happens
also the 1e-3 and 1e-4 pairs (their cameras sit at the origin, so |A|_F is small), the scene scaled by 1e-3, the same
camera twice with two pixels and the noisy pure rotation.  Backward criterion alone: the point 1e6 baselines away, the
scenes translated by 1e3 / 1e4 and scaled by 1e3, the rank-deficient tracks (same camera and pixel twice, exact pure
rotation) where the output is finite.

kappa, the first-order condition of the law-of-cosines angle.  The kernel forms C = -R^T t for both cameras, then
d1 = X - C1, d2 = X - C2, b = C1 - C2, the squares r1 = |d1|^2, r2 = |d2|^2, b2 = |b|^2 and cs = (r1 + r2 - b2) / den with
den = 2 sqrt(r1 r2).  C carries an absolute error of a few eps |C|, so the differences carry the relative errors
eps g1, eps g2, eps gb with g1 = (|X| + |C1|) / |d1|, g2 = (|X| + |C2|) / |d2|, gb = (|C1| + |C2|) / |b|: the cancellation
in X - C and C1 - C2 relative to |C| and |X|.  The squares double them.  The numerator of cs is a sum of three terms of
magnitudes r1, r2, b2, each with its own relative error and one more rounding per addition; den carries eps (g1 + g2 + 1).
To first order

  |d cs| <= eps [ (2 g1 r1 + 2 g2 r2 + 2 gb b2 + r1 + r2 + b2) / den + |cs| (g1 + g2 + 2) ]

which is the (r1 + r2) / den of the law of cosines times the cancellation factors.  acos has the slope 1 / sin(ang); at
ang -> 0 or pi the square root takes over, |d ang| <= sqrt(2 |d cs|), which the slope 1 / max(sin(ang), sqrt(eps))
covers.  Folding to [0, pi/2] does not amplify.  So kappa = [...] / max(sin(ang), sqrt(eps)), evaluated in mpmath at
the exact angle.  The kernel returns the maximum over the pairs of a track: with every pair within its own
C_a eps kappa_i, the maximum lies in [max_i (ang_i - C_a eps kappa_i), max_i (ang_i + C_a eps kappa_i)], which is what
is asserted (no looser than the largest kappa of the track).

Squared error: du = fx xc / zc + cx - u sums terms of the magnitudes m_u = fx / |zc| (|R_0| |X| + |t_0| + |xc / zc| (|R_2| |X| + |t_2|))
+ |cx| + |u| (the terms that cancel in R X + t, the principal point, the pixel), so |d du| <= c eps m_u and
|d e| <= 2 |du| c eps m_u + ... <= c eps (e + m_u^2 + m_v^2): s = m_u^2 + m_v^2.

Measured ratios, error / (eps x form), largest over exactly the cases of this file.  The constant is 8 x the NumPy
figure (np.linalg.eigh / np.linalg.inv / np.arccos on the same fp64 inputs) rounded up to a power of two; the factor
8 is for the device's contracted FMAs, its acos and sqrt, the Jacobi sweeps and the free order of the atomics.  The C
oracle (the kernels' arithmetic, Jacobi and Cholesky included) stands beside it for information.
`PYTHONPATH=. python tests/exact_geometry.py` prints the table.

  quantity                     NumPy    C oracle   constant
  triangulation, backward      1.96     1.34       C_t = 16   (largest of the two triangulation rows)
  triangulation, forward       0.691    0.264
  angle                        0.108    0.108      C_a = 1
  squared error                0.220    0.220      C_e = 2
  covariance                   13.5     7.84       C_p = 128  (the 5000-observation landmark; 0.96 elsewhere)

Candidate tracks (mpsfm_tri_estimate_batch) and init-pair points (mpsfm_init_pair_candidates)

The reference is exact_loransac of exact_geometry.py: the loop of tri_ransac_scratch walked with exact arithmetic
(lexicographic pairs, tri_estimate's depth and angle tests, support by count then residual sum, local optimisation from
more than two inliers for up to ten rounds while the count grows, the tri_num_trials stop rule with min_num_trials, the
final mask).  The two-view sample model is the smallest eigenvector of the exact A2 = sum row^T row over the four
unnormalised rows x P_2 - P_0, y P_2 - P_1 of tri_two_view; the multi-view model is triangulation_matrix's form on the
inlier set.  The walk of a 64-view candidate costs thousands of models, so tests/golden/exact_candidates.npz holds the
inputs and what the walk found (made by tests/golden/make_golden_exact_candidates.py; the CPU file walks a handful again).

Margin.  Every comparison on the exact path is at a distance from its threshold; the margin of the comparison is that
distance over a bound of the error the device can make in the compared quantity, and the margin of the candidate is the
smallest of them.  Above 1 the candidate is decided: ok and the mask are asserted exactly, the point by the backward
criterion above on the matrix of the exact index set, and by the forward criterion where informative.  Otherwise it is
open: ok = 0 with zeros or ok = 1 with a finite point and at least two inliers.  A bound has two parts.

  1. The quantity's own rounding at a given point X, C eps form:
     depth             form = sum_j |P_2j X_j| + |t_2|: the terms that cancel in zc                              (C_z)
     triangulation     form = kappa of the pair, above                                                          (C_a)
       angle
     sq. reprojection  form = e + s, above; the threshold max_error^2 is itself rounded: + eps max_error^2       (C_e)
     angular residual  e = acos(cs), cs = a.b / (|a| |b|), a = (xn, 1), b = P X.  b_k sums terms of the magnitudes
                       m_k = sum_j |P_kj X_j| + |t_k|, so b moves by eps |m| and the angle by eps |m| / |b|, i.e. cs by
                       sin(e) eps |m| / |b|; the products of the dot add eps sum_k |a_k b_k| / (|a| |b|) <= eps, the two
                       norms and the division eps 2 |cs|.  acos has the slope 1 / sin e, and below sqrt(eps) the square
                       root takes over as for kappa:
                         form = [sin(e) |m| / |b| + sum |a_k b_k| / (|a| |b|) + 2 |cs|] / max(sin e, sqrt(eps))
                       The compared quantity is e^2: bound 2 e de + de^2 + eps max_error^2.                      (C_r)
     residual sums     the sum of the bounds of the inliers' residuals + n eps sum; compared only at equal counts
     counts            integers: exact once every residual comparison is decided
     stop rule         v = 3 log(1 - confidence) / log(1 - r^2), r = k / n; 1 - confidence is exact in fp64; r, its square
                       and the difference carry eps (1 + 3 r^2 / denom) relative to denom = 1 - r^2, which the logarithm
                       divides by |log denom|; the rest is a few eps:
                         form = |v| (3 + (1 + 3 r^2 / denom) / |log denom| + 1 / |log(1 - confidence)|)
                       and the margin is the distance of v from the nearest integer (the ceil) over C_s eps form.   (C_s)
  2. The first-order effect of the model's forward error.  A computed v that meets the backward criterion is an
     eigenvector of A + E with |E| <= C_t eps |A|_F, so dv = sum_k c_k v_k over the other eigenvectors with
     |c_k| <= C_t eps |A|_F / (lambda_k - lambda_1), and X = v[:3] / v[3] moves by d_k = c_k (v_k[:3] - X v_k[3]) / v[3] per
     direction.  (Its norm, with every gap replaced by the smallest, is the forward bound above.)  A quantity q with the
     gradient g in X moves by at most sum_k |g . d_k|; g is evaluated in mpmath: the third row of P for the depth,
     -R^T (a^ - cs b^) / (|b| sin e) for e, the sum of the two ray terms for the triangulation angle, 2 du grad du +
     2 dv grad dv for the reprojection error (plus the squares of the first-order terms), and the length bound 1 / |b| or
     1 / |d1| + 1 / |d2| times |d_k| where sin = 0 leaves the gradient without a direction.  Nothing is decided from a model
     whose gap is not above 4 C_t eps |A|_F.
  A false outcome of tri_estimate is as firm as its firmest failing test, a true one as its weakest test; with
  min_tri_angle = 0 the angle test always passes (the device's angle is never negative).

The reference's angle (ref_angle_deg, law of cosines on plain lengths) is compared at the kernel's own point:
c = (r1 + r2 - b) / (2 sqrt(r1 r2)); the lengths carry eps (g + 2) with the g of kappa, so
  dc = [(g1 + 2) r1 + (g2 + 2) r2 + (gb + 2) b] / (2 sqrt(r1 r2)) + |c| ((g1 + g2) / 2 + 5)
and the angle must lie within C_ra eps (dc / max(sin acos c, sqrt(eps)) + angle).  In exact arithmetic |c| <= 1 always
((sqrt r1 - sqrt r2)^2 <= |r1 - r2| <= b <= r1 + r2), so the NaN the reference returns for c > 1 is rounding: it is legal
where 1 - |c| <= C_ra eps dc and nowhere else.  The depth flags are exact where |zc - 2^-52| > C_z eps form.  The lift is
compared with the exact product from the kernel's own d_prior: |L_k - exact_k| <= C_l eps |exact_k|.

The scene translated by 1e4: |A|_F is 1e9 there, C_t eps |A|_F / (lambda_2 - lambda_1) |(X, 1)| allows the point to move
by several 1e-2, and at the rig's own size (depth 10) no comparison of residual sums can be decided from that.  The case is
therefore two views (no sums to compare) of a scene ten times the size, and three views of one three hundred times the size;
five views at the rig's size are decided when translated by 1e3 (shift1e3).  No named case outside the threshold group
is open, and none of the 200 random candidates is.

  quantity                     NumPy    restatement   constant
  two-view point, backward     2.48     9.18          C_t = 16 as above: the issue keeps the criterion unchanged, which is
  two-view point, forward      0.688    4.40          stricter than the 32 the rule would give here (the restatement's
  multi-view point, backward   2.36     2.12          two-view figure is an SVD of the rows with xn rounded first)
  multi-view point, forward    0.622    0.639
  depth                        0.490    0.503         C_z = 4
  angular residual             0.580    0.467         C_r = 8
  squared reprojection         0.0804   0.0621        C_e = 2 as above
  stop rule (all k < n <= 64)  0.361    0.361         C_s = 4
  reference's angle            0.167    0.167         C_ra = 2
  lift                         1.09     1.09          C_l = 16
"""

import numpy as np
import pytest

import exact_geometry as G
from mpsfm_amd import capi
from mpsfm_amd.sfm.scene.observations import reprojection_decisions

pytestmark = pytest.mark.gpu


def _report(stats):
    print({k: f"{v:.3g}" for k, v in G._largest(stats).items()})


def _keep(fn, box):
    """fn, with every result also appended to box: the assertions after the criteria need no second launch."""
    def call(*a):
        box.append(fn(*a))
        return box[-1]

    return call


def test_triangulation_cases():
    """One launch over every case: views per track 2 .. 200, low parallax, translated and scaled scenes, a far point,
    180 degree rotations, negative w, two intrinsics rows, shuffled cameras, repeated cameras, pure rotation, and the
    tracks of fewer than two elements, which are NaN by contract."""
    stats, out = [], []
    fails = G.triangulation_failures(_keep(capi.triangulate_tracks, out), stats=stats)
    _report(stats)
    assert fails == []
    _, groups = G.triangulation_cases()
    xyz = out[0]
    assert np.isnan(xyz[groups["short"]]).all()
    for name in G.TRI_FORWARD_GROUPS + ("same_cam_twice", "pure_rotation_noise", "far_point", "shift1e4", "scale1e3"):
        assert np.isfinite(xyz[groups[name]]).all(), name


@pytest.mark.parametrize("n_tracks", G.BLOCK_EDGES)
def test_triangulation_block_edges(n_tracks):
    """The friendly tracks at n_tracks around the 128 threads of a block."""
    assert G.triangulation_failures(capi.triangulate_tracks, n_tracks) == []


@pytest.mark.parametrize("shift", [0.0, 1e4])
def test_filter_cases(shift):
    """Angles from 1e-7 to 180 degrees with the fold and the exact zeros, the 40-view tracks, squared errors from exact
    projections to 1e4 px and at zc = 0.01, zc < 0 and zc == 0, and the front flag bit for bit at zc around 2^-52; the
    same set translated by 1e4."""
    stats = []
    fails = G.filter_failures(capi.filter_tracks, shift, stats=stats)
    _report(stats)
    assert fails == []


def test_filter_outputs_are_optional_and_equal():
    """Each output alone equals the output of the full call (any pointer may be NULL)."""
    import ctypes as C

    tr, xyz = G.filter_cases(0.0)
    ang, err, front = capi.filter_tracks(tr, xyz)
    ct = tr.c_tracks()
    a1, e1, f1 = np.zeros(tr.n_tracks), np.zeros(tr.n_el), np.zeros(tr.n_el, np.uint8)
    L = capi.lib()
    assert L.mpsfm_filter_tracks(C.byref(ct), xyz.ctypes.data, 0, a1.ctypes.data, None, None) == 0
    assert L.mpsfm_filter_tracks(C.byref(ct), xyz.ctypes.data, 0, None, e1.ctypes.data, f1.ctypes.data) == 0
    np.testing.assert_array_equal(a1, ang)
    np.testing.assert_array_equal(e1, err)
    np.testing.assert_array_equal(f1.astype(bool), front)


def test_an_element_behind_its_camera_is_bad_whatever_its_error():
    """el_sq_err is the plain formula for zc < eps: small for a mirrored point, inf or NaN for zc == 0.  That is safe
    only because reprojection_decisions ORs in ~front: every element with front == 0 is decided bad."""
    tr, xyz = G.filter_cases(0.0)
    _, err, front = capi.filter_tracks(tr, xyz)
    _, bad = reprojection_decisions(tr.track_start, err, front, 4.0)
    assert (~front).sum() >= 8 and bad[~front].all()
    behind = err[~front]
    assert (~np.isfinite(behind)).any() and (behind < 1e-12).any()
    k = tr.labels.index("err_zc_zero_off_axis")
    assert np.isinf(err[tr.track_start[k]])  # (fx * 0.5 / 0)^2 + (fy * -0.25 / 0)^2
    k = tr.labels.index("front_z=0.0")
    assert np.isnan(err[tr.track_start[k]])  # fx * 0 / 0


@pytest.mark.parametrize("magnitude", [0.25, 4.0, 1e-6])
def test_point_covs_friendly_magnitudes(magnitude):
    stats, out = [], []
    fails = G.cov_failures(_keep(capi.point_covs, out), G.friendly_cov_problem, magnitude, stats=stats)
    _report(stats)
    assert fails == []
    assert np.isfinite(out[0]).all()


@pytest.mark.parametrize("n_obs", [255, 256, 257])
def test_point_covs_accumulation_block_edges(n_obs):
    """n_obs around the 256 threads of an accumulation block."""
    assert G.cov_failures(capi.point_covs, G.friendly_cov_problem, 1.0, n_obs) == []


def test_point_covs_hard_cases_twice():
    """5000 observations piling their atomics onto six doubles beside two-observation landmarks, two-view landmarks
    down to a baseline over depth of 1e-4, a landmark 0.01 in front of a camera, and landmarks with 0 and 1 observation
    between ordinary ones: NaN by the count, the neighbours within the criterion.  The call is made twice; both results
    meet the criterion (bitwise equality is not asserted: the order of the atomics is free)."""
    _, labels = G.hard_cov_problem()
    out = []
    for _ in range(2):
        stats = []
        fails = G.cov_failures(_keep(capi.point_covs, out), G.hard_cov_problem, stats=stats)
        _report(stats)
        assert fails == []
    covs = out[1]
    for lab, c in zip(labels, covs):
        assert np.isnan(c).all() == (lab in ("no_obs", "one_obs")), lab
    for lab in ("parallax0.01", "two_obs_a", "obs5000", "zc_0.01"):  # well conditioned: finite
        assert np.isfinite(covs[labels.index(lab)]).all(), lab


# ---- mpsfm_tri_estimate_batch and mpsfm_init_pair_candidates against the exact walk ----------------------------------------
def _batch(box=None):
    def call(cs, P, K, xy, min_angle, max_error, rt, min_num_trials):
        out = capi.tri_estimate_batch(cs, P, K, xy, min_angle, max_error, rt, min_num_trials)
        if box is not None:
            box.append(out)
        return out

    return call


@pytest.mark.parametrize("residual_type", [G.ANGULAR, G.REPROJECTION])
def test_candidate_cases_twice(residual_type):
    """One launch over every candidate that leaves min_num_trials to the library and one over those that set it: ok and
    the mask exact where decided, the point by the backward (and forward) criterion on the matrix of the exact index set,
    zeros for every failed candidate; open candidates (the threshold group) give one of the two legal outcomes.
    Run twice: one thread per candidate and no atomics, so the two runs are equal bit for bit."""
    stats, out = [], []
    fails, open_ = G.candidate_failures(_batch(out), residual_type, stats=stats)
    _report(stats)
    print("open:", open_)
    assert fails == []
    g = G.candidate_golden()
    assert set(open_) <= {str(l) for l, grp in zip(g["labels"], g["groups"]) if grp == "threshold"}
    again = []
    G.candidate_failures(_batch(again), residual_type)
    assert len(out) == len(again) == 2
    for a, b in zip(out, again):
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("n_candidates", G.CAND_BLOCK_EDGES)
def test_candidate_block_edges(n_candidates):
    """The friendly candidates (2, 3, 5, 15, 16, 63, 64 views) repeated up to candidate counts around the 64 threads of a
    block, for both residual types."""
    g = G.candidate_golden()
    friendly = [c for c, grp in enumerate(g["groups"]) if grp == "friendly"]
    which = [friendly[k % len(friendly)] for k in range(n_candidates)]
    for rt in (G.ANGULAR, G.REPROJECTION):
        fails, open_ = G.candidate_failures(_batch(), rt, which)
        assert fails == [] and open_ == []


def test_candidate_contract():
    """Candidates of 0 and 1 views between ordinary ones give ok = 0 and zeros, their neighbours are untouched; a
    caller's min_num_trials of 0, 1 and C(n, 2) is honoured (the three settings end at different points where the exact
    walk says so); the explicit array with the library's own rule in it equals NULL."""
    g = G.candidate_golden()
    labels = g["labels"].tolist()
    contract = [c for c, grp in enumerate(g["groups"]) if grp == "contract"]
    short = [contract.index(labels.index(lab)) for lab in ("empty", "one_view")]
    for rt in (G.ANGULAR, G.REPROJECTION):
        out = []
        fails, open_ = G.candidate_failures(_batch(out), rt, contract, explicit_trials=True)
        assert fails == [] and open_ == []
        xyz, ok, inl = out[0]
        start = G.candidate_launch(contract)[0]
        for k in short:
            assert not ok[k] and not xyz[k].any() and not inl[start[k]:start[k + 1]].any()
        assert ok[[k for k in range(len(contract)) if k not in short]].all()
        named = [c for c, grp in enumerate(g["groups"]) if grp in ("friendly", "outliers", "geometry")]
        a, b = [], []
        G.candidate_failures(_batch(a), rt, named)
        G.candidate_failures(_batch(b), rt, named, explicit_trials=True)
        for x, y in zip(a[0], b[0]):
            assert x.tobytes() == y.tobytes()
    m0, m120 = labels.index("trials_noisy16_mnt0"), labels.index("trials_noisy16_mnt120")
    assert g["idx0"][m0] != g["idx0"][m120] or g["idx1"][m0] != g["idx1"][m120]  # the settings do differ in the exact walk


@pytest.mark.parametrize("what", [G.INIT_TRIANGULATE, G.INIT_LIFT, G.INIT_TRIANGULATE | G.INIT_LIFT])
def test_init_pair_cases(what):
    """Friendly matches, low parallax down to an acos argument within eps of 1 (NaN legal there and nowhere else), a lifted
    point behind camera 2, diverging rays; rescale 1 and 0.437, select with zeros, tri_min_angle 0 and 1.5 degrees."""
    for rescale, min_angle, sel in ((1.0, 0.0, False), (0.437, np.deg2rad(1.5), True)):
        stats = []
        fails, open_ = G.init_pair_failures(capi.init_pair_candidates, what, rescale, min_angle, use_select=sel, stats=stats)
        _report(stats)
        print("open matches:", open_)
        assert fails == []
        assert not set(G.init_pair_cases()["groups"]["friendly"]) & set(open_)


@pytest.mark.parametrize("n_matches", G.INIT_BLOCK_EDGES)
def test_init_pair_block_edges(n_matches):
    """n_matches around the 256 threads of a k_init_candidates block."""
    fails, open_ = G.init_pair_failures(capi.init_pair_candidates, G.INIT_TRIANGULATE | G.INIT_LIFT, 0.437, 0.0, n_matches=n_matches, use_select=True)
    assert fails == [] and open_ == []
