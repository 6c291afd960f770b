"""mpsfm_triangulate_tracks, mpsfm_filter_tracks and mpsfm_point_covs against the exact reference of
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
