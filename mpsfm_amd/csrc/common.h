// Shared device/host definitions for libmpsfm_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <float.h>
#include <math.h>

#include "../../include/mpsfm_hip.h"
#include "chol_plan.h"

namespace mpsfm {

// tuning knobs (overridable with -D for experiments; scripts/sweep_variants.sh)
#ifndef MPSFM_TILE_CAMS
#define MPSFM_TILE_CAMS 16
#endif
#ifndef MPSFM_ITEM_PAIRS
#define MPSFM_ITEM_PAIRS 64
#endif
#ifndef MPSFM_CAM_COPIES
#define MPSFM_CAM_COPIES 3  // LDS copies of the per-camera accumulators of the track sweep
#endif
#ifndef MPSFM_ENT_STAGE
#define MPSFM_ENT_STAGE 1024
#endif
#ifndef MPSFM_OBS_MAX
#define MPSFM_OBS_MAX 252  // 252 records x 144 B of Z + the accumulators = 53.4 KB of LDS: three workgroups of the dense sweep per CU
#endif

// ---- track-sweep chunk geometry ----------------------------------------------------------
// A chunk = a group of consecutive (re-ordered) landmarks processed by one workgroup.
typedef double v4d __attribute__((ext_vector_type(4)));  // accumulators of v_mfma_f64_16x16x4_f64
constexpr int kThreads = 256;   // workgroup size of the sweep kernels
constexpr int kObsMax = MPSFM_OBS_MAX;    // merged (camera, landmark) records per chunk
constexpr int kPtsMax = MPSFM_OBS_MAX / 2;     // landmarks per chunk
constexpr int kTileCams = MPSFM_TILE_CAMS;   // local cameras whose U blocks / g_c are accumulated in LDS
#ifndef MPSFM_LOCAL_CAMS
#define MPSFM_LOCAL_CAMS 254
#endif
constexpr int kLocalCamsMax = MPSFM_LOCAL_CAMS;  // local camera list length (beyond kTileCams: direct atomics); < 255 (8-bit local index)
static_assert(kLocalCamsMax < 255, "local camera indices are 8 bits, 0xff marks a constant camera");
constexpr int kPairGroup = 6;   // lanes cooperating on one 6x6 block of the reduced system (one row each)
constexpr int kItemPairs = MPSFM_ITEM_PAIRS;  // pairs per Schur work item (heavier blocks are split for balance)
constexpr int kEntStage = MPSFM_ENT_STAGE; // pair entries of a chunk staged in LDS (larger chunks read them from HBM)
static_assert(kObsMax <= 256 && kPtsMax <= 128, "chunk-relative record / landmark indices are packed into 8 bits (rec_meta, pair entries)");
constexpr int kMaxDevices = 16;  // per-device pools (allocator cache, streams, staging buffers) are arrays of this length
constexpr int kWStride = 18;    // row stride (doubles) of the per-record W block in LDS: 144 B, keeps rows 16-B aligned for ds_read_b128
constexpr int kCamRec = 24;     // doubles per camera table record

// camera table record: R[9] t[3] K[4] cs[6] pad[2]
// cs = Jacobi column scale * tangent mask (0 for constant cameras / fixed coordinates)

struct ChunkHdr {
  int32_t rec0, nrec;    // merged records [rec0, rec0+nrec)
  int32_t pt0, npt;      // re-ordered landmarks [pt0, pt0+npt)
  int32_t cam0, ncam;    // local camera list in chunk_cams[cam0 ..)
  int32_t blk0, nblk;    // Schur work items (a destination block of S + a run of its pairs) of this chunk
  int32_t ent0, nent;    // the chunk's pair entries
  int32_t dense;         // 1: at most kDenseCams local cameras, kDensePts landmarks and one record per (camera, variable landmark): swept by
                         //    k_track_sweep_dense (Schur products as one small dense product on the matrix pipe, results through the chunk's
                         //    slab); such chunks have no pair tables
  int32_t slab0;         // dense chunks: start of the chunk's slab in SweepArgs::slab, in units of 18 doubles
};
constexpr int kDenseCams = 16;  // 16 cameras x 6 rows = 96 rows = six 16-row MFMA tiles
constexpr int kDensePts = 96;   // landmarks of a dense chunk
// ... by the size of its camera set when `by_cams` (small problems: one workgroup per chunk and CU, the slowest chunk sets the pace and
// a chunk's Schur products grow with landmarks x tile pairs): 96 up to 6 cameras, 64 up to 8, 48 up to 12, 32 beyond
__host__ __device__ inline int dense_pts_cap(int ncams, int by_cams) { return (!by_cams || ncams <= 6) ? kDensePts : (ncams <= 8 ? 64 : (ncams <= 12 ? 48 : 32)); }
// slab of a dense chunk: [ncam (ncam + 1) / 2 blocks (ci <= cj at cj (cj + 1) / 2 + ci) x 36][ncam x (g_c 6 | W V^-1 g_p 6 | diag U 6)] doubles,
// written with plain stores by k_track_sweep_dense and summed per destination by k_reduce_slabs
__host__ __device__ inline int64_t slab_doubles(int ncam) { return (int64_t)(ncam * (ncam + 1) / 2) * 36 + (int64_t)ncam * 18; }

// Estimated life of a dense chunk's workgroup from its header alone, in shader cycles: the order table of k_track_sweep_dense starts
// the chunks by descending cost (SweepArgs::order), so that the dispatcher's last round of workgroups holds the light ones.
// A constant (barriers and the chains of memory trips every chunk pays), the records (P1, P3a: one thread per record, so they
// hardly count) and the Schur products (P3b: tile pairs x groups of four landmarks).  The constants are a least-squares fit of the
// per-chunk phase stamps (debug flag 128, scripts/dbg_sweep_trace.py) of the 3 032 chunks of C3 on the MI355X, the mean of the fits
// in table order (32 565, -8.9, 158.1) and in this order (25 787, 16.5, 177.0); residual 5.5-7.5 k of a mean life of 40.6 k cycles
// (DESIGN.md "Measured on MI355X, round 13").  Only the order of the costs matters.  Integers: the host and the device build must
// sort alike.
constexpr int32_t kSweepCostBase = 29000, kSweepCostRec = 4, kSweepCostPair = 168;
__host__ __device__ inline int32_t dense_sweep_cost(int nrec, int npt, int ncam) {
  const int nt = (6 * ncam + 15) / 16;
  return kSweepCostBase + kSweepCostRec * nrec + kSweepCostPair * (nt * (nt + 1) / 2) * ((npt + 3) / 4);
}
// ... and the table's sort key: descending cost, ties by ascending chunk (an ascending sort of unique 64-bit keys)
__host__ __device__ inline uint64_t dense_sweep_order_key(const ChunkHdr& H, int cix) {
  return ((uint64_t)(0x7fffffffu - (uint32_t)dense_sweep_cost(H.nrec, H.npt, H.ncam)) << 32) | (uint32_t)cix;
}

// One destination of the slab reduction: a 6x6 block of S (kind 0: all 36 entries, 1: a diagonal block, upper triangle) or a camera's
// vectors (kind 2).  Destinations with many sources are split into parts (every part adds atomically into the zeroed buffer).
struct RedDest { int32_t kind; int32_t dst; int32_t s0, s1; };
// Where a destination lands in the tile-major system of the dense solve (the direct form of the slab reduction): the first system
// column of its two slots, lower slot first (a camera's vectors: its one slot's, then 0) — from the plan's col_of_slot, per handle.
struct RedCols { int32_t c0, c1; };
// ... and the table the direct form reads instead of RedDest: the destination with its columns, one 32-byte load
struct alignas(32) RedDestCols { RedDest d; RedCols c; int32_t pad_[2]; };

// A landmark whose track does not fit a chunk (more than kObsMax records or kLocalCamsMax cameras)
// is swept by a workgroup of its own that strides over the records (k_long_track_sweep).
struct LongHdr {
  int32_t rec0, nrec;    // its records (variable cameras first, sorted by slot)
  int32_t pt;            // re-ordered landmark index
  int32_t kv;            // records with a variable camera
  int64_t w0;            // first row of its W scratch (18 doubles per record)
};

// record meta word: lcam | lpt << 8 | flags << 16
constexpr uint32_t kRecHasReproj = 1u << 16;
constexpr uint32_t kRecHasDepth = 1u << 17;
constexpr uint32_t kLcamConst = 255;

struct LossParams {
  int32_t reproj_type;
  double reproj_a;
  double reproj_mag;
  int32_t depth_type;
};

// scalar slots of the reduced buffer tail (all-reduced with S)
constexpr int kMaxRankSlots = 64;  // ranks whose landmark-gradient maxima travel exactly (one slot each in the summed tail)
enum { SC_COST = 0, SC_BAD = 1, SC_GMAX_PTS = 2, SC_RANK0 = 8, SC_COUNT = 8 + kMaxRankSlots };

// scalar slots produced by the update sweep + camera update (host reads these each iteration)
enum {
  U_CAND_COST = 0, U_BAD = 1, U_MCC = 2, U_STEP_SQ_PTS = 3, U_XN_SQ_PTS = 4,
  U_STEP_SQ_CAMS = 5, U_XN_SQ_CAMS = 6, U_GMAX_CAMS = 7, U_X_COST = 8, U_X_BAD = 9,
  U_GMAX_PTS = 10, U_CHOL_FAIL = 11, U_COUNT = 16
};

// Levenberg-Marquardt control block on the device.  The accept / reject decision of an iteration (Ceres
// trust_region_minimizer.cc) is taken by a one-thread kernel (k_lm_decide) from the scalars the sweeps leave behind, so the
// host enqueues iteration i+1 while iteration i still runs and only reads a copy of this block one iteration late: no
// stream synchronisation inside the loop.  Every kernel of an iteration returns at once when `term` says the solve is
// over (the one iteration enqueued ahead of the news).
struct LmHead {  // what travels to the host every iteration
  double radius, decrease_factor, x_norm, cur_cost, fixed_cost, initial_cost;
  double last_x_cost, last_cand, last_rel, last_step_norm, last_mcc;  // diagnostics of the last decided iteration
  int32_t term;          // kLmRunning, MPSFM_TERM_* once decided, kLmNumericError: the initial point cannot be evaluated
  int32_t iter, invalid_run, check_gradient, accepted, n_success, n_unsuccess, n_cost_evals, n_jac_evals, last_chol_fail, trace_len, pad_;
};
struct LmCtl : LmHead {
  double trace_cost[MPSFM_MAX_TRACE], trace_radius[MPSFM_MAX_TRACE];
  uint8_t trace_accepted[MPSFM_MAX_TRACE];
};
constexpr int32_t kLmRunning = -1, kLmNumericError = -2;
struct LmOpts {
  double function_tolerance, gradient_tolerance, parameter_tolerance, min_relative_decrease, max_radius, min_radius;
  int32_t max_iterations, max_invalid_steps;
};
__device__ inline bool lm_over(const LmCtl* c) { return c != nullptr && __hip_atomic_load(&c->term, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != kLmRunning; }
__device__ inline double lm_radius_of(const LmCtl* c) { return __hip_atomic_load(&c->radius, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// The agent-scope atomic of lm_over() is what a reader needs whose writer runs in the SAME launch (local_lm.hip).  In the launch chain
// the writer of `term` and `radius` (k_lm_decide) is an earlier launch of the same stream: the launch boundary publishes its stores
// and nothing writes the block while a later kernel runs, so a plain load is sufficient there, and the kernels of the dense solve
// use one (lm_term_chain / lm_radius_chain).  The block was written by another compute die a moment ago, so the load goes all the
// way to memory; as a vector load it is counted with the kernel's first operand loads: requested in front of them, tested behind
// them and before the first store, its trip runs under theirs instead of in front of them.  (A scalar load would do as well, but
// scalar loads return out of order: the wait for the item's launch record, which hits in L2, would wait for this one too.)
#define MPSFM_CONST_AS __attribute__((address_space(4)))
template <typename T>
__device__ __forceinline__ T load_const(const T* p) { return *reinterpret_cast<const MPSFM_CONST_AS T*>(reinterpret_cast<uintptr_t>(p)); }
__device__ __forceinline__ int32_t lm_term_chain(const LmCtl* c) {
  return c != nullptr ? __hip_atomic_load(&c->term, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : kLmRunning;
}
// the test of a value of lm_term_chain, at the place where it stands: the empty asm keeps the compiler from moving the test, and
// with it the wait for the load, to the front of the requests it was written behind
__device__ __forceinline__ bool lm_over_chain(int32_t term) { asm volatile("" : "+v"(term)); return __builtin_amdgcn_readfirstlane(term) != kLmRunning; }
// the same request without a branch in front of it, so that the kernel's arguments can all be fetched in one batch: without a
// control block it reads `readable` (any readable word) and the caller does not look at the value (c != nullptr && lm_over_chain(v))
__device__ __forceinline__ int32_t lm_term_chain(const LmCtl* c, const void* readable) {
  return __hip_atomic_load(c != nullptr ? &c->term : static_cast<const int32_t*>(readable), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ double lm_radius_chain(const LmCtl* c, double fallback) {
  return c != nullptr ? __hip_atomic_load(&c->radius, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : fallback;
}

// `accepted` and `radius` the same way for the sweeps of the launch chain, which request the control block in one batch with their
// chunk header: no branch in front of the requests; without a control block the value read from `readable` (8 readable bytes,
// 8-aligned) is replaced by `fallback` where it is used.
__device__ __forceinline__ int32_t lm_accepted_chain(const LmCtl* c, const void* readable) {
  return __hip_atomic_load(c != nullptr ? &c->accepted : static_cast<const int32_t*>(readable), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ double lm_radius_chain(const LmCtl* c, const void* readable, double fallback) {
  const double r = __hip_atomic_load(c != nullptr ? &c->radius : static_cast<const double*>(readable), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  return c != nullptr ? r : fallback;
}

// ---- small device math -------------------------------------------------------------------
// Comparison builds (MPSFM_EXTRA_FLAGS): -DMPSFM_LIBM_MATH puts libm's log(), sqrt(), sin(), cos() and the IEEE quotients back where
// lean_log, quat_plus' polynomials and sweep_rcp stand; -DMPSFM_LIBM_LOG, -DMPSFM_LIBM_QUAT and -DMPSFM_LIBM_DIV do so one by one.
#ifdef MPSFM_LIBM_MATH
#define MPSFM_LIBM_LOG 1
#define MPSFM_LIBM_QUAT 1
#define MPSFM_LIBM_DIV 1
#endif
// Reciprocal, square root and reciprocal square root in a handful of instructions: the hardware estimate (v_rcp_f64 / v_rsq_f64,
// ~2^-22 relative) refined by two Newton steps (error ~ e^4: below one ulp; the last bit may differ from the IEEE-rounded quotient
// the compiler's ~30-instruction expansion of `/` and sqrt() delivers).  The sweeps take five quotients and three roots per record.
__host__ __device__ inline double fast_rcp(double x) {
#ifdef __HIP_DEVICE_COMPILE__
  double y = __builtin_amdgcn_rcp(x);
  y = fma(y, fma(-x, y, 1.0), y);
  return fma(y, fma(-x, y, 1.0), y);
#else
  return 1.0 / x;
#endif
}
// s = sqrt(x), r = 1 / sqrt(x) for x > 0 (x == 0: s = 0, r = inf)
__host__ __device__ inline void fast_sqrt_rsqrt(double x, double& s, double& r) {
#ifdef __HIP_DEVICE_COMPILE__
  const double y = __builtin_amdgcn_rsq(x);
  double g = x * y, h = 0.5 * y;
  double e = fma(-g, h, 0.5);
  g = fma(g, e, g); h = fma(h, e, h);
  e = fma(-g, h, 0.5);
  g = fma(g, e, g); h = fma(h, e, h);
  s = x == 0.0 ? 0.0 : g;
  r = x == 0.0 ? y : 2.0 * h;
#else
  s = sqrt(x); r = 1.0 / s;
#endif
}
__host__ __device__ inline double fast_sqrt(double x) { double s, r; fast_sqrt_rsqrt(x, s, r); return s; }

// A polynomial coefficient that lives where it is used and no longer.  As plain constants the compiler lifts all of them out of the
// enclosing loop — the camera loop of cam_update_all, beside the constants of libm's sine and cosine, and the iteration loop of
// k_local_lm — runs out of scalar registers, moves them to vector registers and spills: two scalar moves per use instead.
__host__ __device__ inline double local_const(double c) {
#ifdef __HIP_DEVICE_COMPILE__
  asm volatile("" : "+s"(c));
#endif
  return c;
}

// Natural logarithm of a finite x > 0 (subnormals included; +inf gives +inf), within one ulp: fdlibm's e_log.c without its special
// cases.  x = 2^k m with m in [sqrt(1/2), sqrt(2)), f = m - 1, s = f / (2 + f), log(m) = f - f^2/2 + s (f^2/2 + R(s^2)).  The
// mantissa and the exponent come from the hardware's frexp (which normalises subnormals), the quotient from the reciprocal estimate,
// two Newton steps and one residual correction: about 45 vector instructions where ocml's log() takes about 95.  Arguments <= 0 and
// NaN are the callers' business (they test Zc > 0, and Cauchy's argument is >= 1).
__host__ __device__ inline double lean_log(double x) {
#ifdef MPSFM_LIBM_LOG
  return log(x);
#else
  constexpr double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
  constexpr double Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01,
                   Lg4 = 2.222219843214978396e-01, Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
                   Lg7 = 1.479819860511658591e-01;
#ifdef __HIP_DEVICE_COMPILE__
  double m = __builtin_amdgcn_frexp_mant(x);  // [1/2, 1)
  const int e = __builtin_amdgcn_frexp_exp(x);
#else
  if (x == HUGE_VAL) return x;
  int e;
  double m = frexp(x, &e);
#endif
  const bool low = m < 0.70710678118654752440;
  m = low ? 2.0 * m : m;
  const double k = (double)(low ? e - 1 : e);
  const double f = m - 1.0, den = 2.0 + f;
#ifdef __HIP_DEVICE_COMPILE__
  const double y = fast_rcp(den);
  double s = f * y;
  s = fma(fma(-s, den, f), y, s);
#else
  const double s = f / den;
#endif
  const double z = s * s, w = z * z;
  const double t1 = w * fma(w, fma(w, local_const(Lg6), local_const(Lg4)), local_const(Lg2));
  const double t2 = z * fma(w, fma(w, fma(w, local_const(Lg7), local_const(Lg5)), local_const(Lg3)), local_const(Lg1));
  const double R = t2 + t1, hfsq = 0.5 * f * f;
  const double r = k * ln2_hi - ((hfsq - (s * (hfsq + R) + k * ln2_lo)) - f);
#ifdef __HIP_DEVICE_COMPILE__
  return x == HUGE_VAL ? x : r;
#else
  return r;
#endif
#endif
}

// The quotients of the sweeps — clamp(V) / lm_radius for the damping of a landmark block, g / p and g_c / s for the gradient maxima —
// as products with a fast_rcp reciprocal (k_assemble and damp_columns keep the IEEE quotient for the camera side)
__host__ __device__ inline double sweep_rcp(double x) {
#ifdef MPSFM_LIBM_DIV
  return 1.0 / x;
#else
  return fast_rcp(x);
#endif
}
__host__ __device__ inline double sweep_div(double a, double b) {
#ifdef MPSFM_LIBM_DIV
  return a / b;
#else
  return a * fast_rcp(b);
#endif
}
// V packed upper [00 01 02 11 12 22] += clamp(diag V) * inv_radius, inv_radius = sweep_rcp(lm_radius)
__host__ __device__ inline void damp_landmark(double* V, double min_diag, double max_diag, double lm_radius, double inv_radius) {
#ifdef MPSFM_LIBM_DIV
  V[0] += fmin(fmax(V[0], min_diag), max_diag) / lm_radius;
  V[3] += fmin(fmax(V[3], min_diag), max_diag) / lm_radius;
  V[5] += fmin(fmax(V[5], min_diag), max_diag) / lm_radius;
#else
  V[0] = fma(fmin(fmax(V[0], min_diag), max_diag), inv_radius, V[0]);
  V[3] = fma(fmin(fmax(V[3], min_diag), max_diag), inv_radius, V[3]);
  V[5] = fma(fmin(fmax(V[5], min_diag), max_diag), inv_radius, V[5]);
#endif
}

__host__ __device__ inline void loss_eval(int type, double a, double s, double& rho0, double& rho1) {
  if (type == MPSFM_LOSS_SOFT_L1) {
    const double b = a * a, c = fast_rcp(b);
    const double sum = 1.0 + s * c;
    double tmp, itmp;
    fast_sqrt_rsqrt(sum, tmp, itmp);
    rho0 = 2.0 * b * (tmp - 1.0);
    rho1 = fmax(DBL_MIN, itmp);
  } else if (type == MPSFM_LOSS_CAUCHY) {
    const double b = a * a, c = fast_rcp(b);
    const double sum = 1.0 + s * c;
    rho0 = b * lean_log(sum);
    rho1 = fmax(DBL_MIN, fast_rcp(sum));
  } else {
    rho0 = s;
    rho1 = 1.0;
  }
}

__host__ __device__ inline void quat_to_R(const double* q, double* R) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
  R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
}

// sin(n) / n and cos(n) are even in n: for z = n^2 <= (pi/4)^2 they are fdlibm's __kernel_sin and __kernel_cos as polynomials in z —
// no square root, no division, and z == 0 gives (1, 1) exactly, so that the plus below returns q itself.
constexpr double kQuatPolyMaxZ = 0.61685027506808491368;  // (pi/4)^2
__host__ __device__ inline double quat_sinc_poly(double z) {
  constexpr double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                   S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
  double p = z * local_const(S6) + local_const(S5);
  p = fma(z, p, local_const(S4)); p = fma(z, p, local_const(S3)); p = fma(z, p, local_const(S2)); p = fma(z, p, local_const(S1));
  return fma(z, p, 1.0);
}
__host__ __device__ inline double quat_cos_poly(double z) {
  constexpr double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                   C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
  double p = z * local_const(C6) + local_const(C5);
  p = fma(z, p, local_const(C4)); p = fma(z, p, local_const(C3)); p = fma(z, p, local_const(C2)); p = fma(z, p, local_const(C1));
  const double r = z * p;
  return 1.0 - (0.5 * z - z * r);
}
// ... and beyond the polynomials' range: libm's sine and cosine of n, with n and 1 / n from one reciprocal square root
__host__ __device__ inline void quat_sinc_cos_far(double z, double& sbd, double& pw) {
  double n, in, sn;
  fast_sqrt_rsqrt(z, n, in);
#ifdef __HIP_DEVICE_COMPILE__
  sincos(n, &sn, &pw);
#else
  sn = sin(n); pw = cos(n);
#endif
  sbd = sn * in;
}
// sbd = sin(n) / n, pw = cos(n) for z = n^2 >= 0 (the second branch is lane-divergent; no ordinary step takes it)
__host__ __device__ inline void quat_sinc_cos(double z, double& sbd, double& pw) {
  if (z <= kQuatPolyMaxZ) { sbd = quat_sinc_poly(z); pw = quat_cos_poly(z); }
  else quat_sinc_cos_far(z, sbd, pw);
}

// q' = exp(d) * q from sbd = sin|d| / |d| and pw = cos|d|
__host__ __device__ inline void quat_apply(const double* q, const double* d, double sbd, double pw, double* out) {
  const double px = sbd * d[0], py = sbd * d[1], pz = sbd * d[2];
  const double qx = q[0], qy = q[1], qz = q[2], qw = q[3];
  out[0] = pw * qx + px * qw + py * qz - pz * qy;
  out[1] = pw * qy - px * qz + py * qw + pz * qx;
  out[2] = pw * qz + px * qy - py * qx + pz * qw;
  out[3] = pw * qw - px * qx - py * qy - pz * qz;
}
// EigenQuaternionManifold::Plus, q' = exp(d) * q (the branch of quat_sinc_cos, with the product on either side of it)
__host__ __device__ inline void quat_plus(const double* q, const double* d, double* out) {
#ifdef MPSFM_LIBM_QUAT
  const double n = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  if (n == 0.0) { out[0] = q[0]; out[1] = q[1]; out[2] = q[2]; out[3] = q[3]; return; }
  const double sbd = sin(n) / n, pw = cos(n);
#else
  const double z = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
  if (z <= kQuatPolyMaxZ) { quat_apply(q, d, quat_sinc_poly(z), quat_cos_poly(z), out); return; }
  double sbd, pw;
  quat_sinc_cos_far(z, sbd, pw);
#endif
  quat_apply(q, d, sbd, pw, out);
}

// 3x3 SPD inverse via LL^T; V packed upper [00 01 02 11 12 22]
__host__ __device__ inline bool spd3_inverse(const double* V, double* Vi) {
  const double a = V[0], b = V[1], c = V[2], d = V[3], e = V[4], f = V[5];
  if (!(a > 0.0)) return false;
  const double l00 = sqrt(a);
  const double l10 = b / l00, l20 = c / l00;
  const double t11 = d - l10 * l10;
  if (!(t11 > 0.0)) return false;
  const double l11 = sqrt(t11);
  const double l21 = (e - l20 * l10) / l11;
  const double t22 = f - l20 * l20 - l21 * l21;
  if (!(t22 > 0.0)) return false;
  const double l22 = sqrt(t22);
  const double i00 = 1.0 / l00, i11 = 1.0 / l11, i22 = 1.0 / l22;
  const double i10 = -l10 * i00 * i11;
  const double i21 = -l21 * i11 * i22;
  const double i20 = -(l20 * i00 + l21 * i10) * i22;
  Vi[0] = i00 * i00 + i10 * i10 + i20 * i20;
  Vi[1] = i10 * i11 + i20 * i21;
  Vi[2] = i20 * i22;
  Vi[3] = i11 * i11 + i21 * i21;
  Vi[4] = i21 * i22;
  Vi[5] = i22 * i22;
  return true;
}

// The inverse Cholesky factor of a 3x3 SPD matrix: V = L L^T, F = L^-1 (lower), packed [00 10 11 20 21 22],
// so that V^-1 = F^T F.  With Z = W F^T:  W V^-1 W'^T = Z Z'^T  and  W V^-1 g = Z (F g).
__host__ __device__ inline bool spd3_inv_factor(const double* V, double* F) {
  const double a = V[0], b = V[1], c = V[2], d = V[3], e = V[4], f = V[5];
  if (!(a > 0.0)) return false;
  double l00, i00, l11, i11, l22, i22;  // the factor's diagonal and its inverse from one reciprocal square root each
  fast_sqrt_rsqrt(a, l00, i00);
  const double l10 = b * i00, l20 = c * i00;
  const double t11 = d - l10 * l10;
  if (!(t11 > 0.0)) return false;
  fast_sqrt_rsqrt(t11, l11, i11);
  const double l21 = (e - l20 * l10) * i11;
  const double t22 = f - l20 * l20 - l21 * l21;
  if (!(t22 > 0.0)) return false;
  fast_sqrt_rsqrt(t22, l22, i22);
  const double i10 = -l10 * i00 * i11;
  const double i21 = -l21 * i11 * i22;
  const double i20 = -(l20 * i00 + l21 * i10) * i22;
  F[0] = i00; F[1] = i10; F[2] = i11; F[3] = i20; F[4] = i21; F[5] = i22;
  return true;
}

__host__ __device__ inline void sym3_mul(const double* S, double v0, double v1, double v2, double* o) {
  o[0] = S[0] * v0 + S[1] * v1 + S[2] * v2;
  o[1] = S[1] * v0 + S[3] * v1 + S[4] * v2;
  o[2] = S[2] * v0 + S[4] * v1 + S[5] * v2;
}

// packed index of the upper block triangle (i <= j) of an ncv x ncv block matrix
__host__ __device__ inline int64_t ut_block(int64_t i, int64_t j, int64_t ncv) {
  return i * ncv - (i * (i - 1)) / 2 + (j - i);
}
// Block-skyline storage of the upper block triangle of S: column j keeps the blocks (i, j), first[j] <= i <= j, at
// start[j] + (i - first[j]) — first[j] is the lowest camera slot that shares a landmark with slot j on ANY rank
// (build_tables in ba_build.hip), so every block a sweep can touch exists, and the buffer the ranks all-reduce holds the blocks
// that can be nonzero instead of all ncv (ncv + 1) / 2 (C4: 11 MB instead of 144 MB).
//
// Two forms.  index != NULL (up to kIndexMaxSlots slots): index[j * ns + i], i <= j, is the block's position or -1 — exactly
// the blocks of camera pairs that share a landmark on some rank, whatever the slot order (the nested-dissection order of
// chol_plan.h puts separator cameras last, whose skyline columns would be nearly full).  Otherwise the skyline proper:
// column j keeps the blocks first[j] <= i <= j.
struct BlockSky {
  const int32_t* first;
  const int64_t* start;
  const int32_t* index;
  int32_t ns;
};
constexpr int kIndexMaxSlots = 4096;
__host__ __device__ inline bool sky_has(const BlockSky& k, int64_t i, int64_t j) {
  return k.index ? k.index[j * k.ns + i] >= 0 : i >= k.first[j];
}
__host__ __device__ inline int64_t sky_block(const BlockSky& k, int64_t i, int64_t j) {
  return k.index ? (int64_t)k.index[j * k.ns + i] : k.start[j] + (i - k.first[j]);
}
// position of system column g in the slot-indexed vectors, -1 for a padding column or beyond the system
__host__ __device__ inline int vec_index(const int32_t* col_slot, int g, int n) {
  if (g >= n) return -1;
  if (!col_slot) return g;
  const int cs = col_slot[g];
  return cs < 0 ? -1 : (cs >> 3) * 6 + (cs & 7);
}
// packed index of lower-triangle tile (ti >= tj)
__host__ __device__ inline int64_t lt_tile(int64_t ti, int64_t tj) { return ti * (ti + 1) / 2 + tj; }

// ---- kernel argument blocks ---------------------------------------------------------------
struct SweepArgs {
  const ChunkHdr* chunks;
  const int32_t* chunk_cams;     // reduced-system slot of every local camera
  const int32_t* rec_cam;        // camera index (camera table row)
  const uint32_t* rec_meta;      // lcam | lpt<<8 | flags<<16
  const double* rec_xy;          // [nrec][2]
  const double* rec_d;           // log of the effective prior depth d*exp(s)+b
  const double* rec_m;           // depth loss magnitude
  const double* rec_a;           // depth loss scale
  const int32_t* pt_rec_start;   // [np+1]
  const uint16_t* pt_kv;         // [np] records with a variable camera (0: constant landmark)
  const uint32_t* blk_desc;      // per destination block: li | lj << 8
  const int32_t* blk_ent_start;  // [nblocks+1] entry range of each block
  const uint32_t* ents;          // per Schur pair: ri | rj << 8 | lpt << 16 (chunk-relative records)
  const double* camtab;          // [nc][24] at the linearisation point
  const double* pts;             // [np][3]
  const double* ps;              // [np][3] Jacobi scale (0: constant landmark)
  LossParams loss;
  double radius, min_diag, max_diag;
  int32_t ncv;
  int32_t dbg;  // timing-only ablation switches (0 in production)
  // long tracks
  const LongHdr* lhdr;
  int32_t nlong, nchunks;
  const int32_t* cam_slot;  // [nc] reduced-system slot or -1
  double* wl;               // W scratch of the long tracks
  double* slab;             // slabs of the dense chunks (k_track_sweep_dense -> k_reduce_slabs)
  int32_t chunk0;           // first chunk of this launch (blockIdx.x + chunk0 indexes `chunks` and `part`)
  int32_t pad0_;
  const int32_t* order;     // k_track_sweep_dense: workgroup b takes chunk order[b] (heaviest first, dense_sweep_cost); NULL: chunk b + chunk0
  // outputs of the track sweep (accumulated, caller zeroes)
  BlockSky sky;    // where a block of S lives
  double* Sblk;    // block skyline of the upper block triangle, 36 doubles per block
  double* gc;      // [6 ncv] sum Jc^T r
  double* wv;      // [6 ncv] sum W Vinv g_p
  double* diagU;   // [6 ncv] diag(sum Jc^T Jc)
  double* part;    // [nchunks][4] cost, bad, max|g_p|, -
  double* diagV;   // DIAG mode: [np][3]
  // update sweep
  const double* yc;        // [6 ncv] reduced step (scaled coordinates)
  const double* camtab2;   // candidate cameras
  double* pts2;            // candidate landmarks
  double* part2;           // [nchunks][8]
  const LmCtl* ctl;        // inside a solve: trust-region radius and the stop flag live on the device (NULL: `radius` above)
  // k_track_sweep_dense as the first launch of an iteration (all chunks dense): what k_lm_prologue would do — an accepted
  // candidate becomes the state, the reduced buffer starts from zero — is spread over the sweep's workgroups
  int32_t adopt_on, adopt_nc;
  double* pts_rw; double* q_rw; double* t_rw; double* camtab_rw;
  const double* q2; const double* t2;
  double* red; int64_t nred;
  // direct form (DirectAsm): instead of the whole reduced buffer the workgroups zero what k_assemble would zero or overwrite — the
  // camera vectors (red / nred then cover gc | wv | diagU | scalars only), these blocks, and the listed tiles of the system
  double* zero_p[2]; int64_t zero_n[2];  // y | column-indexed diag U
  double* zero_A; const int32_t* zero_tiles; int32_t zero_ntiles;     // tiles of A (LevelPlanDev::d_asm_tiles)
  double* zero_P; const int32_t* zero_ptiles; int32_t zero_nptiles;   // inverse accumulators (LevelPlanDev::d_pinv_tiles)
  // hand-off of the landmark factors from the dense track sweep to the update sweep of the same iteration (all chunks dense, no
  // long tracks; NULL: the update sweep forms V_p, its factor and g_p again): 9 doubles per landmark, F = chol(V + D)^-1 as
  // spd3_inv_factor packs it, then g_p.  F[0] == 0 marks a failed factorisation; the slot of a constant landmark is never written
  double* pt_fac;
};
// k_update_sweep with the camera update in front (all chunks dense): every workgroup forms the candidate rows of ITS chunk's
// cameras in LDS, workgroup 0 also does what k_cam_update does for all cameras (candidate poses and table, step and state norms,
// gradient maximum, the factorisation's failure flag) — one launch less on the iteration's critical path
struct CamUpdArgs {
  int32_t fuse, nc;
  const int32_t* cam_slot;     // [nc] slot or -1
  const int32_t* cam_of_slot;  // [ncv]
  const double* q; const double* t; const double* cs; const double* gc;
  const double* intr; const int32_t* intr_idx;
  double* q2; double* t2; double* camtab2; double* scal; int* chol_fail;
};
__device__ inline bool lm_accepted(const LmCtl* c) { return c != nullptr && __hip_atomic_load(&c->accepted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0; }

struct CostArgs {
  int64_t nrec;
  const int32_t* rec_cam; const int32_t* rec_pt; const uint32_t* rec_meta; const double* rec_xy;
  const double* rec_d; const double* rec_m; const double* rec_a;
  const double* camtab; const double* pts;
  LossParams loss;
  double* part;  // [gridDim.x][4]: reproj cost, depth cost, bad
};

constexpr int kPanelWavesDefault = 4;
// second stream + events for the outer-panel look-ahead of the dense factorisation (dense_chol.hip)
struct DenseOverlap {
  int nb = 0;            // outer panel width in tile columns; 0: default (one panel up to 64 tile columns, else 8)
  bool big = true;       // LDS-staged 64x64 trailing update (false: per-tile workgroups, for A/B measurements)
  bool overlap = true;   // second-stream look-ahead
  bool no_level = false;    // per-step skyline path instead of the level-scheduled factorisation (A/B measurements)
  bool no_inverse = false;  // plain path: back substitution by groups instead of the inverse propagation (A/B measurements)
  int panel_waves = kPanelWavesDefault;  // waves that factor the stacked panel of a tile column: 4 or 1 (MPSFM_CHOL_PANEL_WAVES)
  bool entry_list = false;  // k_chol_level walks item -> srcs / rows -> operands instead of reading launch records (MPSFM_CHOL_ENTRY=list,
                            // the comparison path; read per solve)
  hipStream_t s2 = nullptr;
  hipEvent_t evF[4] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t evB[4] = {nullptr, nullptr, nullptr, nullptr};
};

// Device tables of the level-scheduled factorisation (chol_plan.h), static per handle.
struct LevelPlanDev {
  bool valid = false, use_pinv = false;
  const CholItem* d_items = nullptr;
  const LevelHead* d_heads = nullptr;  // one launch record per item (chol_plan.h)
  const int32_t* d_srcs = nullptr;
  const int32_t* d_rows = nullptr;
  const int32_t* d_struct_start = nullptr;
  const int32_t* d_struct_rows = nullptr;
  const int32_t* d_back_cols = nullptr;
  const int32_t* d_col_slot = nullptr;   // AssembleArgs::col_slot
  const int32_t* d_asm_tiles = nullptr;
  const uint8_t* d_tile_live = nullptr;  // [(nt+1)(nt+2)/2] 1 for the tiles in d_asm_tiles
  const int32_t* d_pinv_tiles = nullptr; // packed ids of the inverse accumulators the roles write: the others stay zero from the handle's
  int32_t n_pinv_tiles = 0;              // creation on (k_assemble zeroes all of them, the direct form these)
  const uint8_t* d_level0 = nullptr;     // [nt] 1: the tile column is factored in the first launch
  bool damp_in_launch0 = false;          // the first launch holds panel items without sources only (DampArgs)
  int32_t n_asm = 0, nlevels = 0;
  const int32_t* h_launch_start = nullptr;  // host: [nlevels + 1]
  const int32_t* h_back_start = nullptr;    // host: [nlevels + 1]
};

// The direct form of the front of the dense solve (every chunk dense, one rank, inverse propagation): k_reduce_slabs adds the sums
// of the slabs straight into the tiles of A — the element (R, C), R >= C, of the system at lt_tile(R >> 5, C >> 5) * 1024 +
// (R & 31) * 32 + (C & 31), mirrored inside a diagonal tile — and wv - gc into row 0 of tile row nt; no Sblk, no k_assemble.  A stays
// undamped: the first level launch adds the damping (DampArgs), from diag U by COLUMN — its panel items to the diagonal tile they
// factor, in registers, and a few workgroups more to the diagonal tiles of all later columns in memory (nothing else touches those in
// that launch: the first level has no trailing items), so that the later launches run the code they always ran.
struct DirectAsm {
  const RedDestCols* dests;  // per destination part: RedDest and where it lands
  double* A;
  double* diag_col;      // [32 nt] diag U by system column (padding columns stay zero)
  int32_t nt;
};
struct DampArgs {
  const double* diag_col;   // NULL: A is damped already (k_assemble)
  const int32_t* col_slot;  // LevelPlanDev::d_col_slot (NULL: no padding columns inside the system)
  const uint8_t* level0;    // [nt] 1: the tile column is factored in the first launch (LevelPlanDev::d_level0)
  int32_t n;
  double min_diag, max_diag, radius;  // radius: without a control block
};

struct AssembleArgs {
  BlockSky sky;
  const double* Sblk; const double* gc; const double* wv; const double* diagU;
  int32_t ncv, n, nt;
  double radius, min_diag, max_diag;
  double* A;     // tiles
  double* Pinv;  // accumulators of the inverse propagation (same tile indexing as A), zeroed here; may be NULL
  const int32_t* tile_list;  // packed ids of the tiles to assemble (one workgroup each), NULL: all (nt+1)(nt+2)/2
  int32_t n_list;
  const int32_t* col_slot;   // [n] slot * 8 + coordinate of every column of the system, -1: padding column (identity row);
                             // NULL: column c belongs to slot c / 6 (no padding).  Vectors (gc, wv, diagU, y) are indexed by slot.
  int32_t n_vec;             // 6 x slots: length of those vectors
  double* y;                 // solution vector (slot-indexed), zeroed here when the back substitution accumulates into it (else NULL)
  const uint8_t* live;       // all tiles launched (inverse accumulators to zero): per packed id, 0 = the factorisation never
                             // reads this tile of A, skip the gather; NULL: every tile is assembled
  const LmCtl* ctl;  // as in SweepArgs
};


}  // namespace mpsfm
