// Single-launch Levenberg-Marquardt for small problems (local bundle adjustment): the arguments of its launch (ba_launch.h), shared by ba_solver.hip and local_lm.hip.
#pragma once
#include "common.h"

namespace mpsfm {

constexpr int kLocalCams = 16;            // variable cameras the single-launch solver takes (three 32-column tiles)
constexpr int kLocalN = 6 * kLocalCams;   // reduced dimension, padded
// one dense accumulator of the reduced system: S (upper block triangle, row-major kLocalN x kLocalN) | g_c | W V^-1 g_p | diag U
constexpr int kLocalAccDoubles = kLocalN * kLocalN + 3 * kLocalN;

struct LocalArgs {
  SweepArgs A;            // tables and state of the handle (ctl = NULL: the radius travels in the workgroups' own control block)
  LmCtl* ctl;             // in: the initial control block; out: the final one with its traces
  LmOpts o;
  LmHead* log;            // [max_iterations + 2] control-block heads, one per iteration (verbose runs), or NULL
  double* acc[2];         // two zeroed accumulators of kLocalAccDoubles doubles (iterations alternate)
  double* part[2];        // [nchunks][4] track-sweep partial rows (cost, invalid count, gradient maximum), iterations alternate: a
                          // workgroup still reading iteration k's rows after barrier 2 never sees iteration k + 1's
  int32_t* bar;           // [0] arrivals of the grid barrier (monotonic), [1] abort flag; zeroed by the host
  long long* clk;         // [7] wall-clock ticks (100 MHz): sweep + flush, barrier 1, dense + cameras, update sweep, barrier 2, decision; iterations
                          // [11] ticks the skew hook waited (while it is armed; else the dense phase's last clock of debug flag 64)
  int32_t ncv, nc, nchunks, pad_;
  double* q; double* t;   // [nc][4], [nc][3] camera state, written back at the end
  double* camtab;         // [nc][kCamRec] likewise (A.camtab is its read-only view)
  double* pts;            // [np][3] landmark state (A.pts is its read-only view)
  const double* cs;       // [nc][6] camera column scales
  const double* fixed_parts;  // [2] cost of the fixed blocks (reprojection, depth): summed into the control block at the start
  // test hook (mpsfm_debug_local_skew): workgroup skew_chunk (modulo the grid, negative from the last) waits skew_ticks at the
  // phase points of skew_mask (kSkew*); 0: off
  int32_t skew_chunk, skew_mask;
  long long skew_ticks;
};
// the skew hook's phase points: after barrier 0 (the prologue's state-norm sum), start of an iteration (track sweep), after barrier 1
// (the reduced system), before the update sweep, after barrier 2 (the partial rows and the decision)
enum : int32_t { kSkewP = 1, kSkewA = 2, kSkewB = 4, kSkewD = 8, kSkewE = 16, kSkewAll = 31 };
constexpr long long kSkewMaxTicks = 200000;  // 2 ms of the 100 MHz wall clock, far below a grid barrier's bounded spin

}  // namespace mpsfm
