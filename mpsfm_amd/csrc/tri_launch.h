// What tri_kernels.hip offers the other files that work on mpsfm_tracks (lift_tracks.hip): the tracks' device view, their
// check and upload, and the launch of k_filter.  Declarations only and no floating-point arithmetic: this header may be
// included on either side of a header that sets `#pragma clang fp contract`.  The defining file includes it too, so a
// definition that drifts from its declaration does not compile.
#pragma once
#include "common.h"
#include "call_scope.h"

namespace mpsfm {

struct TrackArgs {
  int32_t n_tracks;
  const double* q; const double* t; const double* intr; const int32_t* intr_idx;
  const int64_t* start; const int32_t* el_cam; const double* el_xy;
};

int check_tracks(const mpsfm_tracks* T);                             // MPSFM_EINVAL with a message, or 0
int upload_tracks(const mpsfm_tracks* T, CallScope& B, TrackArgs& a);  // copies on the call's stream
// k_filter over all tracks; any output may be NULL (it is then not computed)
void launch_filter_tracks(const TrackArgs& a, const double* xyz, double* max_angle, double* sq_err, uint8_t* front, hipStream_t st);

}  // namespace mpsfm
