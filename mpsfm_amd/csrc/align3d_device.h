// What align3d.hip offers to another entry point that continues on the same device scope (depth_icp.hip's
// mpsfm_depth_pair_register_dense): the argument check and the device part of mpsfm_depth_pair_register.
#pragma once
#include "call_scope.h"

namespace mpsfm {

// a depth map on the device with its PINHOLE intrinsics
struct A3Map { const double* depth; int32_t H, W; double intr[4]; };

// zeroes *result, then mpsfm_depth_pair_register's MPSFM_EINVAL cases; 0: the arguments are fine (m may be 0)
int a3_register_check(int32_t H0, int32_t W0, const double* depth0, const double* intr0, int32_t H1, int32_t W1, const double* depth1,
                      const double* intr1, int64_t n0, const double* xy0, int64_t n1, const double* xy1, int64_t m, const int32_t* matches,
                      int32_t with_scale, const mpsfm_align3d_options* options, uint8_t* valid, uint8_t* inlier_mask, double* lifted0,
                      double* lifted1, mpsfm_align3d_result* result);

// mpsfm_depth_pair_register behind its checks (m > 0) on the open, timed scope A; everything but result->ms is filled, the
// stream is idle on return and map0 / map1 (may be NULL) receive the maps as uploaded, alive as long as A
int a3_register_device(CallScope& A, int32_t H0, int32_t W0, const double* depth0, const double* intr0, int32_t H1, int32_t W1,
                       const double* depth1, const double* intr1, int64_t n0, const double* xy0, int64_t n1, const double* xy1, int64_t m,
                       const int32_t* matches, int32_t with_scale, const mpsfm_align3d_options* options, uint8_t* valid, uint8_t* inlier_mask,
                       double* lifted0, double* lifted1, mpsfm_align3d_result* result, A3Map* map0, A3Map* map1);

}  // namespace mpsfm
