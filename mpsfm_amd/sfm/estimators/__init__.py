from .absolute_pose import AbsolutePose
from .alignment import (
    depth_to_normals,
    estimate_rigid3d,
    estimate_rigid3d_robust,
    estimate_sim3d,
    estimate_sim3d_robust,
    refine_depth_pair,
    register_depth_pair,
    register_depth_pair_dense,
)
from .relative_pose import RelativePose
from .two_view_geometry import (
    TwoViewGeometry,
    TwoViewGeometryConfig,
    estimate_calibrated_two_view_geometry,
    estimate_calibrated_two_view_geometry_batch,
)

__all__ = ["AbsolutePose", "RelativePose", "TwoViewGeometry", "TwoViewGeometryConfig", "depth_to_normals",
           "estimate_calibrated_two_view_geometry", "estimate_calibrated_two_view_geometry_batch", "estimate_rigid3d",
           "estimate_rigid3d_robust", "estimate_sim3d", "estimate_sim3d_robust", "refine_depth_pair", "register_depth_pair",
           "register_depth_pair_dense"]
