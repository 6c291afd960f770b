from .absolute_pose import AbsolutePose
from .alignment import (
    estimate_rigid3d,
    estimate_rigid3d_robust,
    estimate_sim3d,
    estimate_sim3d_robust,
    register_depth_pair,
)
from .relative_pose import RelativePose
from .two_view_geometry import (
    TwoViewGeometry,
    TwoViewGeometryConfig,
    estimate_calibrated_two_view_geometry,
    estimate_calibrated_two_view_geometry_batch,
)

__all__ = ["AbsolutePose", "RelativePose", "TwoViewGeometry", "TwoViewGeometryConfig", "estimate_calibrated_two_view_geometry",
           "estimate_calibrated_two_view_geometry_batch", "estimate_rigid3d", "estimate_rigid3d_robust", "estimate_sim3d",
           "estimate_sim3d_robust", "register_depth_pair"]
