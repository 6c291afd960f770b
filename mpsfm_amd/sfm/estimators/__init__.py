from .absolute_pose import AbsolutePose
from .relative_pose import RelativePose
from .two_view_geometry import (
    TwoViewGeometry,
    TwoViewGeometryConfig,
    estimate_calibrated_two_view_geometry,
    estimate_calibrated_two_view_geometry_batch,
)

__all__ = ["AbsolutePose", "RelativePose", "TwoViewGeometry", "TwoViewGeometryConfig", "estimate_calibrated_two_view_geometry",
           "estimate_calibrated_two_view_geometry_batch"]
