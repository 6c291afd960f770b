from .absolute_pose import AbsolutePose
from .relative_pose import RelativePose

__all__ = ["AbsolutePose", "RelativePose"]
