from .absolute_pose import AbsolutePose

__all__ = ["AbsolutePose"]
