from .depthconsistency import DepthConsistencyChecker

__all__ = ["DepthConsistencyChecker"]
