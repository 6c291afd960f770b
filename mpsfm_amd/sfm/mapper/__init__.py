from .depthconsistency import DepthConsistencyChecker
from .registration import MpsfmRegistration

__all__ = ["DepthConsistencyChecker", "MpsfmRegistration"]
