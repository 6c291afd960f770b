from .utils import assign_keypoints, sparse_nms, thin_dense_matches

__all__ = ["assign_keypoints", "sparse_nms", "thin_dense_matches"]
