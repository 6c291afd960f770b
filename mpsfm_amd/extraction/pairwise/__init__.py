from .featuremap import NNs_sparse
from .nearest_neighbor import NearestNeighbor, match_descriptors
from .utils import assign_keypoints, sparse_nms, thin_dense_matches

__all__ = ["NNs_sparse", "NearestNeighbor", "assign_keypoints", "match_descriptors", "sparse_nms", "thin_dense_matches"]
