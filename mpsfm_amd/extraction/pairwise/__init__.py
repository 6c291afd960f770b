from .featuremap import NNs_sparse
from .nearest_neighbor import NearestNeighbor, match_descriptors
from .utils import assign_keypoints, sparse_nms, thin_dense_matches
from .warp import kpids_to_matches0, simple_nms, to_pixel_coordinates, warp_to_matches

__all__ = ["NNs_sparse", "NearestNeighbor", "assign_keypoints", "kpids_to_matches0", "match_descriptors", "simple_nms", "sparse_nms",
           "thin_dense_matches", "to_pixel_coordinates", "warp_to_matches"]
