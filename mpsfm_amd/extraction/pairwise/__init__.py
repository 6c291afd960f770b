from .featuremap import NNs_sparse
from .match_sparse import find_unique_new_pairs, match_pairs, names_to_pair, names_to_pair_old
from .nearest_neighbor import NearestNeighbor, match_descriptors
from .reciprocal import extract_correspondences, fast_reciprocal_NNs, map_keypoints_to_original_after_crop, merge_corres
from .utils import assign_keypoints, sparse_nms, thin_dense_matches
from .warp import kpids_to_matches0, simple_nms, to_pixel_coordinates, warp_to_matches

__all__ = ["NNs_sparse", "NearestNeighbor", "assign_keypoints", "extract_correspondences", "fast_reciprocal_NNs", "find_unique_new_pairs", "kpids_to_matches0",
           "map_keypoints_to_original_after_crop", "match_descriptors", "match_pairs", "merge_corres", "names_to_pair", "names_to_pair_old", "simple_nms", "sparse_nms", "thin_dense_matches",
           "to_pixel_coordinates", "warp_to_matches"]
