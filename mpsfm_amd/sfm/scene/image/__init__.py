"""Per-image monocular priors with the reference's class names (mpsfm/sfm/scene/image/depth.py, normals.py): the maps
are built on the GPU by ``mpsfm_depth_priors`` / ``mpsfm_normal_priors``, one batched call per kind for any number of
images (``prepare_mono_priors``); a single construction is a batch of one.  No CPU fallback."""

from .depth import Depth
from .mono import prepare_mono_priors
from .normals import Normals

__all__ = ["Depth", "Normals", "prepare_mono_priors"]
