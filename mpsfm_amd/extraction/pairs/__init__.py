"""Which image pairs to match (reference: mpsfm/extraction/pairs/): by retrieval over global descriptors on the GPU, all of them,
or neighbours in a sequence.  The in-memory half: a feature "file" is a mapping name -> {"global_descriptor": [D]}; HDF5 stays
with the reference."""

from .base import pairs_from_sequential
from .pairs_from_exhaustive import main as pairs_from_exhaustive
from .pairs_from_retrieval import main as pairs_from_retrieval

__all__ = ["pairs_from_exhaustive", "pairs_from_retrieval", "pairs_from_sequential"]
