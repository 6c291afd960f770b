"""``Normals`` with the reference's interface (mpsfm/sfm/scene/image/normals.py:137-246): same ``default_conf``, same
constructor keywords, same attributes (data, uncertainty, data_downscaled, uncertainty_downscaled), built on the GPU.

Deviations from the reference: float64 outputs; the caller's ``normals_dict`` is not modified (the reference resizes,
normalises and scales its entries in place)."""

from __future__ import annotations

import numpy as np

from ....baseclass import BaseClass
from ..priorutils import PriorUtils

large_number = 1e6


class Normals(BaseClass, PriorUtils):
    """Normal prior of one image: unit normals and their 3x3 covariances at full and at half size."""

    default_conf = {
        "inherent_polar_noise": np.pi / 180,
        "std_multiplier": 1,
        "lc_std_multiplier": 1,
        "prior_std_multiplier": 1,
        "downscale_factor": 2,
        "prior_uncertainty": True,  # use the variances the network predicts
        "flip_consistency": False,  # covariance from the disagreement of the estimates on the image and on its mirror image
        "verbose": 0,
    }

    @staticmethod
    def problem(normals_dict, camera, mask=None, continuity_mask=None):
        """The per-image entry of capi.normal_priors."""
        item = {k: normals_dict[k] for k in ("normals", "normals2", "normals_variance", "normals2_variance") if k in normals_dict}
        item.update(mask=mask, continuity_mask=continuity_mask, size=(camera.int_height, camera.int_width))
        return item

    def _init(self, normals_dict=None, camera=None, mask=None, continuity_mask=None, _maps=None, **kwargs):
        self.camera = camera
        if _maps is None:
            from .... import capi

            _maps = capi.normal_priors([self.problem(normals_dict, camera, mask, continuity_mask)], self.conf)[0]
        self.data = _maps["data"]
        self.uncertainty = _maps["uncertainty"]
        self.data_downscaled = _maps["data_downscaled"]
        self.uncertainty_downscaled = _maps["uncertainty_downscaled"]
