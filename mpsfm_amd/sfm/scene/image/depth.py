"""``Depth`` with the reference's interface (mpsfm/sfm/scene/image/depth.py:11-140): same ``default_conf``, same
constructor keywords, same attributes.  ``_init`` runs the prior construction on the GPU (a batch of one); many images
are built with one call by ``prepare_mono_priors``.

Deviations from the reference: the maps are float64 whatever the input's dtype; ``continuity_mask`` is also set when no
resize happens (the reference leaves it unset there and ``Image.init_depth`` then fails); the caller's ``depth_dict`` is
not modified (the reference writes the 0.1 fill into ``depth_dict["depth"]`` when no resize happens)."""

from __future__ import annotations

from ....baseclass import BaseClass
from ..priorutils import PriorUtils


class Depth(BaseClass, PriorUtils):
    """Depth prior of one image: prior map, variance, validity, continuity, variance at the keypoints."""

    default_conf = {
        "inherent_noise": 0.02,
        "std_multiplier": 1,
        "lc_std_multiplier": 10,
        "prior_std_multiplier": 3.33,
        "max_std": None,
        "use_continuity": True,
        "depth_lim": None,
        "fixed_uncertainty_val": 0.03,
        "fixed_uncertainty": False,
        "fill": True,
        "prior_uncertainty": True,  # use the variances the network predicts
        "flip_consistency": False,  # variance from the disagreement of the estimates on the image and on its mirror image
        "depth_uncertainty": 0.0263,  # floor of the standard deviation as a share of the depth
        "verbose": 0,
    }

    uncertainty_update_ap = None
    continuity_mask = None

    @staticmethod
    def problem(depth_dict, camera, kps, mask=None):
        """The per-image entry of capi.depth_priors."""
        item = {k: depth_dict[k] for k in ("depth", "depth2", "depth_variance", "depth_variance2", "valid", "valid2") if k in depth_dict}
        item.update(mask=mask, size=(camera.int_height, camera.int_width), kps=kps, sx=camera.sx, sy=camera.sy)
        return item

    def _init(self, depth_dict=None, camera=None, kps=None, mask=None, _maps=None, **kwargs):
        self.kps = kps
        self.camera = camera

        self.scale = 1
        self.shift = 0
        self.activated = False
        self.data = None
        if _maps is None:
            from .... import capi

            _maps = capi.depth_priors([self.problem(depth_dict, camera, kps, mask)], self.conf)[0]
        self.data_prior = _maps["data_prior"]
        self.uncertainty = _maps["uncertainty"]
        self.valid = _maps["valid"]
        self.continuity_mask = _maps["continuity_mask"] if self.conf.use_continuity else None
        self.uncertainty_update = _maps["uncertainty_update"]

    def reset(self):
        """Back to the unscaled, not activated prior."""
        self.data_prior /= self.scale
        self.uncertainty /= self.scale**2
        self.uncertainty_update = self.uncertainty_at_kps(self.kps)
        self.scale = 1
        self.shift = 0
        self.activated = False
        self.data = None
