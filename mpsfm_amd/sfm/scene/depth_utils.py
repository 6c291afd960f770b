"""Depth bookkeeping of a scene: the ``DepthUtils`` mixin of the reference's ``MpsfmReconstruction``
(mpsfm/sfm/scene/reconstruction/mixins/depth_utils.py:52-92), line by line.

Plain NumPy on host-resident maps: the work is elementwise, a round trip to the device would only add copies.  The
mixin needs ``self.images[imid].depth`` with the reference's attribute names (data, data_prior, uncertainty,
uncertainty_update, scale, shift, activated).  As in the reference, ``rescale_depths`` scales only
``uncertainty_update`` — the integrated map ``depth.data`` keeps its values — while ``normalize_depths`` also scales
``depth.data`` of the activated images.
"""

from __future__ import annotations


class DepthUtils:
    def activate_depths(self, imids):
        """Activates depths for images (:52-57)"""
        for imid in imids:
            if not self.images[imid].depth.activated:
                self.images[imid].depth.activated = True
                self.images[imid].depth.data = self.images[imid].depth.data_prior.copy()

    def _rescale_prior(self, imid, shift, scale):
        """Rescales depth prior (:59-64)"""
        depth = self.images[imid].depth
        depth.data_prior = depth.data_prior * scale + shift
        depth.scale *= scale
        depth.shift = depth.shift * scale + shift
        depth.uncertainty = depth.uncertainty * scale**2

    def _rescale_update(self, imid, shift, scale, rescale_depth=False):
        """Rescales optimized depth (:66-71)"""
        depth = self.images[imid].depth
        if rescale_depth and depth.activated:
            depth.data = depth.data * scale + shift
        depth.uncertainty_update = depth.uncertainty_update * scale**2

    def rescale_all(self, shift_scales):
        """Rescales all depths i.e. priors and optimized depths (:73-76)"""
        self.rescale_priors(shift_scales)
        self.rescale_depths(shift_scales)

    def rescale_depths(self, shift_scales):
        """Rescales optimized depths (:78-81)"""
        for imid, (shift, scale) in shift_scales.items():
            self._rescale_update(imid, shift, scale)

    def rescale_priors(self, shift_scales):
        """Rescales priors (:83-86)"""
        for imid, (shift, scale) in shift_scales.items():
            self._rescale_prior(imid, shift, scale)

    def normalize_depths(self, scale):
        """Normalizes depths (:88-92)"""
        for imid in self.images:
            self._rescale_prior(imid, 0, scale)
            self._rescale_update(imid, 0, scale, rescale_depth=True)
