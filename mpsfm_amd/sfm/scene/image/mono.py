"""``prepare_mono_priors``: the Depth and Normals of many images with ONE mpsfm_depth_priors and ONE mpsfm_normal_priors
call: what ``MpsfmReconstruction.initialize_mono_maps`` (reference reconstruction/mixins/init_utils.py:53-64) loops
over image by image."""

from __future__ import annotations

from .depth import Depth
from .normals import Normals


def prepare_mono_priors(items, depth_conf=None, normals_conf=None, device=0):
    """`items`: list of dicts(depth_dict=, normals_dict=, camera=, kps=, mask=None).  The normals of an image take the
    continuity mask of its depth, as ``Image.init_depth`` passes it on.  Returns [(Depth, Normals)] in the order of `items`."""
    from .... import capi

    items = list(items)
    dconf, nconf = Depth._merged_conf(depth_conf), Normals._merged_conf(normals_conf)
    dmaps = capi.depth_priors([Depth.problem(it["depth_dict"], it["camera"], it["kps"], it.get("mask")) for it in items], dconf, device=device)
    cont = [m["continuity_mask"] if dconf.use_continuity else None for m in dmaps]
    nmaps = capi.normal_priors([Normals.problem(it["normals_dict"], it["camera"], it.get("mask"), c) for it, c in zip(items, cont)], nconf,
                               device=device)
    return [(Depth(depth_conf, camera=it["camera"], kps=it["kps"], _maps=dm), Normals(normals_conf, camera=it["camera"], _maps=nm))
            for it, dm, nm in zip(items, dmaps, nmaps)]
