"""Drop-ins for the reference's posterior pictures, drawn on the device (epropnp.posterior: orient_density, bev_density).

`draw_orient_density` has the name, signature and return value of EPro-PnP-6DoF lib/utils/draw_orient_density.py (called at
lib/test.py:219-225) and needs no cv2: the image is finished on the device and copied to the host once.  Its axis lines follow
`posterior.orient_density`'s rule (within 1.5 px of the segment), not OpenCV's rasteriser.
`bev_density_layer` is the colour layer that `show_bev` (EPro-PnP-Det core/visualizer/image_bev_vis.py:79-95) multiplies its
canvas with, from `posterior.bev_density`'s output.
"""
import torch

from . import posterior


def draw_orient_density(pose_opt, pose_samples, pose_sample_logweights, size=512,
                        saturation=0.5, sphere_opacity=0.6, sample_kernel=(5, 5), intensity_scale=50):
    """-> numpy (bs, size, size, 3) float32, as the reference's function of this name.  pose_opt=None draws no axis lines."""
    res = posterior.orient_density(pose_samples, pose_sample_logweights, pose_opt=pose_opt, size=size, window=sample_kernel,
                                   saturation=saturation, sphere_opacity=sphere_opacity, intensity_scale=intensity_scale)
    return res.image.cpu().numpy()


def bev_density_layer(density, sample_color=(0.9, 0.5, 0.1)):
    """(..., H, W) density -> (..., H, W, 3) layer `sample_color ** density`: 1 where nothing was sampled."""
    color = torch.as_tensor(sample_color, dtype=density.dtype, device=density.device)
    return color ** density[..., None]
