"""CPU oracle of the virtual-camera resample — TEST INFRASTRUCTURE ONLY (never imported by eogs2_amd/).

The reference's own three statements (src/gaussiansplatting/gaussian_renderer/renderer_cc_shadow.py:32-50), in float64,
on top of torch.nn.functional.grid_sample — the third-party routine the reference itself calls (PyTorch 2.x ATen
grid_sampler_2d, bilinear, zeros padding, align_corners=True). Gradients via autograd.

`n_keep` (1..5) and `fill_channel` (-1: none) generalise the reference's "four channels, -100 into the fourth" to what
eogs2_amd.resample.resample accepts; the defaults are the reference's.
"""
import torch


def resample(virtual_render, cam2virt, rendered_uva, n_keep=4, fill_channel=3):
    vr, M, uva = virtual_render.double(), cam2virt.double(), rendered_uva.double()
    assert 1 <= n_keep <= min(5, vr.shape[0]) and -1 <= fill_channel < n_keep
    virtual_uv = torch.einsum("...ij,...j->...i", M, uva)[..., :2]
    s = torch.nn.functional.grid_sample(vr.unsqueeze(0), virtual_uv.unsqueeze(0), align_corners=True).squeeze(0)[:n_keep]
    if fill_channel >= 0:  # `alt[mask] = -100`
        outside = (virtual_uv.abs() > 1).any(-1)
        s = torch.cat([torch.where(outside, torch.full_like(c, -100.0), c)[None] if k == fill_channel else c[None]
                       for k, c in enumerate(s)], 0)
    return s, virtual_uv
