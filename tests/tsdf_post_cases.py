"""TEST INFRASTRUCTURE — restatement of the reference's TSDF stages around `integrate` (checker for eogs_tsdf_normals /
_prior / _surface, include/eogs_tsdf.h), statement by statement, with torch ops in the dtype handed in:
  RangeImageEOGS.__init__ / reconstruct_normals / get_weights   src/gaussiansplatting/tsdf.py:213-231, 243-323
  TSDFVolume.apply_prior                                         tsdf.py:602-638
  TSDFVolume.extract_dsm up to the plyflatten call               tsdf.py:530-562
Pinned against vectors the reference's own tsdf.py produced (tests/golden/make_golden_tsdf_post.py,
tests/test_tsdf_post_oracle.py). Two statements are restated by equivalent ops: einops.rearrange as view + permute (pure
data movement), and the single-channel conv3d of apply_prior as a sum of 27 shifted zero-padded copies of the occupancy (0/1
summands: the counts are small integers, exact in fp32 in any order; conv3d on the GPU goes through MIOpen, which compiles
its kernels at first use). The np.indices z coordinate is arange(nz), broadcast.
"""
import torch
import torch.nn.functional as F


def view_direction(coef):
    """tsdf.py:213-218."""
    v = torch.linalg.solve(coef, torch.tensor([0, 0, 1.0], dtype=coef.dtype, device=coef.device))
    return F.normalize(v, dim=0, eps=1e-6)


def world_positions(alt, coef, intercept):
    """tsdf.py:245-263: [1, 3, H, W] world position of every pixel (view coordinates with align_corners=False pixel centres)."""
    dt, dev = alt.dtype, alt.device
    H, W = alt.shape[-2:]
    u = torch.arange(W, dtype=dt, device=dev)
    v = torch.arange(H, dtype=dt, device=dev)
    U, V = torch.meshgrid(u, v, indexing="ij")
    UVA = torch.stack([U, V, alt.reshape(H, W).T], axis=-1)
    view = (UVA + torch.tensor([0.5, 0.5, 0], dtype=dt, device=dev)) * torch.tensor([1 / W, 1 / H, 1], dtype=dt, device=dev)
    view[..., :2] = view[..., :2] * 2 - 1
    Ainv = torch.linalg.inv(coef)
    Ainvb = Ainv @ intercept
    world_pos = F.linear(view, Ainv, -Ainvb)
    return world_pos.permute(2, 1, 0)[None]  # "w h c -> 1 c h w"


def windows(world_pos):
    """tsdf.py:265-275: F.unfold(5 x 5, zero padding 2) rearranged to [1, c, h, w, k1, k2]."""
    _, _, H, W = world_pos.shape
    win = F.unfold(world_pos, kernel_size=(5, 5), dilation=1, padding=2, stride=1)
    return win.view(1, 3, 5, 5, H, W).permute(0, 1, 4, 5, 2, 3)


def branch_errors(win):
    """tsdf.py:280-313: (error_left_x, error_right_x, error_left_y, error_right_y), each [1, H, W]."""
    c = win[..., 2, 2]
    pl_x = win[..., 2, 0] + 2 * (win[..., 2, 1] - win[..., 2, 0])
    pr_x = win[..., 2, 4] + 2 * (win[..., 2, 3] - win[..., 2, 4])
    pl_y = win[..., 0, 2] + 2 * (win[..., 1, 2] - win[..., 0, 2])
    pr_y = win[..., 4, 2] + 2 * (win[..., 3, 2] - win[..., 4, 2])
    n = lambda t: torch.linalg.vector_norm(t - c, dim=1)
    return n(pl_x), n(pr_x), n(pl_y), n(pr_y)


def reconstruct(alt, coef, intercept, left_x=None, left_y=None):
    """tsdf.py:213-231, 243-323. Returns (view_direction, pixels_normals [1,3,H,W], pixels_angle [1,1,H,W], weights).
    `left_x` / `left_y` ([1, H, W] bool) replace the branch comparisons where given (the tests evaluate the other branch
    of a near-tie)."""
    vd = view_direction(coef)
    win = windows(world_positions(alt, coef, intercept))
    el_x, er_x, el_y, er_y = branch_errors(win)
    lx = el_x < er_x if left_x is None else left_x
    ly = el_y < er_y if left_y is None else left_y
    dx = torch.where(lx, (win[..., 2, 2] - win[..., 2, 0]) * 0.5, (win[..., 2, 4] - win[..., 2, 2]) * 0.5)
    dy = torch.where(ly, (win[..., 2, 2] - win[..., 0, 2]) * 0.5, (win[..., 4, 2] - win[..., 2, 2]) * 0.5)
    normals = F.normalize(torch.cross(dx, dy, dim=1), dim=1, eps=1e-6)
    angle = torch.einsum("bchw,c->bhw", normals, -vd).unsqueeze(1)
    return vd, normals, angle, angle.clamp(min=0.0, max=1.0)


def occupancy_count(occ):
    """conv3d(occ, ones(3, 3, 3), padding=1) of a bool volume [nx, ny, nz], as float."""
    o = F.pad(occ.to(torch.float32)[None], (1, 1, 1, 1, 1, 1))[0]
    nx, ny, nz = occ.shape
    cnt = torch.zeros(occ.shape, dtype=torch.float32, device=occ.device)
    for dx in range(3):
        for dy in range(3):
            for dz in range(3):
                cnt += o[dx:dx + nx, dy:dy + ny, dz:dz + nz]
    return cnt


def apply_prior(tsdf_vol, weight_vol):
    """tsdf.py:602-638. Returns new (tsdf_vol, weight_vol); the inputs are untouched."""
    t, w = tsdf_vol.clone(), weight_vol.clone()
    untouched = (w == 0) & (t == 1.0)
    occ = t <= 0
    t[:, :, 0] = -1.0
    w[:, :, 0] = 1.0
    isolated = (occupancy_count(occ) == 1) & occ
    t[isolated] = 1.0
    w[isolated] = 0.0
    idx = torch.arange(0, t.shape[-1], device=t.device)
    indices = torch.argmax(occ * idx, dim=-1, keepdim=False)
    mask = (idx < indices.unsqueeze(-1)) & untouched
    t[mask] = -1.0
    w[mask] = 1.0
    return t, w


def surface(tsdf_vol, z_axis):
    """tsdf.py:530-535: (indices int64 [nx, ny], z_axis[indices])."""
    idx = torch.arange(0, tsdf_vol.shape[-1], device=tsdf_vol.device)
    indices = torch.argmax((tsdf_vol < 0) * idx, dim=-1, keepdim=False)
    return indices, z_axis[indices]


def surface_cloud(axes, z_values, center):
    """tsdf.py:538-556: the float64 [nx * ny, 3] array handed to plyflatten."""
    xy = torch.stack(torch.meshgrid([axes[0], axes[1]], indexing="ij"), dim=-1)
    cloud = torch.cat([xy, z_values.unsqueeze(-1)], dim=-1).detach().cpu().reshape(-1, 3).numpy()
    return cloud + center
