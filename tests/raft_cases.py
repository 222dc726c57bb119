"""Cases and the float64 oracle of the correlation lookup and the flow upsampling (eogs2_amd.raft, include/eogs_resample.h),
shared by the CPU tests (tests/test_raft_cases.py pins the oracle itself) and the GPU test (tests/test_gpu_raft.py).
Everything is computed from seeds: no fixture, nothing outside the repository.

The oracle states the lookup twice:

  lookup_volume   RAFT's own: the all-pairs volume (matmul), avg_pool2d over the second map's positions,
                  grid_sample(bilinear, align_corners=True, zeros) at coords / 2^l + (d_i, d_j), i offsetting x
  lookup_pooled   the statement of include/eogs_resample.h: pooled FEATURES, (2r+2)^2 dots per pixel and level, exactly 0
                  outside the level, one 2 x 2 blend per tap with the pixel's shared fraction; with `magnitude=True` the
                  same blend of sum_c |fmap1_c| pool_l(|fmap2|)_c / sqrt(C): the M of the error bound

Both work on any device, in the dtype of their inputs (the tests pass float64)."""
import math

import torch
import torch.nn.functional as F

# (N, h, w): 16 x 16 is the smallest map with four levels of at least 2 x 2; 17 x 19 drops a row or a column at every level
MAPS = ((1, 16, 16), (1, 17, 19), (2, 24, 40), (2, 40, 24))
CONFIGS = ((128, 3), (256, 4))  # (C, radius) of RAFT-small and RAFT-large
CPU_CONFIG = (8, 3)             # the CPU self-check of the oracle
LEVELS = 4
FAMILIES = ("zero", "smooth", "integers", "edges", "far", "checker", "outlier")


def features(N, C, h, w, seed):
    """(fmap1, fmap2) float64 [N, C, h, w], correlated so that the dot products are not all noise."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(N, C, h, w, generator=g, dtype=torch.float64)
    b = 0.6 * torch.roll(a, shifts=(1, -2), dims=(2, 3)) + 0.8 * torch.randn(N, C, h, w, generator=g, dtype=torch.float64)
    return a, b


def coords(family, N, h, w, seed=0):
    """float32 [N, 2, h, w] lookup coordinates (plane 0 x, plane 1 y) = the pixel grid + a flow of the family."""
    g = torch.Generator().manual_seed(1000 + seed)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    grid = torch.stack([xs, ys])[None].repeat(N, 1, 1, 1)
    smooth = torch.stack([0.7 * torch.sin(0.31 * xs + 0.17 * ys), 0.6 * torch.cos(0.23 * xs - 0.29 * ys)])[None].repeat(N, 1, 1, 1)
    if family == "zero":
        return grid
    if family == "smooth":  # sub-pixel
        return grid + smooth
    if family == "integers":  # the weights are exactly 0 and 1
        return grid + torch.randint(-3, 4, (N, 2, h, w), generator=g).float()
    if family == "edges":  # coordinates exactly on 0, w - 1 and h - 1
        c = grid.clone()
        c[:, 0] = torch.where(xs % 2 == 0, torch.zeros_like(xs), torch.full_like(xs, w - 1))
        c[:, 1] = torch.where(ys % 2 == 0, torch.zeros_like(ys), torch.full_like(ys, h - 1))
        return c
    if family == "far":  # +-1.5 w: most windows lie outside
        return grid + (torch.rand(N, 2, h, w, generator=g) * 2 - 1) * 1.5 * w
    if family == "checker":  # per pixel +-h: no bounding box fits LDS
        sign = torch.where((xs + ys) % 2 == 0, torch.ones_like(xs), -torch.ones_like(xs))
        return grid + sign * float(h) + 0.25
    if family == "outlier":  # one pixel with a far flow inside a smooth field
        c = grid + smooth
        c[:, 0, h // 2, w // 2] += 0.9 * w
        c[:, 1, h // 2, w // 2] -= 0.8 * h
        return c
    raise ValueError(family)


def pool(x, times):
    """avg_pool2d(., 2, 2) applied `times` times: floor sizes, a trailing odd row or column is dropped."""
    for _ in range(times):
        x = F.avg_pool2d(x, kernel_size=2, stride=2)
    return x


def lookup_volume(fmap1, fmap2, c, radius, levels=LEVELS):
    N, C, h, w = fmap1.shape
    K = 2 * radius + 1
    corr = torch.matmul(fmap1.reshape(N, C, h * w).transpose(1, 2), fmap2.reshape(N, C, h * w)) / math.sqrt(C)
    corr = corr.reshape(N * h * w, 1, h, w)
    d = torch.linspace(-radius, radius, K, dtype=fmap1.dtype, device=fmap1.device)
    delta = torch.stack(torch.meshgrid(d, d, indexing="ij"), dim=-1).view(1, K, K, 2)
    cc = c.to(fmap1.dtype).permute(0, 2, 3, 1).reshape(N * h * w, 1, 1, 2)
    out = []
    for l in range(levels):  # noqa: E741
        hl, wl = corr.shape[-2:]
        s = cc / 2 ** l + delta
        grid = torch.stack([2 * s[..., 0] / (wl - 1) - 1, 2 * s[..., 1] / (hl - 1) - 1], dim=-1)
        out.append(F.grid_sample(corr, grid, mode="bilinear", padding_mode="zeros", align_corners=True).view(N, h, w, K * K))
        corr = F.avg_pool2d(corr, kernel_size=2, stride=2)
    return torch.cat(out, dim=-1).permute(0, 3, 1, 2).contiguous()


def lookup_pooled(fmap1, fmap2, c, radius, levels=LEVELS, magnitude=False):
    """[N, levels K^2, h, w] by the statement of include/eogs_resample.h; returns (out, all_outside) where all_outside marks the
    elements whose four corners all lie outside their level."""
    N, C, h, w = fmap1.shape
    K, T = 2 * radius + 1, 2 * radius + 2
    dt, dev = fmap1.dtype, fmap1.device
    f1 = (fmap1.abs() if magnitude else fmap1).permute(0, 2, 3, 1)  # [N, h, w, C]
    nidx = torch.arange(N, device=dev).view(N, 1, 1).expand(N, h, w)
    outs, outside = [], []
    for l in range(levels):  # noqa: E741
        f2 = pool(fmap2.abs() if magnitude else fmap2, l)
        hl, wl = f2.shape[-2:]
        f2 = F.pad(f2, (1, 1, 1, 1)).permute(0, 2, 3, 1)  # a zero frame: every outside position reads it
        s = c.to(dt) * (0.5 ** l)  # exact
        fl = torch.floor(s)
        wgt = s - fl
        fx, fy, wx, wy = fl[:, 0], fl[:, 1], wgt[:, 0], wgt[:, 1]
        D = torch.zeros(T, T, N, h, w, dtype=dt, device=dev)
        inside = torch.zeros(T, T, N, h, w, dtype=torch.bool, device=dev)
        for a in range(T):
            x = fx - radius + a
            xin = (x >= 0) & (x < wl)
            xi = torch.where(xin, x, torch.full_like(x, -1)).long() + 1
            for b in range(T):
                y = fy - radius + b
                yin = (y >= 0) & (y < hl)
                yi = torch.where(yin, y, torch.full_like(y, -1)).long() + 1
                both = xin & yin
                rows = f2[nidx, torch.where(both, yi, torch.zeros_like(yi)), torch.where(both, xi, torch.zeros_like(xi))]
                D[a, b] = (f1 * rows).sum(-1) / math.sqrt(C)
                inside[a, b] = both
        o = torch.empty(N, K, K, h, w, dtype=dt, device=dev)
        ao = torch.empty(N, K, K, h, w, dtype=torch.bool, device=dev)
        for a in range(K):
            for b in range(K):
                o[:, a, b] = ((1 - wx) * (1 - wy) * D[a, b] + wx * (1 - wy) * D[a + 1, b] + (1 - wx) * wy * D[a, b + 1]
                              + wx * wy * D[a + 1, b + 1])
                ao[:, a, b] = ~(inside[a, b] | inside[a + 1, b] | inside[a, b + 1] | inside[a + 1, b + 1])
        outs.append(o.reshape(N, K * K, h, w))  # channel a K + b: the x offset is the slow index
        outside.append(ao.reshape(N, K * K, h, w))
    return torch.cat(outs, dim=1), torch.cat(outside, dim=1)


def lookup_level_of_channel(radius, levels=LEVELS):
    """int64 [levels K^2]: the level of every output channel."""
    K = 2 * radius + 1
    return torch.arange(levels).repeat_interleave(K * K)


# ---- upsampling ----

UP_SHAPES = ((1, 1, 1), (1, 5, 7), (1, 16, 16), (2, 5, 7))  # (N, h, w): at 1 x 1 every neighbour is padding
MASK_RANGE = 4.0  # mask logits lie in [-4, 4]: the bound of the convex mode counts on |v - max| <= 8


def upsample_inputs(N, h, w, seed):
    """(flow float64 [N, 2, h, w], mask float64 [N, 576, h, w]), both exactly representable in float32."""
    g = torch.Generator().manual_seed(2000 + seed)
    flow = (torch.randn(N, 2, h, w, generator=g) * 3).double()
    mask = ((torch.rand(N, 576, h, w, generator=g) * 2 - 1) * MASK_RANGE).double()
    return flow, mask


def convex_unfold(flow, mask):
    """RAFT's statement: softmax over the 9 taps, unfold of 8 flow, permute."""
    N, _, h, w = flow.shape
    m = torch.softmax(mask.view(N, 1, 9, 8, 8, h, w), dim=2)
    u = F.unfold(8 * flow, kernel_size=3, padding=1).view(N, 2, 9, 1, 1, h, w)
    return torch.sum(m * u, dim=2).permute(0, 1, 4, 2, 5, 3).reshape(N, 2, 8 * h, 8 * w)


def convex_direct(flow, mask, magnitude=False):
    """The statement of include/eogs_resample.h, element by element in loops over (k, i, j): out(8y + i, 8x + j) = sum_k
    softmax_k(mask[k 64 + i 8 + j]) 8 flow(y + k / 3 - 1, x + k % 3 - 1), zero padding. Returns (out, weights sum); with
    `magnitude` sum_k w_k |u_k|."""
    N, _, h, w = flow.shape
    u = 8 * (flow.abs() if magnitude else flow)
    up = F.pad(u, (1, 1, 1, 1))
    out = torch.zeros(N, 2, 8 * h, 8 * w, dtype=flow.dtype, device=flow.device)
    wsum = torch.zeros(N, 8 * h, 8 * w, dtype=flow.dtype, device=flow.device)
    m = mask.view(N, 9, 8, 8, h, w)
    wk = torch.softmax(m, dim=1)
    for k in range(9):
        nb = up[:, :, k // 3: k // 3 + h, k % 3: k % 3 + w]  # flow at (y + k / 3 - 1, x + k % 3 - 1)
        for i in range(8):
            for j in range(8):
                out[:, :, i::8, j::8] += wk[:, k, i, j][:, None] * nb
                wsum[:, i::8, j::8] += wk[:, k, i, j]
    return out, wsum


def bilinear(flow, magnitude=False):
    """8 interpolate(flow, scale_factor=8, bilinear, align_corners=True) (of |flow| with `magnitude`: the weights are
    non-negative, so that is sum_k w_k |u_k|)."""
    x = flow.abs() if magnitude else flow
    return 8 * F.interpolate(x, size=(8 * flow.shape[2], 8 * flow.shape[3]), mode="bilinear", align_corners=True)
