/*
 * eogs_gtprep.h — C-ABI of ground-truth preparation: pansharpening of the PAN target with the low-resolution MSI image,
 * the rescalers every ground-truth image goes through, and the PAN-side losses.
 *
 *   eogs_gtprep_pansharp        brovey_pansharp, simple_brovey     src/gaussiansplatting/pansharpening/algorithm/brovey.py
 *                               ihs_fusion                         src/gaussiansplatting/pansharpening/algorithm/ihs.py
 *   eogs_gtprep_pansharp_l2_*   Pansharploss                       src/gaussiansplatting/loss/pansharp_loss.py
 *   eogs_gtprep_l2_*            Lpan                               src/gaussiansplatting/loss/PAN_loss.py:5-13
 *   eogs_gtprep_grad_l2_*       Lgradient_pan                      src/gaussiansplatting/loss/PAN_loss.py:16-30
 *   eogs_gtprep_minmax, _rescale, _clamp, _equalize                src/gaussiansplatting/utils/rescaler/rescaler.py
 *
 * Same conventions as eogs_reg.h: plain DEVICE pointers + sizes, contiguous fp32, `void* stream` is a hipStream_t, int
 * status (0 ok, <0 error, message via eogs_rast_last_error()). Every entry only queues launches on the stream: no host
 * wait, no allocation, so a stream capture records it. Arguments are checked before anything touches a device. Every
 * sum is accumulated in float64 per workgroup and the partials are combined in a fixed order by one workgroup of the
 * last launch (no float atomics, a grid that depends on the shape alone): results are bitwise reproducible.
 *
 * Upsampling rule, shared by (a) and (b): torch's F.interpolate(size=(H, W), align_corners=False). Per axis, in fp32:
 * scale = in / out, src = scale * (dst + 0.5) - 0.5 with one rounding (a fused multiply-add, as the reference's builds do).
 *   bicubic   src is not clamped; i = floor(src), t = src - i; the four cubic-convolution weights with A = -0.75 on the
 *             taps i-1 .. i+2, each tap index clamped to [0, in-1]
 *   bilinear  src clamped to >= 0; i0 = int(src), i1 = min(i0 + 1, in-1), lambda = src - i0
 * Taps and weights are computed once per pixel and shared by the C channels.
 */
#ifndef EOGS_GTPREP_H_INCLUDED
#define EOGS_GTPREP_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The methods, u_c = channel c of the upsampled MSI image at the pixel, S = u_0 + u_1 + ... in channel order:
 *   BROVEY         bicubic;  d = max(weight * S, 1e-8) (a NaN stays a NaN);  out_c = (pan / d) * u_c
 *   SIMPLE_BROVEY  bilinear; out_c = u_c * (pan / (S + 1e-8))
 *   IHS            bilinear, C = 3; out_c = clamp(u_c + (pan - S / 3), 0, 1) (a NaN stays a NaN)
 * `weight` is read by BROVEY alone (the reference's W = 0.1). */
#define EOGS_GTPREP_BROVEY 0
#define EOGS_GTPREP_SIMPLE_BROVEY 1
#define EOGS_GTPREP_IHS 2
#define EOGS_GTPREP_MAX_CHANNELS 8

/* Workspace of the entries that take one, for images of C channels (the losses: C as given, at most
 * EOGS_GTPREP_MAX_CHANNELS; eogs_gtprep_l2_* and eogs_gtprep_grad_l2_*: C = 1). */
int eogs_gtprep_bytes(int C, size_t* bytes);

/* (a) msi f32[C][h][w], pan f32[H][W] -> out f32[C][H][W], one kernel. 1 <= C <= EOGS_GTPREP_MAX_CHANNELS. */
int eogs_gtprep_pansharp(int method, int C, int h, int w, int H, int W, const float* msi, const float* pan, float weight,
                         float* out, void* stream);

/* (b) Pansharploss: out f32[1] = mean over C*H*W of (syn - target)^2 with target the value of (a), computed on the fly
 * and never stored. syn f32[C][H][W]. */
int eogs_gtprep_pansharp_l2_forward(int method, int C, int h, int w, int H, int W, const float* syn, const float* msi,
                                    const float* pan, float weight, float* out, void* ws, size_t ws_bytes, void* stream);

/* g_syn f32[C][H][W] = 2 (syn - target) / (C H W) * upstream, fully overwritten. `upstream` is a device scalar, NULL = 1. */
int eogs_gtprep_pansharp_l2_backward(int method, int C, int h, int w, int H, int W, const float* syn, const float* msi,
                                     const float* pan, float weight, const float* upstream, float* g_syn, void* stream);

/* Lpan: the same kernels with the target given. image, target f32[n]; out f32[1] = mean (image - target)^2. */
int eogs_gtprep_l2_forward(int64_t n, const float* image, const float* target, float* out, void* ws, size_t ws_bytes,
                           void* stream);
int eogs_gtprep_l2_backward(int64_t n, const float* image, const float* target, const float* upstream, float* g_image,
                            void* stream);

/* (c) Lgradient_pan over B planes [H][W] (B = the product of the leading dimensions), d = pan - gt:
 *   out f32[1] = mean(gy(d)^2) + mean(gx(d)^2), both means over B*H*W
 * g = torch.gradient with unit spacing and edge order 1: (f[i+1] - f[i-1]) / 2 inside, f[1] - f[0] and f[n-1] - f[n-2]
 * at the ends. H < 2 or W < 2 is refused. Backward is the transposed stencil written as a gather: g_pan f32[B][H][W]
 * fully overwritten, `upstream` a device scalar, NULL = 1. */
int eogs_gtprep_grad_l2_forward(int64_t B, int H, int W, const float* pan, const float* gt, float* out, void* ws,
                                size_t ws_bytes, void* stream);
int eogs_gtprep_grad_l2_backward(int64_t B, int H, int W, const float* pan, const float* gt, const float* upstream,
                                 float* g_pan, void* stream);

/* (d) Rescalers over x f32[C][n] (n = H*W). minmax writes mm f32[C][2] = {min, max} per channel with torch.min/max's NaN
 * rule: a channel that holds a NaN has NaN extrema. rescale: out = (x - min_c) / ((max_c - min_c) + 1e-8f), with mm read
 * on the device (out may be x). clamp: out = min(max(x, lo), hi), a NaN stays a NaN (out may be x). The library is built
 * with -ffp-contract=off and correctly rounded division: these equal the fp32 torch expressions bit for bit. */
int eogs_gtprep_minmax(int C, int64_t n, const float* x, float* mm, void* ws, size_t ws_bytes, void* stream);
int eogs_gtprep_rescale(int C, int64_t n, const float* x, const float* mm, float* out, void* stream);
int eogs_gtprep_clamp(int64_t n, const float* x, float lo, float hi, float* out, void* stream);

/* (e) Histogram equalisation per channel, integers only. v = uint8(x * 255): the product in fp32, a NaN becomes 0, then
 * clamped to [0, 255] and truncated. With hist the 256-bin histogram of v over the channel:
 *   step = (sum of the non-empty bins except the last non-empty one) floor-divided by 255
 *   step == 0: lut[v] = v; otherwise lut[0] = 0, lut[v] = clamp((cumsum[v-1] + step / 2) / step, 0, 255)
 *   out = float(lut[v]) / 255
 * The step == 0 decision is made on the device. n < 2^31. out must not overlap x. */
int eogs_gtprep_equalize(int C, int64_t n, const float* x, float* out, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EOGS_GTPREP_H_INCLUDED */
