/*
 * eogs_resample.h — C-ABI of the fused virtual-camera resample (second piece).
 *
 * Replaces steps 2-3 of render_resample_virtual_camera
 * (src/gaussiansplatting/gaussian_renderer/renderer_cc_shadow.py:32-50):
 *     virtual_uv = einsum("...ij,...j->...i", cam2virt, rendered_uva)[..., :2]
 *     sample     = grid_sample(virtual_render[None], virtual_uv[None], align_corners=True)[0]   (bilinear, zeros padding)
 *     sample[3][(virtual_uv.abs() > 1).any(-1)] = -100
 * which PyTorch runs as stack / einsum / grid_sample / mask / index_put forward and their autograd backward
 * (1.2 ms per sun-camera resample at 1024^2 on the MI355X, twice per training iteration: train_pan.py:305-316,375-391).
 * Here: one kernel forward, one backward.
 *
 * Same conventions as eogs_rast.h (DEVICE pointers, `void* stream` = hipStream_t, int status, no allocation).
 *   virtual_render f32[C,Hv,Wv] planar (the virtual camera's render: rgb, altitude, accumulated opacity)
 *   uva            f32[H,W,3]  per output pixel (u, v, altitude) of the true camera   (train_pan.py:281)
 *   cam2virt       f32[9]      row-major 3x3 on the device (affine_cameras.py:360, 428-429)
 *   sample         f32[n_out,H,W]: the first n_out <= C channels of virtual_render resampled (the reference keeps 4)
 *   uv             f32[H,W,2]  the sampling coordinates (returned by the reference, used by its losses)
 *   fill_channel   channel of `sample` overwritten by fill_value where |u| > 1 or |v| > 1 (3 and -100 in the
 *                  reference); -1 disables
 */
#ifndef EOGS_RESAMPLE_H_INCLUDED
#define EOGS_RESAMPLE_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int eogs_resample_forward(int C, int Hv, int Wv, int H, int W, int n_out, const float* virtual_render,
                          const float* uva, const float* cam2virt, int fill_channel, float fill_value,
                          float* sample, float* uv, void* stream);

/* Backward workspace (bounding boxes of the cells touched by each 16x16 output tile). */
int eogs_resample_bytes(int H, int W, size_t* bytes);

/* Backward.
 *   dL_dsample f32[n_out,H,W]; dL_duv f32[H,W,2] or NULL
 *   dL_dvirtual f32[C,Hv,Wv]: fully overwritten. The four-tap scatter is evaluated as a gather per virtual tile (no global
 *     atomics) whose sums run in a fixed order — candidate tiles in tile order, the pixels of a cell in pixel order — so the
 *     result is bitwise reproducible run to run (PyTorch's grid_sampler_2d_backward, which the reference uses, is not).
 *     Exceptions: n_out > 4 or ws == NULL fall back to global fp32 atomic adds, and the round-2 form of the tile kernel
 *     (environment EOGS_RESAMPLE_BWD=1, a tuning aid) sums with LDS float atomics; neither fixes the last bit.
 *   dL_duva f32[H,W,3]: cam2virt[0:2,:]^T (dL_duv + the sampler's gradient with respect to the coordinates), fully overwritten
 * cam2virt itself receives no gradient (the reference derives it from fixed camera matrices). */
int eogs_resample_backward(int C, int Hv, int Wv, int H, int W, int n_out, const float* virtual_render,
                           const float* uva, const float* cam2virt, int fill_channel,
                           const float* dL_dsample, const float* dL_duv,
                           float* dL_dvirtual, float* dL_duva, void* ws, size_t ws_bytes, void* stream);

/* ---- flow-matching warp (flowmatching/flow_matching.py:225-269 of the reference) ----
 * The reference warps an image by a predicted optical flow as grid + flow, two normalisations, a permute and
 * grid_sample(bilinear, padding_mode="border", align_corners=True), with autograd's atomic scatter as backward. Here:
 *   img, out     f32[C,H,W] planar; H >= 2 and W >= 2 (the reference divides by W - 1)
 *   flow         f32, two planes (0: horizontal, 1: vertical, in pixels): element (k, y, x) lies at
 *                flow[k * plane_stride + y * row_stride + x * col_stride]. row_stride == col_stride == 0 names ONE
 *                displacement for the whole image (flow[0], flow[plane_stride]), read on the device
 *   gate         NULL, or one float on the device: where it is 0 the forward copies img and the backward copies dL_dout
 *                (the reference's host-side `if abs(flow).mean() < max_value_flow`, without the host)
 *   out[c][y][x] = bilinear sample of img[c] at (x + flow_x, y + flow_y) clamped to [0, W - 1] x [0, H - 1]
 * The flow receives no gradient (the reference detaches the grid). */
int eogs_resample_flow_forward(int C, int H, int W, const float* img, const float* flow, int64_t plane_stride,
                               int64_t row_stride, int64_t col_stride, const float* gate, float* out, void* stream);

/* Workspace of the backward for a flow FIELD (a constant displacement needs none: ws may be NULL). */
int eogs_resample_flow_bytes(int H, int W, size_t* bytes);

/* dL_dimg f32[C,H,W]: fully overwritten, no memset, no floating-point atomics, bitwise reproducible run to run. A field is
 * gathered through the buckets of eogs_resample_backward; a constant displacement through a closed-form gather. */
int eogs_resample_flow_backward(int C, int H, int W, const float* flow, int64_t plane_stride, int64_t row_stride,
                                int64_t col_stride, const float* gate, const float* dL_dout, float* dL_dimg, void* ws,
                                size_t ws_bytes, void* stream);

/* stats f32[5] = {mean x, mean y, mean |flow| over both planes, std x, std y} (std unbiased, as torch.std): one pass, sums in
 * double in a fixed order, bitwise reproducible (flow_matching.py:67-69,255-269,302; flow_matching_toaffine.py:13-14). */
int eogs_resample_flow_stats_bytes(int H, int W, size_t* bytes);
int eogs_resample_flow_stats(int H, int W, const float* flow, int64_t plane_stride, int64_t row_stride, int64_t col_stride,
                             float* stats, void* ws, size_t ws_bytes, void* stream);

/* ---- The flow network of the flow-matching step (RAFT; the reference takes it from torchvision, flowmatching/
 * flow_matching.py:76-86): the three operators it needs beside convolutions — the correlation between the two feature maps
 * looked up ON DEMAND, and the two ways RAFT brings its 1/8-resolution flow to the image's size. They live in this header,
 * beside the warp and the statistics of the same step.
 *
 * RAFT as published materialises the all-pairs correlation volume (n x n floats for n = h w feature positions, plus three
 * pooled levels) and reads it through grid_sample at every update. Here nothing quadratic is built: average-pooling the
 * correlation over the second image's positions equals correlating with the pooled features, and all (2r+1)^2 taps of a
 * pixel at a level share one fractional offset, so a lookup is (2r+2)^2 dot products per pixel and level against a small
 * feature pyramid, then one 2 x 2 blend per tap. Memory is linear in n. Everything is float32 and forward only. The library
 * never allocates and never waits for the device, arguments are checked before anything touches a device. No atomics and a
 * fixed order of every sum: results are bitwise reproducible. Device pointers must be 16-byte aligned. ---- */

#define EOGS_RAFT_MAX_LEVELS 4
#define EOGS_RAFT_MAX_RADIUS 4

/* eogs_raft_lookup flags: NO_STAGE forces the path that gathers straight from the pyramid (same bits, for tests and probes) */
#define EOGS_RAFT_NO_STAGE 1u

/* eogs_raft_upsample modes */
#define EOGS_RAFT_UP_CONVEX 0
#define EOGS_RAFT_UP_BILINEAR 1
#define EOGS_RAFT_MASK_CHANNELS 576

/* The feature pyramid of a map f32[N][C][h][w]: level l is avg_pool2d(., 2, 2) applied l times, h_l = h >> l, w_l = w >> l (a
 * trailing odd row or column is dropped), every level CHANNEL-LAST f32[N][h_l][w_l][C], level after level in one workspace,
 * each level's start rounded up to 256 bytes. Level 0 is the map itself, so levels = 1 is the channel-last copy the lookup
 * wants of the first map. eogs_raft_bytes gives the workspace's size; eogs_raft_level_offset the byte offset of a level.
 * Each level is pooled from the one above as ((a + b) + (c + d)) * 0.25 over (2y, 2x), (2y, 2x+1), (2y+1, 2x), (2y+1, 2x+1).
 *
 * Refused: N, C, h or w below 1; C not a multiple of 4; levels outside [1, 4]; a level that would be empty (h >> (levels - 1)
 * or w >> (levels - 1) is 0); N above 65535; more than 2^31 - 1 elements in a map; a workspace too small; NULL. */
int eogs_raft_bytes(int N, int C, int h, int w, int levels, size_t* bytes);
int eogs_raft_level_offset(int N, int C, int h, int w, int level, size_t* offset);
int eogs_raft_pyramid(int N, int C, int h, int w, int levels, const float* fmap, void* pyramid, size_t pyramid_bytes,
                      void* stream);

/* The correlation lookup. fmap1_cl: eogs_raft_pyramid(levels = 1) of the first map; pyramid: eogs_raft_pyramid(levels) of the
 * second; coords f32[N][2][h][w], plane 0 x and plane 1 y, in pixels of level 0; out f32[N][levels K^2][h][w], K = 2 radius + 1,
 * fully overwritten. For pixel p and level l, per axis
 *
 *   s = coords * 2^-l,  f = floor(s),  w = s - f
 *   D[a][b] = <fmap1(p), fmap2_l(f_x - r + a, f_y - r + b)> / sqrt(C)   for a, b in [0, 2r + 1]; exactly 0 where the position
 *                                                                        lies outside [0, w_l) x [0, h_l)
 *   out[l K^2 + a K + b] = (1-w_x)(1-w_y) D[a][b] + w_x (1-w_y) D[a+1][b] + (1-w_x) w_y D[a][b+1] + w_x w_y D[a+1][b+1]
 *
 * The x offset a is the slow index. A coordinate whose floor is not within [-(r + 2), n_l + r + 1] (NaN, +-inf, +-1e30 among
 * them) has every tap outside and weight 0: its outputs at that level are exactly 0. The dot product runs over the channels
 * in ascending order, one fused multiply-add per channel, on both paths: a workgroup stages the bounding box of its tile's
 * windows into LDS when it fits (eogs_raft_stage_info) and gathers from the pyramid otherwise, bit for bit the same.
 *
 * Refused: what eogs_raft_bytes refuses; radius outside [1, 4]; unknown flags; NULL; a pointer not 16-byte aligned. */
int eogs_raft_lookup(int N, int C, int h, int w, int levels, int radius, const float* fmap1_cl, const void* pyramid,
                     const float* coords, float* out, unsigned flags, void* stream);

/* The lookup's tiling, for tests and probes: a workgroup owns tile_w x tile_h pixels at one level and stages its windows'
 * bounding box when that holds at most max_positions positions of the level. */
int eogs_raft_stage_info(int* tile_w, int* tile_h, int* max_positions);

/* Flow f32[N][2][h][w] at 1/8 resolution to out f32[N][2][8h][8w].
 *   EOGS_RAFT_UP_CONVEX    mask f32[N][576][h][w]: for output (8y + i, 8x + j) a softmax over the 9 mask channels
 *                          k 64 + i 8 + j of pixel (y, x) weighs 8 flow over the zero-padded 3 x 3 neighbourhood
 *                          (y + k / 3 - 1, x + k % 3 - 1)
 *   EOGS_RAFT_UP_BILINEAR  8 * interpolate(flow, scale_factor = 8, bilinear, align_corners = True); mask must be NULL. The
 *                          source position Y (h - 1) / (8h - 1) is split into integer and fraction in integer arithmetic.
 * Refused: N, h or w below 1; h or w above 8192; N above 65535; an unknown mode; a mask that does not fit the mode; NULL; a
 * pointer not 16-byte aligned. */
int eogs_raft_upsample(int N, int h, int w, int mode, const float* flow, const float* mask, float* out, void* stream);

/* ---- The convolutions of RAFT-small's update block (motion encoder, ConvGRU, flow head): one channel-last convolution on
 * the exact-fp32 matrix instruction, and the update step composed of eight launches of it. Float32, forward only. The
 * conventions are those above: no allocation, no waiting, every argument checked before anything touches a device, the
 * stream last, device pointers 16-byte aligned, no atomics and a fixed order of every sum (bitwise reproducible; a batch
 * gives the bits of its single images). seg_channels, seg_offsets and params are HOST arrays.
 *
 * The convolution: stride 1, zero padding (k - 1) / 2, a cross-correlation as nn.Conv2d's. Its input is the channel
 * concatenation of nseg <= 3 maps in_i f32[N][h][w][C_i] (no concatenated copy is made), in_i = NULL beyond nseg:
 *
 *   v[n][y][x][c] = ((sum over (i, ch, ky, kx) of in_i[n][y + ky - p][x + kx - p][ch] W[c][off_i + ch][ky][kx]) + bias[c]) + add[n][y][x][c]
 *
 * with bias and add (f32[N][h][w][Cout]) optional. The sum takes the segments in order, their channels in chunks of eight,
 * per chunk the taps in row-major order and per tap the chunk's channels ascending, one fused multiply-add per product.
 * Epilogues:
 *   EOGS_FLOWNET_EPI_BIAS   out = v
 *   EOGS_FLOWNET_EPI_RELU   out = v < 0 ? 0 : v (a NaN stays a NaN)
 *   EOGS_FLOWNET_EPI_GATES  Cout even, aux = h f32[N][h][w][Cout / 2]; out is two maps f32[2][N][h][w][Cout / 2]:
 *                           out[0] = sigmoid(v[..., :Cout / 2]) (z), out[1] = sigmoid(v[..., Cout / 2:]) * h (r * h)
 *   EOGS_FLOWNET_EPI_GRU    aux = z f32[N][h][w][Cout]; out holds h and is updated in place: h = (1 - z) h + z tanh(v).
 *                           out must not be one of the inputs.
 * Flags: EOGS_FLOWNET_IN0_NCHW << i reads in_i as f32[N][C_i][h][w] (what a torch convolution or the correlation lookup
 * leaves); EOGS_FLOWNET_OUT_NCHW writes out as f32[N][Cout][h][w] (BIAS and RELU only: the flow head's 128 -> 2 tail writes
 * delta this way).
 *
 * Weights are repacked from torch's f32[cout_n][cin][k][k] by eogs_flownet_conv_pack into the kernel's tap-major layout
 * (eogs_flownet_conv_pack_bytes): a call fills the columns [cout_off, cout_off + cout_n) of a Cout-wide packing, reading
 * segment i's channels at seg_offsets[i] of the weight's cin (NULL: the segments are the weight's channels in order and
 * must sum to cin), so several weight tensors can share one packing and a convolution can be split by input channel.
 * Padded channel lanes and columns are written as zeros, and the kernel stages zeros for them: nothing uninitialised is
 * ever multiplied. Once every column has been filled the packing is complete.
 *
 * Refused: N, h, w, a segment's channels or Cout below 1 (channels and Cout above 4096, N above 65535, more than 2^31 - 1
 * elements in a map); k not 1, 3, 5 or 7; nseg outside [1, 3]; segments that do not sum to cin, or lie outside it; columns
 * outside Cout; an unknown epilogue; unknown flags (a flag of a segment beyond nseg among them); OUT_NCHW with a gate
 * epilogue; an odd Cout with GATES; aux missing for a gate epilogue or given for another; an input beyond nseg; NULL; a
 * pointer not 16-byte aligned; a packing too small (EOGS_ERR_WORKSPACE).
 *
 * The same convolution over rectangular taps (1 x 5, 5 x 1) and RAFT-large's update block composed of it: eogs_flowrect_*
 * and eogs_flowlarge_* below. */

#define EOGS_FLOWNET_MAX_SEGMENTS 3
#define EOGS_FLOWNET_MAX_KERNEL 7
#define EOGS_FLOWNET_EPI_BIAS 0
#define EOGS_FLOWNET_EPI_RELU 1
#define EOGS_FLOWNET_EPI_GATES 2
#define EOGS_FLOWNET_EPI_GRU 3
#define EOGS_FLOWNET_IN0_NCHW 1u
#define EOGS_FLOWNET_OUT_NCHW 8u
#define EOGS_FLOWNET_UPDATE_PARAMS 18

/* The kernel's position tile, for tests and probes: a workgroup owns tile_w x tile_h positions of one image. */
int eogs_flownet_conv_info(int* tile_w, int* tile_h);
int eogs_flownet_conv_pack_bytes(int k, int nseg, const int* seg_channels, int cout, size_t* bytes);
int eogs_flownet_conv_pack(int k, int nseg, const int* seg_channels, const int* seg_offsets, int cin, int cout, int cout_off,
                           int cout_n, const float* weight, void* packed, size_t packed_bytes, void* stream);
int eogs_flownet_conv(int N, int h, int w, int k, int nseg, const int* seg_channels, const float* in0, const float* in1,
                      const float* in2, int cout, const void* packed, size_t packed_bytes, const float* bias, const float* add,
                      const float* aux, float* out, int epilogue, unsigned flags, void* stream);

/* RAFT-small's update block (hidden 96, context 64, correlation 196 = 4 levels at radius 3) over one workspace
 * (eogs_flownet_update_bytes: packed weights, biases, the hoisted planes, the hidden state and the intermediates;
 * rounded up to 256 bytes inside, as the pyramid's).
 *
 * begin: params are the 18 device pointers weight, bias of convcorr1, convflow1, convflow2, conv (motion encoder), convz,
 * convr, convq (GRU), conv1, conv2 (flow head) in torch's layouts; hidden f32[N][96][h][w] and context f32[N][64][h][w]
 * are the context encoder's halves after tanh / relu. It repacks every weight, copies the biases, stores the hidden state
 * channel-last, and forms the context's share of the three GRU convolutions, which does not change between updates and
 * is linear under zero padding: with W = [W_h | W_ctx | W_motion | W_flow] along the 242 input channels,
 *     plane_zr = conv3x3(context, [W_z; W_r]_ctx) + [b_z; b_r]   (192 channels),   plane_q = conv3x3(context, W_q,ctx) + b_q
 * step: corr f32[N][196][h][w] (the lookup's output) and flow f32[N][2][h][w] are read as they are; eight launches:
 *     c  = relu(conv1x1(corr) + b)            f1 = relu(conv7x7(flow) + b)       f2 = relu(conv3x3(f1) + b)
 *     m  = relu(conv3x3([c | f2]) + b)        z, r h = gates(conv3x3([h | m | flow], [W_z; W_r]) + plane_zr)
 *     h  = (1 - z) h + z tanh(conv3x3([r h | m | flow], W_q) + plane_q)          (in place in the workspace)
 *     d  = relu(conv3x3(h) + b)               delta f32[N][2][h][w] = conv3x3(d) + b
 * eogs_flownet_update_hidden_offset: the byte offset of h f32[N][h][w][96] from the workspace's 256-byte aligned base.
 * Refused: N, h or w below 1; N above 65535; more than 2^31 - 1 elements in a map; NULL (a NULL among params too); a
 * pointer not 16-byte aligned; a workspace too small (EOGS_ERR_WORKSPACE). */
int eogs_flownet_update_bytes(int N, int h, int w, size_t* bytes);
int eogs_flownet_update_hidden_offset(int N, int h, int w, size_t* offset);
int eogs_flownet_update_begin(int N, int h, int w, const float* const* params, const float* hidden, const float* context, void* ws,
                              size_t ws_bytes, void* stream);
int eogs_flownet_update_step(int N, int h, int w, const float* corr, const float* flow, void* ws, size_t ws_bytes, float* delta,
                             void* stream);

/* ---- The convolution over RECTANGULAR taps, and RAFT-large's update block and mask predictor composed of it. RAFT-large (the
 * reference's default flow network: flowmatching/flow_matching.py, model_name = "large") runs two ConvGRUs per update, one of
 * 1 x 5 and one of 5 x 1 taps, and predicts the mask of the convex upsampling from the hidden state. What is stated for the
 * eogs_flownet_* entries above (the convolution, the packing, the epilogues, the conventions) holds here word for word; what
 * follows is what differs. The entries carry prefixes of their own, eogs_flowrect_ and eogs_flowlarge_. ---- */

/* The three convolution entries of eogs_resample.h with (kh, kw) in place of k: kh x kw taps, stride 1, zero padding
 * ((kh - 1) / 2, (kw - 1) / 2), a cross-correlation as nn.Conv2d's; the weight is torch's f32[cout_n][cin][kh][kw]:
 *
 *   v[n][y][x][c] = ((sum over (i, ch, ky, kx) of in_i[n][y + ky - (kh - 1) / 2][x + kx - (kw - 1) / 2][ch] W[c][off_i + ch][ky][kx]) + bias[c])
 *                   + add[n][y][x][c]
 *
 * The order of the sum is the stated one: the segments in order, their channels in chunks of eight, per chunk the kh kw
 * taps in row-major order and per tap the chunk's channels ascending, one fused multiply-add per product. The tap shapes are
 * the four squares 1 x 1, 3 x 3, 5 x 5, 7 x 7 and 1 x 5 and 5 x 1. With kh == kw the three entries give the bits (a packing:
 * the bytes) of eogs_flownet_conv_pack_bytes, eogs_flownet_conv_pack and eogs_flownet_conv, and a packing made by either
 * serves the other. Epilogues, flags, the packing by column ranges and the segment offsets are those entries'. One
 * epilogue is added:
 *   EOGS_FLOWRECT_EPI_QUARTER  out = 0.25 v (an exact scaling by a power of two; a NaN stays a NaN): the mask predictor's
 *                             multiplier. No aux. Under EOGS_FLOWNET_OUT_NCHW with Cout = 576 it writes the f32[N][576][h][w]
 *                             that eogs_raft_upsample takes.
 *
 * Refused: N, h, w, a segment's channels or Cout below 1 (channels and Cout above 4096, N above 65535, more than 2^31 - 1
 * elements in a map); (kh, kw) not one of (1, 1), (3, 3), (5, 5), (7, 7), (1, 5), (5, 1); nseg outside [1, 3]; segments that
 * do not sum to cin, or lie outside it; columns outside Cout; an unknown epilogue; unknown flags (a flag of a segment beyond
 * nseg among them); OUT_NCHW with a gate epilogue; an odd Cout with GATES; aux missing for a gate epilogue or given for
 * another (QUARTER among them); an input beyond nseg; NULL; a pointer not 16-byte aligned; a packing too small
 * (EOGS_ERR_WORKSPACE). */

#define EOGS_FLOWRECT_EPI_QUARTER 4
#define EOGS_FLOWLARGE_PARAMS 30

int eogs_flowrect_pack_bytes(int kh, int kw, int nseg, const int* seg_channels, int cout, size_t* bytes);
int eogs_flowrect_pack(int kh, int kw, int nseg, const int* seg_channels, const int* seg_offsets, int cin, int cout,
                                int cout_off, int cout_n, const float* weight, void* packed, size_t packed_bytes, void* stream);
int eogs_flowrect_conv(int N, int h, int w, int kh, int kw, int nseg, const int* seg_channels, const float* in0, const float* in1,
                           const float* in2, int cout, const void* packed, size_t packed_bytes, const float* bias, const float* add,
                           const float* aux, float* out, int epilogue, unsigned flags, void* stream);

/* RAFT-large's update block (hidden 128, context 128, correlation 324 = 4 levels at radius 4) and its mask predictor over
 * one workspace (eogs_flowlarge_bytes: packed weights, biases, the four hoisted planes, the hidden state and the
 * intermediates; rounded up to 256 bytes inside).
 *
 * begin: params are the 30 device pointers weight, bias of convcorr1, convcorr2, convflow1, convflow2, conv (motion encoder),
 * convgru1.convz, .convr, .convq (1 x 5), convgru2.convz, .convr, .convq (5 x 1), conv1, conv2 (flow head), then the mask
 * predictor's convrelu.0 and conv, in torch's layouts; hidden f32[N][128][h][w] and context f32[N][128][h][w] are the
 * context encoder's halves after tanh / relu. It repacks every weight, copies the biases, stores the hidden state
 * channel-last, and forms the context's share of the six GRU convolutions, which does not change between updates and is
 * linear under zero padding: with W = [W_h | W_ctx | W_motion | W_flow] along the 384 input channels, per GRU g
 *     plane_zr_g = conv_g(context, [W_z; W_r]_ctx) + [b_z; b_r]   (256 channels),   plane_q_g = conv_g(context, W_q,ctx) + b_q   (128)
 * with conv_1 over 1 x 5 taps and conv_2 over 5 x 1: 768 channels in all.
 * step: corr f32[N][324][h][w] (the lookup's output) and flow f32[N][2][h][w] are read as they are; eleven launches:
 *     c1 = relu(conv1x1(corr) + b)  (256)       c2 = relu(conv3x3(c1) + b)  (192)
 *     f1 = relu(conv7x7(flow) + b)  (128)       f2 = relu(conv3x3(f1) + b)  (64)
 *     m  = relu(conv3x3([c2 | f2]) + b)  (126)
 *     z, r h = gates(conv1x5([h | m | flow], [W_z; W_r]) + plane_zr_1)
 *     h  = (1 - z) h + z tanh(conv1x5([r h | m | flow], W_q) + plane_q_1)          (in place in the workspace)
 *     the same two with convgru2's 5 x 1 weights and planes
 *     d  = relu(conv3x3(h) + b)  (256)          delta f32[N][2][h][w] = conv3x3(d) + b
 * mask: reads the hidden state the workspace holds now (after begin, or after the last step); two launches:
 *     mask f32[N][576][h][w] = 0.25 (conv1x1(relu(conv3x3(h) + b)) + b)
 * It leaves the hidden state as it is; a step may follow it.
 * eogs_flowlarge_hidden_offset: the byte offset of h f32[N][h][w][128] from the workspace's 256-byte aligned base.
 * Refused: N, h or w below 1; N above 65535; more than 2^31 - 1 elements in a map (the mask's 576 channels count); NULL (a
 * NULL among params too); a pointer not 16-byte aligned; a workspace too small (EOGS_ERR_WORKSPACE). */
int eogs_flowlarge_bytes(int N, int h, int w, size_t* bytes);
int eogs_flowlarge_hidden_offset(int N, int h, int w, size_t* offset);
int eogs_flowlarge_begin(int N, int h, int w, const float* const* params, const float* hidden, const float* context,
                                    void* ws, size_t ws_bytes, void* stream);
int eogs_flowlarge_step(int N, int h, int w, const float* corr, const float* flow, void* ws, size_t ws_bytes, float* delta,
                                   void* stream);
int eogs_flowlarge_mask(int N, int h, int w, void* ws, size_t ws_bytes, float* mask, void* stream);

/* ---- RAFT-small's two encoders (bottleneck blocks of 8, 16 and 24 mid channels behind a 7 x 7 stride-2 stem, a 1 x 1 head;
 * the feature encoder with an instance norm and a ReLU after every convolution, the context encoder with the ReLU alone):
 * the convolution above with a stride, the producer's norm applied on load, the block's residual tail and the map's
 * statistics; the kernel that makes (mean, rstd) of them; the pointwise pass that closes a normalised block; and each
 * encoder as one call. Float32, forward only, RAFT-small only. Every convention above holds: no allocation, no waiting,
 * every argument checked before anything touches a device, the stream last, device pointers 16-byte aligned, no atomics,
 * a fixed order of every sum (bitwise reproducible; a batch gives the bits of its single images). params is a HOST array.
 *
 * eogs_flowenc_conv: one input map of cin channels, k in {1, 3, 7}, stride s in {1, 2}, zero padding p = (k - 1) / 2, output
 * h' x w' = ceil(h / s) x ceil(w / s); a cross-correlation as nn.Conv2d's:
 *
 *   sum[n][y][x][c] = sum over (ch, ky, kx) of X[n][s y + ky - p][s x + kx - p][ch] W[c][ch][ky][kx]
 *
 * in eogs_flownet_conv's order: the channels in chunks of eight, per chunk the taps in row-major order, per tap the chunk's
 * channels ascending, one fused multiply-add per product. The weights are packed by eogs_flownet_conv_pack with nseg = 1
 * (eogs_flownet_conv_pack_bytes). The input is in f32[N][h][w][cin], or f32[N][cin][h][w] under EOGS_FLOWENC_IN_NCHW (the
 * image of the 7 x 7 stem). With in_norm f32[N][cin][2] = (mean, rstd) per image and channel, the value multiplied is
 *   X = max((in - mean) * rstd, 0)
 * as two separately rounded float32 operations and a select that keeps a NaN: the producer's instance norm and ReLU,
 * applied on load (positions outside the map stay zeros: the padding is the normalised map's). Without in_norm, X = in.
 * Epilogues, with v = sum + bias[c] (bias may be NULL: v = sum):
 *   EOGS_FLOWENC_EPI_BIAS      out = v
 *   EOGS_FLOWENC_EPI_RELU      out = v < 0 ? 0 : v (a NaN stays a NaN)
 *   EOGS_FLOWENC_EPI_RESIDUAL  out = relu(res + relu(v)), res f32[N][h'][w'][cout]: a bottleneck's tail where there is no norm
 * out is f32[N][h'][w'][cout], or f32[N][cout][h'][w'] under EOGS_FLOWENC_OUT_NCHW (BIAS only: the heads).
 * With partials given (BIAS only; eogs_flowenc_conv_partials gives rows and bytes: f64[N][rows][cout][2], one row per
 * workgroup's 16 x 8 tile of output positions), each workgroup also stores per output channel the double-precision sum and
 * sum of squares of the float32 values it stored, over its valid positions: per lane its rows ascending and per row its four
 * positions ascending, the four lanes of a channel by the butterfly (offsets 32, 16), the four waves left to right.
 * Refused: N, h, w, cin or cout below 1 (cin and cout above 4096, N above 65535, more than 2^31 - 1 elements in the input
 * or the output map); k not 1, 3 or 7; a stride not 1 or 2; an unknown epilogue; unknown flags; OUT_NCHW or partials with an
 * epilogue other than BIAS; res missing for RESIDUAL or given for another; NULL in, packed or out; a pointer not 16-byte
 * aligned; a packing or partials too small (EOGS_ERR_WORKSPACE).
 *
 * eogs_flowenc_norm: stage 2 of the two-stage sum over the partials of an h x w map of C channels (h, w: the
 * convolution's OUTPUT size): one workgroup of 256 threads per (channel, image), thread t adds rows t, t + 256, ... in that
 * order, then the butterfly and the four waves left to right. In double, with n = h w:
 *   mean = S1 / n,   var = max(S2 / n - mean^2, 0) (biased; a NaN stays a NaN),   rstd = 1 / sqrt(var + 1e-5)
 * mean and rstd are rounded to float32 once each and written to norm f32[N][C][2]. One launch.
 * Refused: N, h, w or C below 1 (C above 4096, N above 65535, 2^31 - 1 elements); NULL; a pointer not 16-byte aligned;
 * partials too small (EOGS_ERR_WORKSPACE).
 *
 * eogs_flowenc_finish: one pointwise pass over f32[N][h][w][C], C a multiple of 4:
 *   out = relu(S + relu((v - mean_v) * rstd_v))        (each a separately rounded float32 operation; a NaN stays a NaN)
 *   EOGS_FLOWENC_SHORTCUT_NONE   S = 0: out = relu((v - mean_v) * rstd_v), the stem's output; s and norm_s NULL
 *   EOGS_FLOWENC_SHORTCUT_PLAIN  S = s; norm_s NULL
 *   EOGS_FLOWENC_SHORTCUT_NORM   S = (s - mean_s) * rstd_s: the normalised 1 x 1 stride-2 downsample, no ReLU
 * Refused: sizes as above; C no multiple of 4; an unknown shortcut; s or norm_s that does not fit the shortcut; NULL v,
 * norm_v or out; a pointer not 16-byte aligned.
 *
 * eogs_flowenc_run: a whole encoder. kind EOGS_FLOWENC_FEATURE (widths 32, 32, 64, 96 -> 128, an instance norm after
 * every convolution but the head) or EOGS_FLOWENC_CONTEXT (the same -> 160, no norm). params: the 44 device pointers
 * weight, bias of the 22 convolutions in module order: convnormrelu; per block of layer1.0, layer1.1, layer2.0, layer2.1,
 * layer3.0, layer3.1 its convnormrelu1, 2, 3 and, where it has one (layer2.0, layer3.0), its downsample; conv. image
 * f32[N][3][H][W]; out f32[N][128 or 160][h3][w3] (NCHW) with h1 = ceil(H / 2), h2 = ceil(h1 / 2), h3 = ceil(h2 / 2). The
 * weights are repacked at every call. A unit is conv -> statistics -> (v - mean) rstd -> ReLU, a block relu(S + y):
 *   FEATURE  stem: conv, norm, finish(NONE). Block: conv1 (statistics), norm; conv2 normalising conv1's output on load,
 *            norm; conv3 normalising conv2's on load, norm; with a downsample its conv and norm; finish(PLAIN with the
 *            block's input, or NORM with the downsample's output). Head: conv (BIAS, OUT_NCHW).
 *   CONTEXT  stem RELU. Block: conv1 RELU, conv2 RELU, the downsample (BIAS) where there is one, conv3 RESIDUAL with the
 *            block's input or the downsample's output as res. Head as above. No pointwise pass.
 * The workspace (eogs_flowenc_bytes; rounded up to 256 bytes inside) holds the packed weights, the maps, the partials and
 * the norm tables; a call relies on nothing in it that it did not write.
 * Refused: an unknown kind; N, H or W below 1; N above 65535; more than 2^31 - 1 elements in a map; for FEATURE a final
 * map of a single position (h3 w3 = 1: torch's instance norm raises there); NULL (a NULL among params too); a pointer not
 * 16-byte aligned; a workspace too small (EOGS_ERR_WORKSPACE). */

#define EOGS_FLOWENC_EPI_BIAS 0
#define EOGS_FLOWENC_EPI_RELU 1
#define EOGS_FLOWENC_EPI_RESIDUAL 2
#define EOGS_FLOWENC_IN_NCHW 1u
#define EOGS_FLOWENC_OUT_NCHW 8u
#define EOGS_FLOWENC_SHORTCUT_NONE 0
#define EOGS_FLOWENC_SHORTCUT_PLAIN 1
#define EOGS_FLOWENC_SHORTCUT_NORM 2
#define EOGS_FLOWENC_FEATURE 0
#define EOGS_FLOWENC_CONTEXT 1
#define EOGS_FLOWENC_PARAMS 44

int eogs_flowenc_conv_partials(int N, int h, int w, int cout, int* rows, size_t* bytes);
int eogs_flowenc_conv(int N, int h, int w, int cin, int cout, int k, int stride, const float* in, const float* in_norm,
                      const void* packed, size_t packed_bytes, const float* bias, const float* res, float* out, double* partials,
                      size_t partials_bytes, int epilogue, unsigned flags, void* stream);
int eogs_flowenc_norm(int N, int h, int w, int C, const double* partials, size_t partials_bytes, float* norm, void* stream);
int eogs_flowenc_finish(int N, int h, int w, int C, const float* v, const float* norm_v, const float* s, const float* norm_s,
                        int shortcut, float* out, void* stream);
int eogs_flowenc_bytes(int N, int H, int W, int kind, size_t* bytes);
int eogs_flowenc_run(int N, int H, int W, int kind, const float* const* params, const float* image, void* ws, size_t ws_bytes,
                     float* out, void* stream);

/* ---- RAFT-large's two encoders (residual blocks of two 3 x 3 convolutions at widths 64, 64, 96, 128 behind a 7 x 7 stride-2
 * stem, a 1 x 1 head of 256 channels; the feature encoder with an instance norm after every convolution but the head, the
 * context encoder with a batch norm in eval mode there): eogs_flowenc_conv, eogs_flowenc_norm and eogs_flowenc_finish above,
 * a kernel that folds an eval-mode batch norm into its convolution, and each encoder as one call. Float32, forward only.
 * Every convention above holds. params and bn are HOST arrays of device pointers.
 *
 * eogs_flowres_fold: a batch norm in eval mode folded into its convolution, one kernel, per output channel c over
 * per_out = Cin k k weights:
 *   s[c] = float(gamma[c] / sqrt(double(var[c]) + eps)), computed in double and rounded once
 *   w'[c, .] = w[c, .] * s[c], one float32 product per weight
 *   b'[c] = float((double(b[c]) - double(mean[c])) * double(s[c]) + double(beta[c])), where s[c] is the rounded float32 above
 * w and w_out f32[cout][per_out]; b, gamma, beta, mean, var and b_out f32[cout]. Nothing is read back on the host: a NaN
 * stays a NaN, a negative var is not refused and gives NaN (in its channel alone).
 * Refused: cout or per_out below 1 (cout above 4096, more than 2^31 - 1 weights); a NULL pointer; a pointer not 16-byte
 * aligned.
 *
 * eogs_flowres_run: a whole encoder. kind EOGS_FLOWENC_FEATURE (bn must be NULL) or EOGS_FLOWENC_CONTEXT (bn required).
 * params: the 32 device pointers weight, bias of the 16 convolutions in module order: convnormrelu; per block of layer1.0,
 * layer1.1, layer2.0, layer2.1, layer3.0, layer3.1 its convnormrelu1 (3 x 3, stride 2 in layer2.0 and layer3.0),
 * convnormrelu2 (3 x 3) and, where it has one (layer2.0, layer3.0), its downsample (1 x 1, stride 2); conv. bn: the 60 device
 * pointers gamma, beta, running mean, running var of the 15 convolutions that have a norm, in the same order. image
 * f32[N][3][H][W]; out f32[N][256][h3][w3] (NCHW) with h1 = ceil(H / 2), h2 = ceil(h1 / 2), h3 = ceil(h2 / 2). The packings
 * (and the folds) are rebuilt at every call.
 *   FEATURE  stem: conv (statistics), norm, finish(NONE). Block: conv1(x) -> r1 and its table; conv2 normalising r1 on load
 *            -> r2 and its table; with a downsample down(x) -> rd and its table; y = finish(r2, table, S) with S = x (PLAIN)
 *            or rd with its table (NORM): relu(S + relu(norm(r2))), the block's forward. Head: conv (BIAS, OUT_NCHW).
 *            16 convolutions, 15 norms, 7 pointwise passes.
 *   CONTEXT  every convolution with a norm is folded by eogs_flowres_fold's kernel with eps 1e-5 into the workspace first.
 *            Stem RELU. Block: conv1 RELU, the downsample (BIAS) where there is one, conv2 RESIDUAL with the block's input
 *            or the downsample's output as res. Head as above. 16 convolutions and 15 folds, no pointwise pass.
 * The workspace (eogs_flowres_bytes; rounded up to 256 bytes inside) holds the packed weights, for CONTEXT the folded ones,
 * a block's maps at the stem's resolution, the partials and the norm tables; a call relies on nothing in it that it did not
 * write.
 * Refused: an unknown kind; N, H or W below 1; N above 65535; more than 2^31 - 1 elements in a map; for FEATURE a final
 * map of a single position; bn given under FEATURE or missing under CONTEXT; NULL (a NULL among params or bn too); a
 * pointer not 16-byte aligned; a workspace too small (EOGS_ERR_WORKSPACE). */

#define EOGS_FLOWRES_PARAMS 32
#define EOGS_FLOWRES_BN 60

int eogs_flowres_fold(int cout, int per_out, const float* w, const float* b, const float* gamma, const float* beta, const float* mean,
                      const float* var, double eps, float* w_out, float* b_out, void* stream);
int eogs_flowres_bytes(int N, int H, int W, int kind, size_t* bytes);
int eogs_flowres_run(int N, int H, int W, int kind, const float* const* params, const float* const* bn, const float* image, void* ws,
                     size_t ws_bytes, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EOGS_RESAMPLE_H_INCLUDED */
