// bucket_gather.h — the fixed-order bucketed gather that turns a four-tap bilinear scatter into plain stores; shared by the
// backward of the virtual-camera resample (resample.hip) and of the flow warp (flow.hip). A `Src` names where an output pixel
// samples:
//   Raw  load(size_t pix, int x, int y) const     what the pixel reads from memory (issued for a whole chunk before any use)
//   void taps(const Raw&, int Wv, int Hv, int& x0, int& y0, float& wx1, float& wy1, bool& outside) const
//                                                   north-west tap cell, weights of the east / south taps, "fill" flag
//   bool bypass() const                             true: the sampler is switched off (dL/dvirtual = dL/dsample; same-size grids)
#pragma once
#include "common.h"

namespace {

constexpr int OT = 16;  // output tile edge (256 pixels = one workgroup)

// ---- tile kernel, second form (round 4): bucketed gather, no float atomics ----
// The first form spends its time in ds_add_f32: four taps x n_out channels per output pixel, ~2 LDS cycles per lane each
// (profiles/r04 resample probes: 72-107 us per backward at 1024^2). Here a pixel that lands in the tile costs two INTEGER LDS
// atomics: the workgroup takes its candidate output tiles CHT at a time (four, or eight with one channel),
//   count : every pixel whose north-west tap cell (x0, y0) lies in [vx0-1, vx0+VTX) x [vy0-1, vy0+VTY) — the cells whose taps can
//           reach the tile — adds one to the counter of that cell's BUCKET;
//   scan  : exclusive prefix of the (VTX+1) x (VTY+1) counters;
//   fill  : the same pixels again, each takes the next place of its bucket and parks {wx1, wy1, g[0..3]} there;
//   gather: every virtual cell (cx, cy) of the tile — a few per thread, accumulators in registers — adds the entries of its four
//           buckets (x0, y0) in {cx-1, cx} x {cy-1, cy} with the tap weight that cell has in them,
// and writes its cells once with plain stores. Every tap of every pixel is counted exactly once, by the tile that owns its
// cell; taps outside the virtual image have no cell. The sums run in a FIXED order (bit-reproducible, unlike the first form and
// unlike grid_sample's backward in the reference): the candidate tiles are listed in tile order (ballot ranks, not an atomic
// cursor), and inside a bucket — whose places the integer atomics hand out in any order — every entry ranks itself among the
// bucket's pixel ids before it parks its payload, so a bucket's entries lie in pixel order.
// (registers: held to the occupancy each variant had before the fixed-order fill — the compiler otherwise keeps a few more
// values live across the two new barriers and drops a wave per SIMD, +50 % on the one-channel kernel)
template <int NACC, int VX, int VY, class Src>
__global__ __launch_bounds__(BLK) __attribute__((amdgpu_waves_per_eu((NACC == 4 && VX == 32) ? 4 : 3)))
void resample_bwd_gather_kernel(int C, int Hv, int Wv, int H, int W, int n_out, const Src src,
                                                                  int fill_channel, const float* __restrict__ gs,
                                                                  const int4* __restrict__ bbox, int ntx, int nty,
                                                                  float* __restrict__ gvr) {
  constexpr int BXN = VX + 1, BYN = VY + 1, NB = BXN * BYN;  // buckets: north-west cells x0 = vx0-1 .. vx0+VX-1
  constexpr int CHT = NACC == 1 ? 8 : 4;                       // candidate output tiles per chunk
  // boxes per scan round, each thread's loads independent. One channel: the whole 1024^2 grid in one round (38.9 us against
  // 46.5 with rounds of 1024 at 2048^2); four channels: rounds of 1024 — the parked entries already take 24 KB of LDS and the
  // larger candidate list costs the fourth resident workgroup (70.9 -> 78.2 us, 31.8 -> 39.1 at 1024^2)
  constexpr int RB = NACC == 1 ? 4096 : 1024;
  constexpr int CAP = CHT * OT * OT;                           // entries a chunk can park
  constexpr int PAY = 2 + NACC;                                // floats per entry: wx1, wy1, g[NACC]
  constexpr int CPT = VX * VY / BLK;                           // cells per thread
  static_assert(VX * VY % BLK == 0 && BLK == OT * OT, "cells dealt evenly; one thread per pixel of an output tile");
  __shared__ uint32_t s_cnt[NB + 1];
  __shared__ uint32_t s_start[NB + 1];
  __shared__ float s_pay[CAP * PAY];
  __shared__ uint16_t s_list[RB];  // candidates of the round, as offsets into it
  __shared__ uint32_t s_n;
  __shared__ uint32_t s_wsum[BLK / 64];
  __shared__ uint32_t s_wc[64];  // candidates per (scan step, wave), then their exclusive prefix
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int vx0 = blockIdx.x * VX, vy0 = blockIdx.y * VY;
  const int HW = H * W;
  const bool bypass = src.bypass();
  const int nt = bypass ? 0 : ntx * nty;
  float acc[CPT][NACC];
#pragma unroll
  for (int c = 0; c < CPT; c++)
#pragma unroll
    for (int ch = 0; ch < NACC; ch++) acc[c][ch] = 0.f;
  for (int e = t; e <= NB; e += BLK) s_cnt[e] = 0u;

  for (int scanned = 0; scanned < nt; scanned += RB) {  // candidate output tiles: RB boxes per round (1024^2: one round, or four)
    {
      constexpr int RBN = RB / BLK, NW = BLK / 64;
      static_assert(RBN * NW <= 64, "the per-wave candidate counts are scanned by one wave");
      int4 bb[RBN];
#pragma unroll
      for (int i = 0; i < RBN; i++) {
        const int k = scanned + i * BLK + t;
        bb[i] = k < nt ? bbox[k] : make_int4(1, 1, 0, 0);  // (empty box: x0 > x1)
      }
      // the candidates in tile order: per (i, wave) ballot counts, their exclusive scan, ballot ranks
      uint32_t pred = 0;
#pragma unroll
      for (int i = 0; i < RBN; i++) {
        const bool c = bb[i].x <= bb[i].z && bb[i].x <= vx0 + VX - 1 && bb[i].z >= vx0 && bb[i].y <= vy0 + VY - 1 && bb[i].w >= vy0;
        pred |= (c ? 1u : 0u) << i;
        const unsigned long long m = __ballot(c);
        if (lane == 0) s_wc[i * NW + wv] = (uint32_t)__popcll(m);
      }
      __syncthreads();
      if (t < 64) {
        const uint32_t v = t < RBN * NW ? s_wc[t] : 0u;
        uint32_t inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const uint32_t nb2 = __shfl_up(inc, o, 64);
          if (lane >= o) inc += nb2;
        }
        if (t < RBN * NW) s_wc[t] = inc - v;
        if (t == 63) s_n = inc;
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < RBN; i++) {
        const bool c = (pred >> i) & 1u;
        const unsigned long long m = __ballot(c);
        if (c) s_list[s_wc[i * NW + wv] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)(i * BLK + t);
      }
    }
    __syncthreads();
    const uint32_t n = s_n;
    for (uint32_t k0 = 0; k0 < n; k0 += CHT) {
      const uint32_t kn = min(n - k0, (uint32_t)CHT);
      // This thread's pixel of each of the chunk's candidate tiles. The loads of all CHT pixels are issued before anything
      // waits for one of them (the first version walked the candidates one by one and spent its time in four dependent
      // round trips per pass: 98 us per backward at 2048^2 against 113 for the atomics it had been written to avoid).
      size_t pix[CHT];
      typename Src::Raw raw[CHT];
      bool in_img[CHT];
#pragma unroll
      for (int k = 0; k < CHT; k++) {
        const int tile = (uint32_t)k < kn ? scanned + (int)s_list[k0 + k] : 0;
        const int x = (tile % ntx) * OT + (t & (OT - 1)), y = (tile / ntx) * OT + (t >> 4);
        in_img[k] = (uint32_t)k < kn && x < W && y < H;
        pix[k] = in_img[k] ? (size_t)y * W + x : 0;
        raw[k] = src.load(pix[k], in_img[k] ? x : 0, in_img[k] ? y : 0);
      }
      int bucket[CHT];
      float wx1[CHT], wy1[CHT];
      bool outside[CHT];
      // count
#pragma unroll
      for (int k = 0; k < CHT; k++) {
        int tx0, ty0;
        src.taps(raw[k], Wv, Hv, tx0, ty0, wx1[k], wy1[k], outside[k]);
        const int lx = tx0 - vx0, ly = ty0 - vy0;
        const bool lands = in_img[k] && lx >= -1 && lx < VX && ly >= -1 && ly < VY;
        bucket[k] = lands ? (ly + 1) * BXN + (lx + 1) : -1;
        if (lands) atomicAdd(&s_cnt[bucket[k]], 1u);
      }
      // the gradients the fill pass parks: requested now, used after the scan
      float gq[CHT][NACC];
#pragma unroll
      for (int k = 0; k < CHT; k++)
#pragma unroll
        for (int ch = 0; ch < NACC; ch++) {
          float g = (bucket[k] >= 0 && ch < n_out) ? gs[(size_t)ch * HW + pix[k]] : 0.f;
          if (ch == fill_channel && outside[k]) g = 0.f;  // the value was overwritten by a constant
          gq[k][ch] = g;
        }
      __syncthreads();
      // exclusive scan of the NB counters: thread t owns a contiguous run, waves chained through s_wsum
      {
        constexpr int PER = (NB + BLK - 1) / BLK;
        uint32_t loc[PER], sum = 0;
#pragma unroll
        for (int i = 0; i < PER; i++) {
          const int e = t * PER + i;
          loc[i] = e < NB ? s_cnt[e] : 0u;
          sum += loc[i];
        }
        uint32_t inc = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const uint32_t nb2 = __shfl_up(inc, o, 64);
          if (lane >= o) inc += nb2;
        }
        if (lane == 63) s_wsum[wv] = inc;
        __syncthreads();
        uint32_t pre = inc - sum;
#pragma unroll
        for (int k = 0; k < BLK / 64; k++)
          if (k < wv) pre += s_wsum[k];
#pragma unroll
        for (int i = 0; i < PER; i++) {
          const int e = t * PER + i;
          if (e < NB) { s_start[e] = pre; s_cnt[e] = 0u; }
          pre += loc[i];
        }
      }
      __syncthreads();
      // fill, in pixel order inside every bucket: the atomics hand out the bucket's places to the pixel IDS (candidate k of the
      // chunk, thread t), each pixel then counts the smaller ids of its bucket (a bucket holds a few entries; one alone skips
      // the loop) and parks its payload at that rank
      uint32_t* s_id = reinterpret_cast<uint32_t*>(s_pay);
#pragma unroll
      for (int k = 0; k < CHT; k++)
        if (bucket[k] >= 0) s_id[(s_start[bucket[k]] + atomicAdd(&s_cnt[bucket[k]], 1u)) * PAY] = (uint32_t)(k * BLK + t);
      __syncthreads();
      uint32_t pos[CHT];
#pragma unroll
      for (int k = 0; k < CHT; k++) {
        pos[k] = 0u;
        if (bucket[k] >= 0) {
          const uint32_t st = s_start[bucket[k]], cnt = s_cnt[bucket[k]], me = (uint32_t)(k * BLK + t);
          uint32_t r = 0u;
          if (cnt > 1u)
            for (uint32_t e = st; e < st + cnt; e++) r += s_id[e * PAY] < me ? 1u : 0u;
          pos[k] = st + r;
        }
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < CHT; k++) {
        if (bucket[k] >= 0) {
          float* e = s_pay + pos[k] * PAY;
          e[0] = wx1[k]; e[1] = wy1[k];
#pragma unroll
          for (int ch = 0; ch < NACC; ch++) e[2 + ch] = gq[k][ch];
        }
      }
      __syncthreads();
      // gather: cell (lx, ly) <- buckets (lx + dx, ly + dy), dx, dy in {0, 1}: bucket column lx holds x0 = cell - 1 (the cell is
      // the EAST tap: weight wx1), column lx + 1 holds x0 = cell (WEST tap: 1 - wx1); rows likewise
#pragma unroll
      for (int c = 0; c < CPT; c++) {
        const int cell = c * BLK + t, lx = cell % VX, ly = cell / VX;
#pragma unroll
        for (int dy = 0; dy < 2; dy++)
#pragma unroll
          for (int dx = 0; dx < 2; dx++) {
            const int bk = (ly + dy) * BXN + lx + dx;
            const uint32_t cnt = s_cnt[bk];
            if (cnt == 0u) continue;
            const uint32_t st = s_start[bk];
            for (uint32_t e = st; e < st + cnt; e++) {
              const float* q = s_pay + e * PAY;
              const float wx = dx ? 1.f - q[0] : q[0], wy = dy ? 1.f - q[1] : q[1];
              const float wgt = wx * wy;
#pragma unroll
              for (int ch = 0; ch < NACC; ch++) acc[c][ch] += q[2 + ch] * wgt;
            }
          }
      }
      __syncthreads();
      for (int e = t; e <= NB; e += BLK) s_cnt[e] = 0u;  // (ordered against the next count pass by the barrier that follows)
      __syncthreads();
    }
  }
  // every virtual pixel of the tile, every channel (channels >= n_out get zeros): plain coalesced stores
  const size_t plane = (size_t)Hv * Wv;
#pragma unroll
  for (int c = 0; c < CPT; c++) {
    const int cell = c * BLK + t, lx = cell % VX, ly = cell / VX;
    const int gx = vx0 + lx, gy = vy0 + ly;
    if (gx < Wv && gy < Hv) {
      for (int ch = 0; ch < C; ch++) {
        float v = 0.f;
#pragma unroll
        for (int a = 0; a < NACC; a++)
          if (a == ch && ch < n_out) v = acc[c][a];
        if (bypass && ch < n_out) v = gs[(size_t)ch * HW + (size_t)gy * W + gx];
        gvr[ch * plane + (size_t)gy * Wv + gx] = v;
      }
    }
  }
}

}  // namespace
