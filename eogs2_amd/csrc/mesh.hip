// mesh.hip — marching cubes over a TSDF volume (include/eogs_mesh.h): what the reference does with the third-party mcubes
// on a host copy of the volume (tsdf.py:522-528); the semantics are stated in the header, the case table is generated
// (mesh_table.h, tools/gen_mesh_table.py).
//
// One voxel per lane, lanes consecutive in z, 256 voxels per workgroup, the same grid in every pass:
//   count     owned-edge flags + the cell's triangle count -> one packed total per workgroup (plain stores)
//   scan      two levels in a fixed order: every chunk of 256 totals by a workgroup of its own, then the chunks by ONE
//             workgroup in rounds of 256 with a carry -> the exclusive vertex / triangle base per workgroup
//   vertex    ballot / popcount ranks inside the workgroup + its base: the interpolated vertices and, for every voxel
//             that owns one, the word `first vertex | flags << 29`
//   triangle  per cell: each table edge -> its owner's word -> the vertex index
// voxel_steps(), owned_edges() and cell_case() serve every pass that needs them, so the passes see the same edges and cases by
// construction. No atomics anywhere: the same bits on every run.
#include <float.h>
#include <math.h>

#include "api_util.h"
#include "eogs_mesh.h"
#include "mesh_table.h"
#include "reduce.h"

namespace {

constexpr int MT = EOGS_MESH_WG_VOXELS;
constexpr int MR = EOGS_MESH_SCAN_ROUND;
static_assert(MT == 256 && MR == 256, "four waves per workgroup: the s_w[4] exchanges below");
constexpr uint32_t MESH_BASE_MASK = EOGS_MESH_MAX_VERTICES - 1u;
// a workgroup's totals in one word: vertices <= 3 * 256 (10 bits), triangles <= 5 * 256 (11 bits), non-finite <= 256
constexpr int PACK_T = 10, PACK_F = 21;

const int8_t h_table[256][16] = EOGS_MESH_TABLE_ROWS;
__constant__ int8_t d_table[256][16] = EOGS_MESH_TABLE_ROWS;

struct MeshDims { int nx, ny, nz, n; };  // n = nx ny nz < 2^31
struct MeshShift { int on; double s[3]; };

__device__ inline bool inside(float v, double iso) { return (double)v < iso; }

__device__ inline void voxel_xyz(const MeshDims& d, int v, int& x, int& y, int& z) {
  z = v % d.nz;
  const int r = v / d.nz;
  y = r % d.ny;
  x = r / d.ny;
}

// Offsets to the +x, +y, +z neighbours of voxel (x, y, z), 0 where the volume ends: every read stays inside the volume and
// none depends on another, so a lane's loads are in flight together.
struct MeshStep { int sx, sy, sz; };
__device__ inline MeshStep voxel_steps(const MeshDims& d, int x, int y, int z) {
  return MeshStep{x + 1 < d.nx ? d.ny * d.nz : 0, y + 1 < d.ny ? d.nz : 0, z + 1 < d.nz ? 1 : 0};
}

// bit a: the edge from voxel v along axis a (x, y, z) crosses the surface: va and the three neighbours' values (a
// neighbour past the end is the voxel itself and never differs). A volume without a cell has no mesh.
__device__ inline uint32_t owned_edges(const MeshDims& d, double iso, float va, float vx, float vy, float vz) {
  if (d.nx < 2 || d.ny < 2 || d.nz < 2) return 0u;
  const bool in = inside(va, iso);
  return (inside(vx, iso) != in ? 1u : 0u) | (inside(vy, iso) != in ? 2u : 0u) | (inside(vz, iso) != in ? 4u : 0u);
}

// the eight corners of the cell whose lowest corner is voxel v, corner b = dx + 2 dy + 4 dz
__device__ inline void load_corners(const float* __restrict__ vol, int v, const MeshStep& st, float c[8]) {
#pragma unroll
  for (int b = 0; b < 8; b++) c[b] = vol[v + (b & 1) * st.sx + ((b >> 1) & 1) * st.sy + (b >> 2) * st.sz];
}

// the case of that cell (bit b: corner b is inside); 0 where there is no cell
__device__ inline int cell_case(const MeshStep& st, double iso, const float c[8]) {
  if (!(st.sx && st.sy && st.sz)) return 0;
  int k = 0;
#pragma unroll
  for (int b = 0; b < 8; b++)
    if (inside(c[b], iso)) k |= 1 << b;
  return k;
}

__global__ __launch_bounds__(MT) void mesh_count_kernel(MeshDims d, const float* __restrict__ vol, double iso,
                                                        uint32_t* __restrict__ totals) {
  __shared__ int s_red[4];
  const int v = (int)(blockIdx.x * (unsigned)MT + threadIdx.x);
  int packed = 0;
  if (v < d.n) {
    int x, y, z;
    voxel_xyz(d, v, x, y, z);
    const MeshStep st = voxel_steps(d, x, y, z);
    float c[8];
    load_corners(vol, v, st, c);
    const int nonfinite = fabsf(c[0]) <= FLT_MAX ? 0 : 1;  // NaN and +-inf
    packed = __popc(owned_edges(d, iso, c[0], c[1], c[2], c[4])) | ((int)d_table[cell_case(st, iso, c)][15] << PACK_T) |
             (nonfinite << PACK_F);
  }
  packed = wg_sum(packed, s_red);  // the fields cannot carry into each other
  if (threadIdx.x == 0) totals[blockIdx.x] = (uint32_t)packed;
}

__device__ inline uint32_t saturate32(unsigned long long v) { return v > 0xffffffffull ? 0xffffffffu : (uint32_t)v; }

// The exclusive scan of three counters over a workgroup of four waves, in a fixed order: lanes by a shuffle scan, waves
// 0..3 left to right through s_w. Returns the thread's exclusive vertex and triangle offsets and the workgroup's totals.
struct MeshScan { uint32_t ev, et, tv, tt, tf; };
__device__ inline MeshScan wg_scan3(uint32_t nv, uint32_t nt, uint32_t nf, uint32_t (*s_w)[4]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t iv = nv, it = nt;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t a = __shfl_up(iv, o, 64), b = __shfl_up(it, o, 64);
    if (lane >= o) {
      iv += a;
      it += b;
    }
  }
  const uint32_t f = (uint32_t)wave_sum((int)nf);
  if (lane == 63) {
    s_w[0][w] = iv;
    s_w[1][w] = it;
    s_w[2][w] = f;
  }
  __syncthreads();
  MeshScan r{iv - nv, it - nt, 0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (k < w) {
      r.ev += s_w[0][k];
      r.et += s_w[1][k];
    }
    r.tv += s_w[0][k];
    r.tt += s_w[1][k];
    r.tf += s_w[2][k];
  }
  return r;
}

// Level 1, one workgroup per chunk of 256 workgroup totals: each total's exclusive base inside its chunk, the chunk's totals.
__global__ __launch_bounds__(MR) void mesh_scan_chunk_kernel(int nblk, const uint32_t* __restrict__ totals, uint2* __restrict__ bases,
                                                             uint4* __restrict__ chunk_totals) {
  __shared__ uint32_t s_w[3][4];
  const int i = (int)(blockIdx.x * (unsigned)MR + threadIdx.x);
  const uint32_t p = i < nblk ? totals[i] : 0u;
  const uint32_t nv = p & ((1u << PACK_T) - 1u), nt = (p >> PACK_T) & ((1u << (PACK_F - PACK_T)) - 1u);
  const MeshScan r = wg_scan3(nv, nt, p >> PACK_F, s_w);
  if (i < nblk) bases[i] = make_uint2(r.ev, r.et);
  if (threadIdx.x == 0) chunk_totals[blockIdx.x] = make_uint4(r.tv, r.tt, r.tf, 0u);  // <= 256 * 1280: no overflow
}

// Level 2, one workgroup: the chunks in rounds of 256 with a 64-bit carry (a round sums at most 2^16 * 1280 < 2^32). The
// LDS exchange is double-buffered, so a round costs one barrier.
__global__ __launch_bounds__(MR) void mesh_scan_top_kernel(int nchunk, const uint4* __restrict__ chunk_totals,
                                                           uint2* __restrict__ chunk_bases, uint32_t* __restrict__ header,
                                                           uint32_t* __restrict__ counts_out) {
  __shared__ uint32_t s_w[2][3][4];
  unsigned long long cv = 0, ct = 0, cf = 0;
  int buf = 0;
  for (int base = 0; base < nchunk; base += MR, buf ^= 1) {
    const int i = base + (int)threadIdx.x;
    const uint4 p = i < nchunk ? chunk_totals[i] : make_uint4(0u, 0u, 0u, 0u);
    const MeshScan r = wg_scan3(p.x, p.y, p.z, s_w[buf]);
    // the bases are only used when the totals are within the limits, where they fit 32 bits
    if (i < nchunk) chunk_bases[i] = make_uint2((uint32_t)(cv + r.ev), (uint32_t)(ct + r.et));
    cv += r.tv;
    ct += r.tt;
    cf += r.tf;
  }
  if (threadIdx.x == 0) {
    const uint32_t r[4] = {saturate32(cv), saturate32(ct), saturate32(cf), 0u};
#pragma unroll
    for (int k = 0; k < 4; k++) {
      header[k] = r[k];
      counts_out[k] = r[k];
    }
  }
}

__device__ inline double node_coord(const float* __restrict__ a, int i) { return a ? (double)a[i] : (double)i; }
__device__ inline double edge_coord(const float* __restrict__ a, int i, double t) {
  if (!a) return (double)i + t;
  const double a0 = (double)a[i];
  return a0 + t * ((double)a[i + 1] - a0);
}
__device__ inline double crossing(double iso, float va, float vb) { return (iso - (double)va) / ((double)vb - (double)va); }

__device__ inline void put_vertex(double* __restrict__ vertices, uint32_t k, uint32_t n_vertices, const MeshShift& sh, double cx,
                                  double cy, double cz) {
  if (k >= n_vertices) return;
  if (sh.on) {
    cx = cx + sh.s[0];
    cy = cy + sh.s[1];
    cz = cz + sh.s[2];
  }
  double* p = vertices + (size_t)k * 3;
  p[0] = cx;
  p[1] = cy;
  p[2] = cz;
}

__global__ __launch_bounds__(MT) void mesh_vertex_kernel(MeshDims d, const float* __restrict__ vol, double iso,
                                                         const float* __restrict__ ax, const float* __restrict__ ay,
                                                         const float* __restrict__ az, MeshShift sh, const uint2* __restrict__ bases,
                                                         const uint2* __restrict__ chunk_bases, uint32_t* __restrict__ words, double* __restrict__ vertices,
                                                         uint32_t n_vertices) {
  __shared__ uint32_t s_w[4];
  const int v = (int)(blockIdx.x * (unsigned)MT + threadIdx.x);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int x = 0, y = 0, z = 0;
  float va = 0.f, vx = 0.f, vy = 0.f, vz = 0.f;
  uint32_t flags = 0u;
  if (v < d.n) {
    voxel_xyz(d, v, x, y, z);
    const MeshStep st = voxel_steps(d, x, y, z);
    va = vol[v];
    vx = vol[v + st.sx];
    vy = vol[v + st.sy];
    vz = vol[v + st.sz];
    flags = owned_edges(d, iso, va, vx, vy, vz);
  }
  const unsigned long long b0 = __ballot(flags & 1u), b1 = __ballot(flags & 2u), b2 = __ballot(flags & 4u);
  const unsigned long long below = (1ull << lane) - 1ull;
  const uint32_t rank = __popcll(b0 & below) + __popcll(b1 & below) + __popcll(b2 & below);
  if (lane == 0) s_w[w] = __popcll(b0) + __popcll(b1) + __popcll(b2);
  __syncthreads();
  if (!flags) return;
  uint32_t k = chunk_bases[blockIdx.x / MR].x + bases[blockIdx.x].x + rank;
  for (int q = 0; q < w; q++) k += s_w[q];
  words[v] = (k & MESH_BASE_MASK) | (flags << 29);
  const double cx = node_coord(ax, x), cy = node_coord(ay, y), cz = node_coord(az, z);
  if (flags & 1u) put_vertex(vertices, k++, n_vertices, sh, edge_coord(ax, x, crossing(iso, va, vx)), cy, cz);
  if (flags & 2u) put_vertex(vertices, k++, n_vertices, sh, cx, edge_coord(ay, y, crossing(iso, va, vy)), cz);
  if (flags & 4u) put_vertex(vertices, k++, n_vertices, sh, cx, cy, edge_coord(az, z, crossing(iso, va, vz)));
}

__global__ __launch_bounds__(MT) void mesh_triangle_kernel(MeshDims d, const float* __restrict__ vol, double iso,
                                                           const uint2* __restrict__ bases, const uint2* __restrict__ chunk_bases,
                                                           const uint32_t* __restrict__ words, int32_t* __restrict__ triangles, uint32_t n_triangles) {
  __shared__ uint32_t s_w[4];
  const int v = (int)(blockIdx.x * (unsigned)MT + threadIdx.x);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int c = 0;
  if (v < d.n) {
    int x, y, z;
    voxel_xyz(d, v, x, y, z);
    const MeshStep st = voxel_steps(d, x, y, z);
    float corner[8];
    load_corners(vol, v, st, corner);
    c = cell_case(st, iso, corner);
  }
  const uint32_t nt = (uint32_t)d_table[c][15];
  uint32_t incl = nt;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t a = __shfl_up(incl, o, 64);
    if (lane >= o) incl += a;
  }
  if (lane == 63) s_w[w] = incl;
  __syncthreads();
  if (!nt) return;
  uint32_t t0 = chunk_bases[blockIdx.x / MR].y + bases[blockIdx.x].y + incl - nt;
  for (int q = 0; q < w; q++) t0 += s_w[q];
  const int S = d.ny * d.nz;
  for (uint32_t k = 0; k < nt; k++) {
    if (t0 + k >= n_triangles) return;
    int32_t* out = triangles + (size_t)(t0 + k) * 3;
    for (int j = 0; j < 3; j++) {
      const int e = d_table[c][3 * k + j], axis = e >> 2, u = e & 1, vv = (e >> 1) & 1;
      // the edge's lower corner: (u, vv) are its coordinates on the two other axes, in increasing axis order
      const int dx = axis == 0 ? 0 : u, dy = axis == 0 ? u : (axis == 1 ? 0 : vv), dz = axis == 2 ? 0 : vv;
      const uint32_t word = words[v + dx * S + dy * d.nz + dz];  // inside the volume: v is the lowest corner of a cell
      out[j] = (int32_t)((word & MESH_BASE_MASK) + __popc((word >> 29) & ((1u << axis) - 1u)));
    }
  }
}

struct MeshWS {
  uint32_t* words;   // [n] first vertex | flags << 29, written for the voxels that own a vertex
  uint32_t* totals;  // [nblk] packed totals of the count pass
  uint2* bases;      // [nblk] exclusive vertex and triangle bases inside the chunk of 256 workgroups
  uint4* chunk_totals;  // [nchunk] {vertices, triangles, non-finite, 0} of a chunk
  uint2* chunk_bases;   // [nchunk] exclusive vertex and triangle bases of the chunks
  uint32_t* header;  // {n_vertices, n_triangles, n_nonfinite, 0}
  int nblk, nchunk;
  size_t bytes;
};

MeshWS mesh_layout(char* base, int64_t n) {
  MeshWS w;
  w.nblk = (int)((n + MT - 1) / MT);
  w.nchunk = (w.nblk + MR - 1) / MR;
  size_t off = 0;
  auto carve = [&](size_t bytes) {
    char* p = base + off;
    off += (bytes + 255) & ~(size_t)255;
    return p;
  };
  w.words = reinterpret_cast<uint32_t*>(carve((size_t)n * 4));
  w.totals = reinterpret_cast<uint32_t*>(carve((size_t)w.nblk * 4));
  w.bases = reinterpret_cast<uint2*>(carve((size_t)w.nblk * 8));
  w.chunk_totals = reinterpret_cast<uint4*>(carve((size_t)w.nchunk * 16));
  w.chunk_bases = reinterpret_cast<uint2*>(carve((size_t)w.nchunk * 8));
  w.header = reinterpret_cast<uint32_t*>(carve(16));
  w.bytes = off;
  return w;
}

int mesh_dims_check(const char* who, int nx, int ny, int nz, MeshDims* d) {
  if (nx < 1 || ny < 1 || nz < 1) return fail(EOGS_ERR_INVALID_ARG, "%s: nx, ny and nz must be positive", who);
  const int64_t n = (int64_t)nx * ny * nz;  // nx ny < 2^62
  if ((int64_t)nx * ny >= ((int64_t)1 << 31) || n >= ((int64_t)1 << 31))
    return fail(EOGS_ERR_INVALID_ARG, "%s: the volume must hold fewer than 2^31 voxels", who);
  *d = MeshDims{nx, ny, nz, (int)n};
  return EOGS_OK;
}

}  // namespace

extern "C" {

int eogs_mesh_bytes(int nx, int ny, int nz, size_t* bytes) {
  MeshDims d;
  const int rc = mesh_dims_check("mesh_bytes", nx, ny, nz, &d);
  if (rc != EOGS_OK) return rc;
  if (!bytes) return fail(EOGS_ERR_INVALID_ARG, "mesh_bytes: NULL argument");
  *bytes = 256 + mesh_layout(nullptr, d.n).bytes;
  return EOGS_OK;
}

int eogs_mesh_count(int nx, int ny, int nz, const float* vol, double iso, void* ws, size_t ws_bytes, uint32_t* counts_out,
                    void* stream) {
  clear_error();
  MeshDims d;
  const int rc = mesh_dims_check("mesh_count", nx, ny, nz, &d);
  if (rc != EOGS_OK) return rc;
  if (!(iso == iso)) return fail(EOGS_ERR_INVALID_ARG, "mesh_count: iso is NaN");
  if (!vol || !ws || !counts_out) return fail(EOGS_ERR_INVALID_ARG, "mesh_count: NULL argument");
  if ((uintptr_t)counts_out & 3u) return fail(EOGS_ERR_INVALID_ARG, "mesh_count: counts_out not 4-byte aligned");
  char* base = ws_base(ws);
  const MeshWS w = mesh_layout(base, d.n);
  if ((size_t)(base - (char*)ws) + w.bytes > ws_bytes) return fail(EOGS_ERR_WORKSPACE, "mesh_count: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(mesh_count_kernel, dim3(w.nblk), dim3(MT), 0, s, d, vol, iso, w.totals);
  hipLaunchKernelGGL(mesh_scan_chunk_kernel, dim3(w.nchunk), dim3(MR), 0, s, w.nblk, w.totals, w.bases, w.chunk_totals);
  hipLaunchKernelGGL(mesh_scan_top_kernel, dim3(1), dim3(MR), 0, s, w.nchunk, w.chunk_totals, w.chunk_bases, w.header, counts_out);
  LAUNCH_TRY(s, false, "mesh_count");
  return EOGS_OK;
}

int eogs_mesh_emit(int nx, int ny, int nz, const float* vol, double iso, const float* ax, const float* ay, const float* az,
                   const double* shift, void* ws, size_t ws_bytes, double* vertices, int64_t n_vertices, int32_t* triangles,
                   int64_t n_triangles, void* stream) {
  clear_error();
  MeshDims d;
  const int rc = mesh_dims_check("mesh_emit", nx, ny, nz, &d);
  if (rc != EOGS_OK) return rc;
  if (!(iso == iso)) return fail(EOGS_ERR_INVALID_ARG, "mesh_emit: iso is NaN");
  if (!vol || !ws) return fail(EOGS_ERR_INVALID_ARG, "mesh_emit: NULL argument");
  if ((ax != nullptr) != (ay != nullptr) || (ax != nullptr) != (az != nullptr))
    return fail(EOGS_ERR_INVALID_ARG, "mesh_emit: give the three axes or none");
  if (n_vertices < 0 || n_triangles < 0) return fail(EOGS_ERR_INVALID_ARG, "mesh_emit: negative count");
  if (n_vertices >= (int64_t)EOGS_MESH_MAX_VERTICES) return fail(EOGS_ERR_OVERFLOW, "mesh_emit: 2^29 vertices or more");
  if (n_triangles >= ((int64_t)1 << 31)) return fail(EOGS_ERR_OVERFLOW, "mesh_emit: 2^31 triangles or more");
  if ((n_vertices > 0 && !vertices) || (n_triangles > 0 && !triangles)) return fail(EOGS_ERR_INVALID_ARG, "mesh_emit: NULL output");
  if ((uintptr_t)vertices & 7u) return fail(EOGS_ERR_INVALID_ARG, "mesh_emit: vertices not 8-byte aligned");
  if ((uintptr_t)triangles & 3u) return fail(EOGS_ERR_INVALID_ARG, "mesh_emit: triangles not 4-byte aligned");
  MeshShift sh{};
  if (shift) {
    sh.on = 1;
    for (int k = 0; k < 3; k++) sh.s[k] = shift[k];
  }
  char* base = ws_base(ws);
  const MeshWS w = mesh_layout(base, d.n);
  if ((size_t)(base - (char*)ws) + w.bytes > ws_bytes) return fail(EOGS_ERR_WORKSPACE, "mesh_emit: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  uint32_t counted[4];
  HIP_TRY(hipMemcpyAsync(counted, w.header, sizeof counted, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if ((int64_t)counted[0] != n_vertices || (int64_t)counted[1] != n_triangles)
    return fail(EOGS_ERR_INVALID_ARG, "mesh_emit: n_vertices / n_triangles are not the counts of mesh_count on this workspace");
  if (n_vertices == 0) return EOGS_OK;  // no vertex, no triangle
  hipLaunchKernelGGL(mesh_vertex_kernel, dim3(w.nblk), dim3(MT), 0, s, d, vol, iso, ax, ay, az, sh, w.bases, w.chunk_bases, w.words, vertices,
                     (uint32_t)n_vertices);
  if (n_triangles > 0)
    hipLaunchKernelGGL(mesh_triangle_kernel, dim3(w.nblk), dim3(MT), 0, s, d, vol, iso, w.bases, w.chunk_bases, w.words, triangles,
                       (uint32_t)n_triangles);
  LAUNCH_TRY(s, false, "mesh_emit");
  return EOGS_OK;
}

int eogs_mesh_case(int mesh_case, int8_t* edges, int* ntris) {
  if (mesh_case < 0 || mesh_case > 255) return fail(EOGS_ERR_INVALID_ARG, "mesh_case: the case is 0 .. 255");
  if (!edges || !ntris) return fail(EOGS_ERR_INVALID_ARG, "mesh_case: NULL argument");
  for (int k = 0; k < 15; k++) edges[k] = h_table[mesh_case][k];
  *ntris = h_table[mesh_case][15];
  return EOGS_OK;
}

}  // extern "C"
