// Exact nearest neighbour between two clouds (g2vlm_utils.nearest_points / evaluate_reconstruction): for every query point the
// target point that minimises the fp32 squared distance, ties to the lowest index.  Inputs are queries fp32 [Nq,3] and targets fp32
// [Nt,3], each with an optional u8 mask, and an optional largest distance.
//
// The rule (include/g2vlm_hip.h and DESIGN.md 6p state it in full; tests/nn_check.py restates it in numpy): a point takes part if
// its mask byte is non-zero and its coordinates are finite (cloud_common.h's load_eligible); d = q - t, d2 = (d0 d0 + d1 d1) + d2 d2
// in fp32, every operation rounded once (cloud_common.h's sq_dist3, contraction off in its body as in this file); a target counts
// unless d2 > max_distance^2; the answer is the minimum of the 64-bit key bits(d2) << 32 | index (dist_key) over the counting
// targets.  A minimum of integers does not depend on the order in which it is taken, so
// the search structure below is free to visit the targets in any order and to skip those that provably cannot hold the minimum.
//
//   nn_init_kernel      zeroes the stats and the bounds accumulators.
//   nn_bounds_kernel    per-axis minimum and maximum of the participating targets and their number (cloud_common.h's
//                       bounds_accumulate, as voxel.hip: ordered-integer atomics, order-free).
//   nn_setup_kernel     one thread: the grid's origin, its cell width (cubic cells: the smallest width whose grid has at most C
//                       cells, C = the largest cube <= 2 Nt, known on the host) and cells per axis from the bounds; stats[1].
//   brute path          nn_keys_kernel fills the keys with EMPTY; nn_brute_kernel: a workgroup of 256 queries (one per lane, the
//                       running minimum key in registers) walks a slice of the targets through LDS in tiles of 1024 (x, y, z,
//                       index or -1) and ends with one 64-bit atomicMin per query; at most 2^36 pairs per launch.
//   grid path           nn_cell_kernel: the cell of every target and its rank inside the cell (the return value of the histogram's
//                       atomicAdd); nn_scan_*: exclusive scan of the histogram (blocks of 1024, one workgroup over the block sums,
//                       add); nn_scatter_kernel: (x, y, z, index) of every target to cell start + rank; nn_query_kernel: a lane per
//                       query walks Chebyshev rings of cells around the cell of its position clamped to the box until the stop test
//                       (below) holds or the grid is exhausted.
//   nn_finalize_kernel  key -> index and sq_distance; stats.
//
// The ranks inside a cell depend on the order in which the atomics arrive, so the sorted copy in the workspace is not reproducible
// byte for byte; the outputs are, because the key minimum does not see that order.
#include <math.h>

#include "cloud_common.h"                                   // load_eligible, sq_dist3, dist_key, the bounds, the scan of a block
#include "common.h"
#include "g2vlm_hip.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

constexpr int NN_THREADS = 256;
static_assert(NN_THREADS == PC_THREADS, "cloud_common.h's scan and bounds are written for this workgroup");
constexpr int NN_TILE = 1024;                               // targets of one LDS tile of the brute path: 16 KiB
constexpr long NN_BRUTE_PAIRS = 1L << 36;                   // pairs of one launch of the brute path at most: 26 ms at the measured rate
constexpr int NN_SCAN_PER = 4, NN_SCAN_BLOCK = NN_THREADS * NN_SCAN_PER;   // cells per workgroup of the scan
constexpr int NN_MAX_CELLS = 256;                           // cells per axis at most
constexpr int NN_HEADER = 256;                              // bytes of the workspace before the arrays
constexpr u64 NN_EMPTY = ~0ull;                             // no key has this value: bits(d2) <= 0x7f800000
// Default dispatch: the brute path below this many targets.  Measured on the MI355X (tools/bench_nn.py, profiles/nn_bench.json,
// DESIGN.md 6p): on the floor-and-sphere scene the brute path was faster than the grid path at every size measured - Nt from 256 to
// 131 072 at 7 770 and 268 324 queries (2.4 - 100 x), and 16 384 queries against 2.1 M and 8.4 M targets (105 and 102 x) - because
// a few targets near the horizon stretch the box to 3 km and one cubic cell then holds a quarter of the targets.  So the default
// is the brute path for every Nt, and the grid path runs only under G2V_NN_GRID until it copes with such boxes.
constexpr int64_t NN_BRUTE_BELOW = INT64_MAX;
// The stop test's safety factor: the fp32 d2 of the rule lies within 4 * 2^-24 relative of the real squared distance (three
// roundings of a difference, three of a square, two of a sum, each 2^-24; first order), cell coordinates are fp64.  2^-20 leaves 4x.
constexpr double NN_SAFE = 1.0 + 1.0 / 1048576.0;
constexpr double NN_TINY = 1e-30;                           // below this bound fp32 underflow could matter: never stop on it

struct Params {                                             // at the start of the workspace; written by nn_setup_kernel
  uint32_t bounds[8];                                       // ordered lo[3], hi[3], count, -
  double lo[3], inv[3], w;                                  // origin, cells per unit (0 on an axis of zero extent), the cells' width
  float flo[3], fhi[3];                                     // the box
  int g[3];                                                 // cells per axis; 1 on an axis of zero extent; g0 g1 g2 <= C
};
static_assert(sizeof(Params) <= NN_HEADER, "header");

__global__ void nn_init_kernel(Params* P, int* stats) {
  const int t = threadIdx.x;
  if (t < 3) P->bounds[t] = 0xffffffffu;
  else if (t < 8) P->bounds[t] = 0u;
  if (t < 4) stats[t] = 0;
}

__global__ __launch_bounds__(NN_THREADS) void nn_bounds_kernel(const float* __restrict__ target, const uint8_t* __restrict__ mask, long Nt,
                                                                Params* P) {
  bounds_accumulate(target, mask, Nt, P->bounds);
}

// cells along an axis of extent e under cell width w: the last one holds the maximum itself
__device__ __forceinline__ double nn_cells(double e, double w) { return e > 0.0 ? floor(e / w) + 1.0 : 1.0; }

// one thread.  The cells are cubes of one width w on every axis - the ring walk's bound is r w, so a box that is thin along one axis
// must not make the cells thin along it - and w is the smallest width (to 2^-40 relative, by bisection) under which the grid has at
// most C cells.  An axis of zero extent (all targets equal there, one target, no target) has one cell: nothing is divided by an
// extent of zero and the ring walk never looks for room along it.
__global__ void nn_setup_kernel(Params* P, long C, int* stats) {
  if (threadIdx.x != 0) return;
  const int cnt = (int)P->bounds[6];
  stats[1] = cnt;
  double ext[3], emax = 0.0;
  for (int k = 0; k < 3; ++k) {
    const float lo = cnt ? float_unord(P->bounds[k]) : 0.f, hi = cnt ? float_unord(P->bounds[3 + k]) : 0.f;
    ext[k] = (double)hi - (double)lo;                       // finite: both are finite floats
    if (!(ext[k] > 0.0)) ext[k] = 0.0;
    emax = fmax(emax, ext[k]);
    P->flo[k] = lo; P->fhi[k] = hi;
    P->lo[k] = (double)lo;
  }
  double w = 0.0;
  if (emax > 0.0) {
    double lo_w = emax * (1.0 / 16777216.0), hi_w = emax * 2.0;   // hi_w: one cell per axis, always allowed; lo_w: > C cells or good enough
    if (nn_cells(ext[0], lo_w) * nn_cells(ext[1], lo_w) * nn_cells(ext[2], lo_w) <= (double)C) hi_w = lo_w;
    else
      for (int it = 0; it < 64; ++it) {
        const double mid = sqrt(lo_w * hi_w);
        if (nn_cells(ext[0], mid) * nn_cells(ext[1], mid) * nn_cells(ext[2], mid) <= (double)C) hi_w = mid; else lo_w = mid;
      }
    w = hi_w;
  }
  P->w = w;
  for (int k = 0; k < 3; ++k) {
    const bool flat = !(ext[k] > 0.0);
    P->g[k] = flat ? 1 : (int)nn_cells(ext[k], w);          // <= C <= 2^24
    P->inv[k] = flat ? 0.0 : 1.0 / w;
  }
}

// cell coordinate along one axis of a coordinate inside the box
__device__ __forceinline__ int nn_cell1(float c, double lo, double inv, int g) {
  const double t = ((double)c - lo) * inv;                  // in [0, g) up to rounding: c is inside the box
  int i = (int)t;
  return i < 0 ? 0 : (i > g - 1 ? g - 1 : i);
}

__global__ __launch_bounds__(NN_THREADS) void nn_keys_kernel(u64* keys, long Nq) {
  const long q = (long)blockIdx.x * NN_THREADS + threadIdx.x;
  if (q < Nq) keys[q] = NN_EMPTY;
}

// ---------------------------------------------------------------------------------------------------------------- brute path
// grid (query blocks, target slices): slice s holds the tiles [tile0 + s * tiles_per, tile0 + (s + 1) * tiles_per) below tile_end
__global__ __launch_bounds__(NN_THREADS) void nn_brute_kernel(const float* __restrict__ query, const uint8_t* __restrict__ qmask, long Nq,
                                                               const float* __restrict__ target, const uint8_t* __restrict__ tmask, long Nt,
                                                               float m2, long tile0, long tile_end, long tiles_per,
                                                               u64* __restrict__ keys) {
  __shared__ float4 tile[NN_TILE];
  const long q = (long)blockIdx.x * NN_THREADS + threadIdx.x;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  const bool part = q < Nq && load_eligible(query, qmask, q, qx, qy, qz);
  u64 best = NN_EMPTY;
  const long t_begin = (tile0 + (long)blockIdx.y * tiles_per) * NN_TILE;
  long t_end = t_begin + tiles_per * NN_TILE;
  if (t_end > tile_end * NN_TILE) t_end = tile_end * NN_TILE;
  if (t_end > Nt) t_end = Nt;
  for (long t0 = t_begin; t0 < t_end; t0 += NN_TILE) {
    const int n = (int)((t_end - t0) < NN_TILE ? (t_end - t0) : NN_TILE);
    __syncthreads();                                         // the tile of the pass before has been read
    for (int j = threadIdx.x; j < n; j += NN_THREADS) {
      float x, y, z;
      const bool ok = load_eligible(target, tmask, t0 + j, x, y, z);
      tile[j] = make_float4(x, y, z, __int_as_float(ok ? (int)(t0 + j) : -1));
    }
    __syncthreads();
    if (!part) continue;
    for (int j = 0; j < n; ++j) {
      const float4 t = tile[j];                             // every lane reads the same address: a broadcast
      const int idx = __float_as_int(t.w);
      const float d2 = sq_dist3(qx, qy, qz, t.x, t.y, t.z);
      if (idx >= 0 && d2 <= m2) {                           // d2 is never NaN for finite inputs; m2 = +inf: no limit
        const u64 k = dist_key(d2, (uint32_t)idx);
        best = k < best ? k : best;
      }
    }
  }
  if (part && best != NN_EMPTY) atomicMin(&keys[q], best);
}

// ---------------------------------------------------------------------------------------------------------------- grid path
__global__ __launch_bounds__(NN_THREADS) void nn_zero_kernel(int* a, long n) {
  for (long i = (long)blockIdx.x * NN_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * NN_THREADS) a[i] = 0;
}

// cell_of[t] = the cell of target t or -1, rank[t] = how many targets reached the cell before it; count[cell] = the histogram
__global__ __launch_bounds__(NN_THREADS) void nn_cell_kernel(const float* __restrict__ target, const uint8_t* __restrict__ tmask, long Nt,
                                                              const Params* __restrict__ P, int* __restrict__ cell_of,
                                                              int* __restrict__ rank, int* __restrict__ count) {
  const long t = (long)blockIdx.x * NN_THREADS + threadIdx.x;
  if (t >= Nt) return;
  float x, y, z;
  int cell = -1, r = 0;
  if (load_eligible(target, tmask, t, x, y, z)) {
    const int ix = nn_cell1(x, P->lo[0], P->inv[0], P->g[0]), iy = nn_cell1(y, P->lo[1], P->inv[1], P->g[1]),
              iz = nn_cell1(z, P->lo[2], P->inv[2], P->g[2]);
    cell = (iz * P->g[1] + iy) * P->g[0] + ix;              // < g0 g1 g2 <= C <= 2^24
    r = atomicAdd(&count[cell], 1);
  }
  cell_of[t] = cell;
  rank[t] = r;
}

// a[0..C) -> its exclusive scan inside every block of NN_SCAN_BLOCK cells; bsum[b] = the block's total
__global__ __launch_bounds__(NN_THREADS) void nn_scan_block_kernel(int* __restrict__ a, long C, int* __restrict__ bsum) {
  __shared__ int sh[NN_THREADS / 64];
  const long i = (long)blockIdx.x * NN_SCAN_BLOCK + threadIdx.x * NN_SCAN_PER;
  int v[NN_SCAN_PER], c = 0;
#pragma unroll
  for (int k = 0; k < NN_SCAN_PER; ++k) {
    v[k] = (i + k < C) ? a[i + k] : 0;
    c += v[k];
  }
  int total;
  int run = block_incl_scan(c, sh, total) - c;
#pragma unroll
  for (int k = 0; k < NN_SCAN_PER; ++k) {
    if (i + k < C) a[i + k] = run;
    run += v[k];
  }
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one workgroup: bsum -> its exclusive scan, in place (block_offset_scan)
__global__ __launch_bounds__(NN_THREADS) void nn_scan_sums_kernel(int* bsum, long nb) {
  __shared__ int sh[NN_THREADS / 64];
  block_offset_scan(bsum, bsum, nb, sh);
}

// start[c] += the sum of the blocks before its own; start[C] = the number of participating targets
__global__ __launch_bounds__(NN_THREADS) void nn_scan_add_kernel(int* __restrict__ start, long C, const int* __restrict__ bsum,
                                                                  const Params* __restrict__ P) {
  const long i = (long)blockIdx.x * NN_SCAN_BLOCK + threadIdx.x * NN_SCAN_PER;
  const int add = bsum[blockIdx.x];
#pragma unroll
  for (int k = 0; k < NN_SCAN_PER; ++k)
    if (i + k < C) start[i + k] += add;
  if (blockIdx.x == 0 && threadIdx.x == 0) start[C] = (int)P->bounds[6];
}

__global__ __launch_bounds__(NN_THREADS) void nn_scatter_kernel(const float* __restrict__ target, long Nt, const int* __restrict__ cell_of,
                                                                 const int* __restrict__ rank, const int* __restrict__ start,
                                                                 float4* __restrict__ sorted) {
  const long t = (long)blockIdx.x * NN_THREADS + threadIdx.x;
  if (t >= Nt) return;
  const int cell = cell_of[t];
  if (cell < 0) return;
  // start[cell] + rank < start[cell + 1] <= the number of participating targets <= Nt: inside `sorted`
  sorted[start[cell] + rank[t]] = make_float4(target[3 * t], target[3 * t + 1], target[3 * t + 2], __int_as_float((int)t));
}

__device__ __forceinline__ void nn_scan_range(const float4* __restrict__ sorted, int b, int e, float qx, float qy, float qz, float m2,
                                              u64& best) {
  for (int j = b; j < e; ++j) {
    const float4 t = sorted[j];
    const float d2 = sq_dist3(qx, qy, qz, t.x, t.y, t.z);
    if (d2 <= m2) {
      const u64 k = dist_key(d2, __float_as_uint(t.w));
      best = k < best ? k : best;
    }
  }
}

// A lane per query.  c = the query clamped to the box, (ix, iy, iz) = its cell.  Ring r = the cells at Chebyshev distance r from
// that cell, cut to the grid.  The stop test after ring r: a target t in a cell not yet visited has a cell coordinate
// that differs by at least r + 1 from the query's along some axis a, so |c_a - t_a| >= r w; the box is convex and c is q's
// projection onto it, so (q - c) . (t - c) <= 0 and |q - t|^2 >= |q - c|^2 + |c - t|^2 >= |q - c|^2 + B^2 with B = r w.
// Once best d2 * NN_SAFE <= that bound no unvisited target can have a key below the best one (its fp32 d2 is strictly larger), and
// once m2 * NN_SAFE < the bound none can count.  A best d2 of +inf never stops the walk: the whole grid is then visited and the key
// minimum is the lowest participating index.
__global__ __launch_bounds__(NN_THREADS) void nn_query_kernel(const float* __restrict__ query, const uint8_t* __restrict__ qmask, long Nq,
                                                               const Params* __restrict__ P, const int* __restrict__ start,
                                                               const float4* __restrict__ sorted, float m2, u64* __restrict__ keys) {
  const long q = (long)blockIdx.x * NN_THREADS + threadIdx.x;
  if (q >= Nq) return;
  float qx, qy, qz;
  u64 best = NN_EMPTY;
  if (load_eligible(query, qmask, q, qx, qy, qz) && P->bounds[6] != 0) {
    const float qv[3] = {qx, qy, qz};
    int i0[3], g[3];
    double qc2 = 0.0;
    const double w = P->w;
    int rmax = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float c = fminf(fmaxf(qv[a], P->flo[a]), P->fhi[a]);
      g[a] = P->g[a];
      i0[a] = nn_cell1(c, P->lo[a], P->inv[a], g[a]);
      const double dq = (double)qv[a] - (double)c;
      qc2 += dq * dq;
      const int reach = max(i0[a], g[a] - 1 - i0[a]);
      rmax = max(rmax, reach);
    }
    for (int r = 0; r <= rmax; ++r) {
      const int x0 = max(i0[0] - r, 0), x1 = min(i0[0] + r, g[0] - 1);
      const int y0 = max(i0[1] - r, 0), y1 = min(i0[1] + r, g[1] - 1);
      const int z0 = max(i0[2] - r, 0), z1 = min(i0[2] + r, g[2] - 1);
      for (int z = z0; z <= z1; ++z) {
        const bool zshell = (z - i0[2] == r) || (i0[2] - z == r);
        for (int y = y0; y <= y1; ++y) {
          const int row = (z * g[1] + y) * g[0];
          if (zshell || (y - i0[1] == r) || (i0[1] - y == r)) {      // a whole row of the ring: its cells are consecutive
            nn_scan_range(sorted, start[row + x0], start[row + x1 + 1], qx, qy, qz, m2, best);
          } else {                                                  // r > 0 here: the two end cells, where the grid has them
            if (i0[0] - r >= 0) nn_scan_range(sorted, start[row + i0[0] - r], start[row + i0[0] - r + 1], qx, qy, qz, m2, best);
            if (i0[0] + r <= g[0] - 1) nn_scan_range(sorted, start[row + i0[0] + r], start[row + i0[0] + r + 1], qx, qy, qz, m2, best);
          }
        }
      }
      if (r == rmax) break;
      const double B = (double)r * w;                        // some axis has room (r < rmax), so w > 0
      const double bound = qc2 + B * B;
      if (!(bound > NN_TINY)) continue;
      const float bd = __uint_as_float((uint32_t)(best >> 32));
      if (best != NN_EMPTY && finite_f(bd) && (double)bd * NN_SAFE <= bound) break;
      if (finite_f(m2) && (double)m2 * NN_SAFE < bound) break;
    }
  }
  keys[q] = best;
}

// ---------------------------------------------------------------------------------------------------------------- results
__global__ __launch_bounds__(NN_THREADS) void nn_finalize_kernel(const float* __restrict__ query, const uint8_t* __restrict__ qmask, long Nq,
                                                                  const u64* __restrict__ keys, int* __restrict__ index,
                                                                  float* __restrict__ sq_distance, int* __restrict__ stats) {
  const long q = (long)blockIdx.x * NN_THREADS + threadIdx.x;
  int part = 0, none = 0;
  if (q < Nq) {
    float x, y, z;
    part = load_eligible(query, qmask, q, x, y, z) ? 1 : 0;
    const u64 k = part ? keys[q] : NN_EMPTY;                // a query that takes no part: whatever the slot holds is not read
    const bool found = k != NN_EMPTY;
    none = part && !found;
    index[q] = found ? (int)(uint32_t)k : -1;
    sq_distance[q] = found ? __uint_as_float((uint32_t)(k >> 32)) : INFINITY;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    part += __shfl_xor(part, o, 64);
    none += __shfl_xor(none, o, 64);
  }
  if ((threadIdx.x & 63) == 0 && part) {
    atomicAdd(&stats[0], part);
    if (none) atomicAdd(&stats[2], none);
    if (part - none) atomicAdd(&stats[3], part - none);
  }
}

// G: the largest G with G^3 <= 2 Nt, in [1, NN_MAX_CELLS]; the grid has at most G^3 cells - from Nt alone, so the workspace is
// known on the host
inline int cells_per_axis(int64_t Nt) {
  int G = 1;
  while (G < NN_MAX_CELLS && (int64_t)(G + 1) * (G + 1) * (G + 1) <= 2 * Nt) ++G;
  return G;
}

struct Layout { int64_t sorted, keys, cell_of, rank, start, bsum, bytes, cells, nb; };
inline Layout layout(int64_t Nq, int64_t Nt) {
  Layout l;
  const int G = cells_per_axis(Nt);
  l.cells = (int64_t)G * G * G;
  l.nb = (l.cells + NN_SCAN_BLOCK - 1) / NN_SCAN_BLOCK;
  l.sorted = NN_HEADER;                                     // 16-byte aligned
  l.keys = l.sorted + 16 * Nt;
  l.cell_of = l.keys + 8 * Nq;
  l.rank = l.cell_of + 4 * Nt;
  l.start = l.rank + 4 * Nt;
  l.bsum = l.start + 4 * (l.cells + 1);
  l.bytes = l.bsum + 4 * l.nb;
  return l;
}

inline bool bad_counts(int64_t Nq, int64_t Nt) { return Nq < 0 || Nt < 0 || Nq > 0x7fffffffLL || Nt > 0x7fffffffLL; }
inline unsigned blocks_of(long n, long per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

extern "C" int64_t g2v_cloud_nn_workspace(int64_t Nq, int64_t Nt) {
  if (bad_counts(Nq, Nt)) return 0;
  return layout(Nq, Nt).bytes;
}

extern "C" int g2v_cloud_nn(const void* query, const void* query_mask, int64_t Nq, const void* target, const void* target_mask, int64_t Nt,
                            float max_distance, int flags, void* index, void* sq_distance, void* stats, void* workspace,
                            int64_t workspace_bytes, void* stream) {
  if (bad_counts(Nq, Nt) || !stats || !workspace || (flags & ~(G2V_NN_BRUTE | G2V_NN_GRID)) ||
      (flags & (G2V_NN_BRUTE | G2V_NN_GRID)) == (G2V_NN_BRUTE | G2V_NN_GRID))
    return G2V_ERR_ARG;
  if (!(max_distance >= 0.f)) return G2V_ERR_ARG;            // negative or NaN; +inf: no limit
  if ((Nq > 0 && (!query || !index || !sq_distance)) || (Nt > 0 && !target)) return G2V_ERR_ARG;
  if (!aligned(query, 4) || !aligned(target, 4) || !aligned(index, 4) || !aligned(sq_distance, 4) || !aligned(stats, 4) ||
      !aligned(workspace, 16) || workspace_bytes < g2v_cloud_nn_workspace(Nq, Nt))
    return G2V_ERR_ARG;
  const Layout l = layout(Nq, Nt);
  uint8_t* ws = (uint8_t*)workspace;
  Params* P = (Params*)ws;
  float4* sorted = (float4*)(ws + l.sorted);
  u64* keys = (u64*)(ws + l.keys);
  int *cell_of = (int*)(ws + l.cell_of), *rank = (int*)(ws + l.rank), *start = (int*)(ws + l.start), *bsum = (int*)(ws + l.bsum);
  const float m2 = max_distance * max_distance;              // one fp32 product (+inf stays +inf)
  const float* Q = (const float*)query;
  const float* T = (const float*)target;
  const uint8_t *qm = (const uint8_t*)query_mask, *tm = (const uint8_t*)target_mask;
  hipStream_t s = (hipStream_t)stream;
  const dim3 th(NN_THREADS);
  const unsigned qblocks = blocks_of(Nq, NN_THREADS), tblocks = blocks_of(Nt, NN_THREADS);

  hipLaunchKernelGGL(nn_init_kernel, dim3(1), dim3(64), 0, s, P, (int*)stats);
  G2V_CHECK_LAUNCH();
  if (Nt > 0) {
    hipLaunchKernelGGL(nn_bounds_kernel, dim3(tblocks < 2048u ? tblocks : 2048u), th, 0, s, T, tm, (long)Nt, P);
    G2V_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(nn_setup_kernel, dim3(1), dim3(64), 0, s, P, (long)l.cells, (int*)stats);
  G2V_CHECK_LAUNCH();
  if (Nq == 0) return G2V_OK;
  const bool brute = (flags & G2V_NN_BRUTE) || (!(flags & G2V_NN_GRID) && Nt < NN_BRUTE_BELOW);
  if (Nt == 0 || brute) {
    hipLaunchKernelGGL(nn_keys_kernel, dim3(qblocks), th, 0, s, keys, (long)Nq);
    G2V_CHECK_LAUNCH();
    if (Nt > 0) {
      // One launch covers at most NN_BRUTE_PAIRS pairs, so that no single kernel occupies a device for long; the launches and,
      // inside one, the slices of its targets (enough workgroups to fill the device when the queries alone do not) are merged by
      // the atomic minimum.
      const long all_tiles = (Nt + NN_TILE - 1) / NN_TILE;
      long per_launch = NN_BRUTE_PAIRS / ((long)qblocks * NN_THREADS * NN_TILE);
      if (per_launch < 1) per_launch = 1;
      for (long tile0 = 0; tile0 < all_tiles; tile0 += per_launch) {
        const long tile_end = tile0 + per_launch < all_tiles ? tile0 + per_launch : all_tiles;
        const long tiles = tile_end - tile0;
        long slices = qblocks >= 2048u ? 1 : (2048 + qblocks - 1) / qblocks;
        if (slices > tiles) slices = tiles;
        if (slices > 65535) slices = 65535;
        const long tiles_per = (tiles + slices - 1) / slices;
        slices = (tiles + tiles_per - 1) / tiles_per;
        hipLaunchKernelGGL(nn_brute_kernel, dim3(qblocks, (unsigned)slices), th, 0, s, Q, qm, (long)Nq, T, tm, (long)Nt, m2, tile0, tile_end,
                           tiles_per, keys);
        G2V_CHECK_LAUNCH();
      }
    }
  } else {
    const unsigned zb = blocks_of(l.cells, NN_THREADS);
    hipLaunchKernelGGL(nn_zero_kernel, dim3(zb < 4096u ? zb : 4096u), th, 0, s, start, (long)l.cells);
    G2V_CHECK_LAUNCH();
    hipLaunchKernelGGL(nn_cell_kernel, dim3(tblocks), th, 0, s, T, tm, (long)Nt, (const Params*)P, cell_of, rank, start);
    G2V_CHECK_LAUNCH();
    hipLaunchKernelGGL(nn_scan_block_kernel, dim3((unsigned)l.nb), th, 0, s, start, (long)l.cells, bsum);
    G2V_CHECK_LAUNCH();
    hipLaunchKernelGGL(nn_scan_sums_kernel, dim3(1), th, 0, s, bsum, (long)l.nb);
    G2V_CHECK_LAUNCH();
    hipLaunchKernelGGL(nn_scan_add_kernel, dim3((unsigned)l.nb), th, 0, s, start, (long)l.cells, (const int*)bsum, (const Params*)P);
    G2V_CHECK_LAUNCH();
    hipLaunchKernelGGL(nn_scatter_kernel, dim3(tblocks), th, 0, s, T, (long)Nt, (const int*)cell_of, (const int*)rank, (const int*)start,
                       sorted);
    G2V_CHECK_LAUNCH();
    hipLaunchKernelGGL(nn_query_kernel, dim3(qblocks), th, 0, s, Q, qm, (long)Nq, (const Params*)P, (const int*)start,
                       (const float4*)sorted, m2, keys);
    G2V_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(nn_finalize_kernel, dim3(qblocks), th, 0, s, Q, qm, (long)Nq, (const u64*)keys, (int*)index, (float*)sq_distance,
                     (int*)stats);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}
