// Voxel-grid downsampling of the exported point cloud on the device (g2vlm_utils.voxel_downsample / save_point_cloud(voxel_size=)):
// one vertex per occupied cell of a regular grid - the mean of the cell's points and of their colour bytes - in the order in which
// the cells first appear in the flat pixel order (view-major, row-major: g2v_cloud_compact's).  DESIGN.md 6j states the rule;
// tests/voxel_check.py restates it in numpy and the kernels are held to it byte for byte.
//
//   g2v_voxel_bounds   per-axis minimum and maximum of the participating points (the default grid origin; the extent an error names)
//   g2v_voxel_assign   voxel_of i32 [N,H,W]: the dense id of every pixel's cell, -1 for a pixel that does not take part.
//                      Six launches: table init | insert (64-bit compare-and-swap on the cell key, atomicMin of the pixel index
//                      into the slot) | mark the pixel that is its slot's first, count per block of VX_BLOCK pixels | one
//                      workgroup's scan of the block counts | first pixels take their rank | every other pixel reads the rank of
//                      its slot's first pixel.
//   g2v_voxel_reduce   per cell the integer sums n, sum q[3] (24-bit fractions inside the cell), sum colour byte[3], then one thread
//                      per cell writes the 15-byte PLY record.  Three launches: zero | accumulate | finalise.
//
// Every sum is an integer sum and every position an integer prefix sum: the bytes do not depend on the order in which anything ran.
// All arithmetic on coordinates is fp64 without contraction, so that numpy computes the same bits: it stays in this file, under
// the pragma below, which does not cover the header included above it.
#include <math.h>

// cloud_common.h: the bounds (bounds_accumulate reads a point before its mask byte, so voxel_bounds_kernel reads the points of
// masked-out pixels too; voxel_insert_kernel tests the mask first and does not), finite_f, cc_colour, the scan and count of a block
#include "cloud_common.h"
#include "common.h"
#include "g2vlm_hip.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

constexpr int VX_THREADS = 256, VX_PER = 4, VX_BLOCK = VX_THREADS * VX_PER;   // pixels (flat) per workgroup of the scan passes
constexpr int VX_REC = 15, VX_ACC = 8;                      // u64 per cell: n, Sx, Sy, Sz, Cr, Cg, Cb, key (one 64-byte line)
constexpr u64 VX_EMPTY = ~0ull;                             // a key has bit 63 clear
constexpr double VX_Q = 16777216.0, VX_G = 1048576.0;       // 2^24 fraction steps per cell, cells [-2^20, 2^20) per axis

static_assert(VX_THREADS == PC_THREADS, "cloud_common.h's scan, count and bounds are written for this workgroup");

// the cell of a finite point: key = (gx + 2^20) | (gy + 2^20) << 21 | (gz + 2^20) << 42, q = round(2^24 (t - g)); false: out of range
__device__ __forceinline__ bool vx_cell(const float p[3], double v, const double o[3], u64& key, uint32_t q[3]) {
  key = 0;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double t = ((double)p[k] - o[k]) / v;
    const double g = floor(t);
    if (!(g >= -VX_G && g < VX_G)) {                        // tested on the double: an infinite or huge t never reaches a conversion
      ok = false;
      q[k] = 0;
      continue;
    }
    const double f = t - g;
    q[k] = (uint32_t)(long long)floor(f * VX_Q + 0.5);
    key |= (u64)((long long)g + (1 << 20)) << (21 * k);
  }
  return ok;
}

__device__ __forceinline__ u64 vx_mix(u64 x) {              // splitmix64's finaliser: the keys are lattice points
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27; x *= 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

// ---------------------------------------------------------------------------------------------------------------- bounds
__global__ void voxel_bounds_init_kernel(uint32_t* b) {
  if (threadIdx.x < 3) b[threadIdx.x] = 0xffffffffu;
  else if (threadIdx.x < 7) b[threadIdx.x] = 0u;
}

__global__ __launch_bounds__(VX_THREADS) void voxel_bounds_kernel(const float* points, const uint8_t* mask, long P, uint32_t* b) {
  bounds_accumulate(points, mask, P, b);                     // the entry point refuses a NULL mask
}

__global__ void voxel_bounds_decode_kernel(uint32_t* b) {
  if (threadIdx.x < 6) b[threadIdx.x] = b[6] ? __float_as_uint(float_unord(b[threadIdx.x])) : 0u;
}

// ---------------------------------------------------------------------------------------------------------------- assign
__global__ __launch_bounds__(VX_THREADS) void voxel_init_kernel(u64* keys, int* first, u64 slots, int* stats) {
  for (u64 s = (u64)blockIdx.x * VX_THREADS + threadIdx.x; s < slots; s += (u64)gridDim.x * VX_THREADS) {
    keys[s] = VX_EMPTY;
    first[s] = 0x7fffffff;
  }
  if (blockIdx.x == 0 && threadIdx.x < 4) stats[threadIdx.x] = 0;
}

// grid ceil(P / VX_THREADS): flags[p] = 1 and slot_of[p] = the slot of p's cell where p takes part, else flags[p] = 0
__global__ __launch_bounds__(VX_THREADS) void voxel_insert_kernel(const float* points, const uint8_t* mask, long P, double v, double ox,
                                                                   double oy, double oz, u64* keys, int* first, uint32_t* slot_of,
                                                                   uint8_t* flags, int* stats, u64 smask) {
  const long p = (long)blockIdx.x * VX_THREADS + threadIdx.x;
  bool part = false, out_of_range = false;
  if (p < P && mask[p]) {                                    // the mask first: no point is read for a pixel it drops (load_eligible would)
    const float c[3] = {points[3 * p], points[3 * p + 1], points[3 * p + 2]};
    if (finite_f(c[0]) && finite_f(c[1]) && finite_f(c[2])) {
      const double o[3] = {ox, oy, oz};
      u64 key;
      uint32_t q[3];
      if (vx_cell(c, v, o, key, q)) {
        u64 slot = vx_mix(key) & smask;
        // at most one visit of every slot: the table is at most half full, so this ends long before; it never spins
        for (u64 i = 0; i <= smask; ++i) {
          // a key is written once and never changes: a stale read can only show "empty", and then the CAS tells the truth
          u64 k = __hip_atomic_load(&keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (k == VX_EMPTY) {
            k = atomicCAS(&keys[slot], VX_EMPTY, key);
            if (k == VX_EMPTY) k = key;
          }
          if (k == key) {
            part = true;
            break;
          }
          slot = (slot + 1) & smask;
        }
        if (part) {
          atomicMin(&first[slot], (int)p);
          slot_of[p] = (uint32_t)slot;
        } else {
          atomicOr(&stats[3], 1);
        }
      } else {
        out_of_range = true;
      }
    }
  }
  if (p < P) flags[p] = part ? 1 : 0;
  const int np = __popcll(__ballot(part)), no = __popcll(__ballot(out_of_range));
  if ((threadIdx.x & 63) == 0) {
    if (np) atomicAdd(&stats[1], np);
    if (no) atomicAdd(&stats[2], no);
  }
}

// grid ceil(P / VX_BLOCK): flags[p] = 2 where p is the first pixel of its cell; block_cnt[b] = such pixels of the block
__global__ __launch_bounds__(VX_THREADS) void voxel_first_kernel(long P, const int* first, const uint32_t* slot_of, uint8_t* flags,
                                                                  int* block_cnt) {
  __shared__ int sh[VX_THREADS / 64];
  const long i = (long)blockIdx.x * VX_BLOCK + threadIdx.x * VX_PER;
  int c = 0;
#pragma unroll
  for (int k = 0; k < VX_PER; ++k) {
    const long p = i + k;
    if (p < P && flags[p] == 1 && first[slot_of[p]] == (int)p) {
      flags[p] = 2;
      ++c;
    }
  }
  c = block_sum(c, sh);
  if (threadIdx.x == 0) block_cnt[blockIdx.x] = c;
}

// one workgroup: block_off[b] = first pixels before block b (block_offset_scan); stats[0] = M
__global__ __launch_bounds__(VX_THREADS) void voxel_scan_kernel(const int* block_cnt, int* block_off, long nb, int* stats) {
  __shared__ int sh[VX_THREADS / 64];
  const int cells = block_offset_scan(block_cnt, block_off, nb, sh);
  if (threadIdx.x == 0) stats[0] = cells;
}

// grid ceil(P / VX_BLOCK): the first pixel of a cell writes the cell's dense id, its rank among the first pixels
__global__ __launch_bounds__(VX_THREADS) void voxel_rank_kernel(long P, const uint8_t* flags, const int* block_off, int* voxel_of) {
  __shared__ int sh[VX_THREADS / 64];
  const long i = (long)blockIdx.x * VX_BLOCK + threadIdx.x * VX_PER;
  bool f[VX_PER];
  int c = 0;
#pragma unroll
  for (int k = 0; k < VX_PER; ++k) {
    f[k] = i + k < P && flags[i + k] == 2;
    c += f[k];
  }
  int total;
  int rank = block_off[blockIdx.x] + block_incl_scan(c, sh, total) - c;
#pragma unroll
  for (int k = 0; k < VX_PER; ++k)
    if (f[k]) voxel_of[i + k] = rank++;
}

// grid ceil(P / VX_THREADS): every other pixel reads the id that its cell's first pixel wrote in the launch before
__global__ __launch_bounds__(VX_THREADS) void voxel_label_kernel(long P, const uint8_t* flags, const int* first, const uint32_t* slot_of,
                                                                  int* voxel_of) {
  const long p = (long)blockIdx.x * VX_THREADS + threadIdx.x;
  if (p >= P) return;
  const int f = flags[p];
  if (f == 0) voxel_of[p] = -1;
  else if (f == 1) voxel_of[p] = voxel_of[first[slot_of[p]]];
}

// ---------------------------------------------------------------------------------------------------------------- reduce
__global__ __launch_bounds__(VX_THREADS) void voxel_zero_kernel(u64* acc, long n) {
  for (long i = (long)blockIdx.x * VX_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * VX_THREADS) acc[i] = 0;
}

// grid ceil(P / VX_THREADS), one pixel per lane.  runs: neighbouring lanes of a wave that share a cell are summed by a segmented
// shuffle scan and only the head of each run issues atomics (integer sums: exactly the same result).
__global__ __launch_bounds__(VX_THREADS) void voxel_accumulate_kernel(const float* points, const float* colors, const int* voxel_of,
                                                                       long P, long hw, double v, double ox, double oy, double oz, int M,
                                                                       u64* acc, int runs) {
  const long p = (long)blockIdx.x * VX_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int id = -1;
  u64 key = 0;
  uint32_t val[5] = {0, 0, 0, 0, 0};                         // q[3], n | Cr << 8, Cg | Cb << 16: a wave's sums fit 32 bits
  if (p < P) {
    id = voxel_of[p];
    if (id >= M) id = -1;                                    // never outside the accumulators, whatever the caller passed
  }
  if (id >= 0) {
    const float c[3] = {points[3 * p], points[3 * p + 1], points[3 * p + 2]};
    const double o[3] = {ox, oy, oz};
    if (vx_cell(c, v, o, key, val)) {
      const long n = p / hw, i = p - n * hw;
      const uint32_t r = cc_colour(colors[(n * 3 + 0) * hw + i]), g = cc_colour(colors[(n * 3 + 1) * hw + i]),
                     b = cc_colour(colors[(n * 3 + 2) * hw + i]);
      val[3] = 1u | (r << 8);
      val[4] = g | (b << 16);
    } else {
      id = -1;                                               // not the grid voxel_of was made with
    }
  }
  bool head = id >= 0;
  if (runs) {
    const int prev = __shfl_up(id, 1, 64);
    const bool starts = lane == 0 || prev != id;
    int run = starts ? lane : 0;                             // the lane at which this lane's run starts
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(run, o, 64);
      if (lane >= o) run = max(run, u);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int ro = __shfl_down(run, o, 64);
      const bool same = lane + o < 64 && ro == run;
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const uint32_t u = (uint32_t)__shfl_down((int)val[k], o, 64);
        if (same) val[k] += u;
      }
    }
    head = head && starts;
  }
  if (head) {
    u64* a = acc + (long)id * VX_ACC;
    atomicAdd(&a[0], (u64)(val[3] & 0xffu));
    atomicAdd(&a[1], (u64)val[0]);
    atomicAdd(&a[2], (u64)val[1]);
    atomicAdd(&a[3], (u64)val[2]);
    atomicAdd(&a[4], (u64)(val[3] >> 8));
    atomicAdd(&a[5], (u64)(val[4] & 0xffffu));
    atomicAdd(&a[6], (u64)(val[4] >> 16));
    a[7] = key;                                              // racing lanes all store the same key
  }
}

// one thread per cell
__global__ __launch_bounds__(VX_THREADS) void voxel_finalize_kernel(const u64* acc, int M, double v, double ox, double oy, double oz,
                                                                     uint8_t* rec, int* counts, float* out_points, uint8_t* out_colors) {
  const long m = (long)blockIdx.x * VX_THREADS + threadIdx.x;
  if (m >= M) return;
  const u64* a = acc + m * VX_ACC;
  const u64 n = a[0], key = a[7];
  const double o[3] = {ox, oy, oz};
  uint8_t* r = rec + m * VX_REC;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double g = (double)((long long)((key >> (21 * k)) & 0x1fffffu) - (1 << 20));
    const double mean = (double)(long long)a[1 + k] / ((double)(long long)n * VX_Q);
    const float x = (float)(o[k] + (g + mean) * v);
    const uint32_t b = __float_as_uint(x);
    r[4 * k] = (uint8_t)b; r[4 * k + 1] = (uint8_t)(b >> 8); r[4 * k + 2] = (uint8_t)(b >> 16); r[4 * k + 3] = (uint8_t)(b >> 24);
    if (out_points) out_points[m * 3 + k] = x;
    const uint8_t c = n ? (uint8_t)((2 * a[4 + k] + n) / (2 * n)) : 0;   // rounds half up
    r[12 + k] = c;
    if (out_colors) out_colors[m * 3 + k] = c;
  }
  counts[m] = (int)n;
}

inline bool bad_grid(double v, double ox, double oy, double oz) {
  return !(v > 0.0) || !isfinite(v) || !isfinite(ox) || !isfinite(oy) || !isfinite(oz);
}
inline int64_t vx_slots(int64_t P) {                         // the power of two >= 2 P: the load never exceeds 0.5
  int64_t s = 2;
  while (s < 2 * P) s <<= 1;
  return s;
}
inline int64_t vx_blocks(int64_t P) { return (P + VX_BLOCK - 1) / VX_BLOCK; }
inline unsigned vx_grid(int64_t items) {                     // grid of a grid-stride loop
  const int64_t b = (items + VX_THREADS - 1) / VX_THREADS;
  return (unsigned)(b < 1 ? 1 : b > 16384 ? 16384 : b);
}

}  // namespace

extern "C" int g2v_voxel_bounds(const void* points, const void* mask, int N, int H, int W, void* bounds, void* stream) {
  if (bad_nhw(N, H, W) || !points || !mask || !bounds || !aligned(points, 4) || !aligned(bounds, 4)) return G2V_ERR_ARG;
  const long P = (long)N * H * W;
  hipLaunchKernelGGL(voxel_bounds_init_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (uint32_t*)bounds);
  G2V_CHECK_LAUNCH();
  hipLaunchKernelGGL(voxel_bounds_kernel, dim3(vx_grid(P) > 2048 ? 2048 : vx_grid(P)), dim3(VX_THREADS), 0, (hipStream_t)stream,
                     (const float*)points, (const uint8_t*)mask, P, (uint32_t*)bounds);
  G2V_CHECK_LAUNCH();
  hipLaunchKernelGGL(voxel_bounds_decode_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (uint32_t*)bounds);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

extern "C" int64_t g2v_voxel_assign_workspace(int N, int H, int W) {
  if (bad_nhw(N, H, W)) return 0;
  const int64_t P = (int64_t)N * H * W;
  return 12 * vx_slots(P) + 4 * P + 8 * vx_blocks(P) + P;    // keys u64, first i32 | slot_of u32 | block counts, offsets | flags u8
}

extern "C" int g2v_voxel_assign(const void* points, const void* mask, int N, int H, int W, double voxel_size, double origin_x,
                                double origin_y, double origin_z, void* voxel_of, void* stats, void* workspace,
                                int64_t workspace_bytes, void* stream) {
  if (bad_nhw(N, H, W) || !points || !mask || !voxel_of || !stats || !workspace || bad_grid(voxel_size, origin_x, origin_y, origin_z))
    return G2V_ERR_ARG;
  if (workspace_bytes < g2v_voxel_assign_workspace(N, H, W) || !aligned(points, 4) || !aligned(voxel_of, 4) || !aligned(stats, 4) ||
      !aligned(workspace, 8))
    return G2V_ERR_ARG;
  const long P = (long)N * H * W;
  const int64_t slots = vx_slots(P), nb = vx_blocks(P);
  u64* keys = (u64*)workspace;
  int* first = (int*)(keys + slots);
  uint32_t* slot_of = (uint32_t*)(first + slots);
  int* block_cnt = (int*)(slot_of + P);
  int* block_off = block_cnt + nb;
  uint8_t* flags = (uint8_t*)(block_off + nb);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 per_pixel((unsigned)((P + VX_THREADS - 1) / VX_THREADS)), per_block((unsigned)nb), wg(VX_THREADS);
  hipLaunchKernelGGL(voxel_init_kernel, dim3(vx_grid(slots)), wg, 0, st, keys, first, (u64)slots, (int*)stats);
  G2V_CHECK_LAUNCH();
  hipLaunchKernelGGL(voxel_insert_kernel, per_pixel, wg, 0, st, (const float*)points, (const uint8_t*)mask, P, voxel_size, origin_x,
                     origin_y, origin_z, keys, first, slot_of, flags, (int*)stats, (u64)(slots - 1));
  G2V_CHECK_LAUNCH();
  hipLaunchKernelGGL(voxel_first_kernel, per_block, wg, 0, st, P, (const int*)first, (const uint32_t*)slot_of, flags, block_cnt);
  G2V_CHECK_LAUNCH();
  hipLaunchKernelGGL(voxel_scan_kernel, dim3(1), wg, 0, st, (const int*)block_cnt, block_off, (long)nb, (int*)stats);
  G2V_CHECK_LAUNCH();
  hipLaunchKernelGGL(voxel_rank_kernel, per_block, wg, 0, st, P, (const uint8_t*)flags, (const int*)block_off, (int*)voxel_of);
  G2V_CHECK_LAUNCH();
  hipLaunchKernelGGL(voxel_label_kernel, per_pixel, wg, 0, st, P, (const uint8_t*)flags, (const int*)first, (const uint32_t*)slot_of,
                     (int*)voxel_of);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

extern "C" int64_t g2v_voxel_reduce_workspace(int64_t M) {
  if (M <= 0 || M > 0x7fffffffLL) return 0;
  return 8 * (int64_t)VX_ACC * M;
}

extern "C" int g2v_voxel_reduce(const void* points, const void* colors, const void* voxel_of, int N, int H, int W, double voxel_size,
                                double origin_x, double origin_y, double origin_z, int64_t M, void* records, void* counts,
                                void* out_points, void* out_colors, void* workspace, int64_t workspace_bytes, int flags, void* stream) {
  if (bad_nhw(N, H, W) || !points || !colors || !voxel_of || bad_grid(voxel_size, origin_x, origin_y, origin_z) || M < 0 ||
      M > (int64_t)N * H * W || (flags & ~G2V_VOXEL_NO_RUNS))
    return G2V_ERR_ARG;
  if (!aligned(points, 4) || !aligned(colors, 4) || !aligned(voxel_of, 4)) return G2V_ERR_ARG;
  if (M == 0) return G2V_OK;
  if (!records || !counts || !workspace || workspace_bytes < g2v_voxel_reduce_workspace(M) || !aligned(counts, 4) ||
      !aligned(workspace, 8) || (out_points && !aligned(out_points, 4)))
    return G2V_ERR_ARG;
  const long P = (long)N * H * W, hw = (long)H * W;
  u64* acc = (u64*)workspace;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 wg(VX_THREADS);
  hipLaunchKernelGGL(voxel_zero_kernel, dim3(vx_grid(M * VX_ACC)), wg, 0, st, acc, (long)M * VX_ACC);
  G2V_CHECK_LAUNCH();
  hipLaunchKernelGGL(voxel_accumulate_kernel, dim3((unsigned)((P + VX_THREADS - 1) / VX_THREADS)), wg, 0, st, (const float*)points,
                     (const float*)colors, (const int*)voxel_of, P, hw, voxel_size, origin_x, origin_y, origin_z, (int)M, acc,
                     (flags & G2V_VOXEL_NO_RUNS) ? 0 : 1);
  G2V_CHECK_LAUNCH();
  hipLaunchKernelGGL(voxel_finalize_kernel, dim3((unsigned)((M + VX_THREADS - 1) / VX_THREADS)), wg, 0, st, (const u64*)acc, (int)M,
                     voxel_size, origin_x, origin_y, origin_z, (uint8_t*)records, (int*)counts, (float*)out_points, (uint8_t*)out_colors);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}
