// What the point-cloud kernels share (cloud.hip, voxel.hip, consistency.hip, render.hip, mesh.hip, nn.hip): one definition of every
// rule that two of them must agree on bit for bit - which pixel takes part, how a point is projected into a camera, the squared
// distance, the colour byte, the depth key, the float order of the bounds - and of the workgroup primitives of their compaction
// passes (counts per block of 1024 items, one workgroup's scan of the block counts, ranks inside a block, the staged write-out).
//
// A file-scope `#pragma clang fp contract(off)` of the including file does not reach up into this header: every function here whose
// result depends on uncontracted arithmetic (to_camera, sq_dist3) carries the pragma inside its own body.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The scan and flush helpers are written for this one workgroup size; every file asserts that its own *_THREADS equals it.
constexpr int PC_THREADS = 256, PC_WAVES = PC_THREADS / 64;

// ------------------------------------------------------------------------------------------------------- per-point rules
__device__ __forceinline__ uint8_t cc_colour(float c) {      // host.write_ply_binary: (uint8)(clip((double)c, 0, 1) * 255)
  const double v = fmin(fmax((double)c, 0.0), 1.0) * 255.0;
  return (uint8_t)(int)v;
}

__device__ __forceinline__ bool finite_f(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// The point of pixel p of a [..,3] fp32 array; true where it takes part: the mask (NULL: all pixels) keeps it and x, y, z are
// finite.  The point is read first, whatever the mask says: a masked-out pixel's point is read too (in bounds, like the mask
// byte), so x, y, z are always the pixel's.  A kernel that must not read what the mask drops tests the mask itself.
__device__ __forceinline__ bool load_eligible(const float* __restrict__ points, const uint8_t* __restrict__ mask, long p, float& x,
                                              float& y, float& z) {
  x = points[3 * p]; y = points[3 * p + 1]; z = points[3 * p + 2];
  return (!mask || mask[p] != 0) && finite_f(x) && finite_f(y) && finite_f(z);
}

// A world point in a pinhole camera: q = R^T (P - t), u = fx q0/q2 + cx, v = fy q1/q2 + cy.  pose = the camera-to-world matrix
// [4,4] row-major, k = K [3,3] row-major.  Contraction off: every - * + below is its own rounding (v_sub_f32 / v_mul_f32 /
// v_add_f32, never v_fma / v_fmac), so that a numpy restatement gives the same bytes.
struct CamPoint { float q0, q1, q2, u, v; };
__device__ __forceinline__ CamPoint to_camera(float px, float py, float pz, const float* __restrict__ pose, const float* __restrict__ k) {
#pragma clang fp contract(off)
  const float d0 = px - pose[3], d1 = py - pose[7], d2 = pz - pose[11];
  CamPoint c;
  c.q0 = (pose[0] * d0 + pose[4] * d1) + pose[8] * d2;
  c.q1 = (pose[1] * d0 + pose[5] * d1) + pose[9] * d2;
  c.q2 = (pose[2] * d0 + pose[6] * d1) + pose[10] * d2;
  c.u = k[0] * (c.q0 / c.q2) + k[2];                         // correctly rounded divisions: no fast-math in this build
  c.v = k[4] * (c.q1 / c.q2) + k[5];
  return c;
}

// |a - b|^2 in fp32, (d0 d0 + d1 d1) + d2 d2 with every operation rounded once (contraction off, as in to_camera)
__device__ __forceinline__ float sq_dist3(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
  const float d0 = ax - bx, d1 = ay - by, d2 = az - bz;
  return (d0 * d0 + d1 * d1) + d2 * d2;
}

// bits(d) << 32 | index: for d >= 0 (no NaN) bit order is value order, so the minimum key is the smallest d, the lowest index
// among equals
__device__ __forceinline__ unsigned long long dist_key(float d, uint32_t index) {
  return ((unsigned long long)__float_as_uint(d) << 32) | index;
}

// ------------------------------------------------------------------------------------------------------- bounding box
__device__ __forceinline__ uint32_t float_ord(float x) {    // order-preserving map of the finite floats onto unsigned integers
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float float_unord(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// Grid-stride over n points: per-axis minimum and maximum (as float_ord) and the number of the points that take part
// (load_eligible), into b = {lo[3], hi[3], count}, which starts as {~0 x 3, 0 x 4}.  One butterfly per wave, then seven integer
// atomics per wave that saw a point: order-free.
__device__ __forceinline__ void bounds_accumulate(const float* __restrict__ points, const uint8_t* __restrict__ mask, long n, uint32_t* b) {
  uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  int cnt = 0;
  for (long p = (long)blockIdx.x * PC_THREADS + threadIdx.x; p < n; p += (long)gridDim.x * PC_THREADS) {
    float c[3];
    if (!load_eligible(points, mask, p, c[0], c[1], c[2])) continue;
    ++cnt;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const uint32_t u = float_ord(c[k]);
      lo[k] = min(lo[k], u);
      hi[k] = max(hi[k], u);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o, 64);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      lo[k] = min(lo[k], (uint32_t)__shfl_xor((int)lo[k], o, 64));
      hi[k] = max(hi[k], (uint32_t)__shfl_xor((int)hi[k], o, 64));
    }
  }
  if ((threadIdx.x & 63) == 0 && cnt) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      atomicMin(&b[k], lo[k]);
      atomicMax(&b[3 + k], hi[k]);
    }
    atomicAdd(&b[6], (uint32_t)cnt);
  }
}

// ------------------------------------------------------------------------------------------------------- workgroup primitives
// All of them: PC_THREADS threads, sh = PC_WAVES ints of LDS, called by every thread of the workgroup.

// The workgroup's sum of one int per thread, for thread 0 to write out (every thread gets it).  There is no barrier in front: a
// second call in one kernel needs its own sh, or a __syncthreads() between the two.
__device__ __forceinline__ int block_sum(int c, int* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}
static_assert(PC_WAVES == 4, "block_sum adds four waves");

__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}
// inclusive scan over the workgroup's values; `total` is their sum
__device__ __forceinline__ int block_incl_scan(int v, int* sh, int& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  v = wave_incl_scan(v, lane);
  __syncthreads();                                           // sh may still be read from an earlier call
  if (lane == 63) sh[wv] = v;
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < PC_WAVES; ++w) {
    if (w < wv) before += sh[w];
    total += sh[w];
  }
  return v + before;
}

// One workgroup: off[b] = the sum of cnt before b, for b in [0, nb), PC_THREADS entries per pass with the running sum carried
// over; returns the sum of all.  off == cnt is allowed (a thread reads its entry before it writes it).
__device__ __forceinline__ int block_offset_scan(const int* cnt, int* off, long nb, int* sh) {
  int carry = 0;
  for (long b0 = 0; b0 < nb; b0 += PC_THREADS) {
    const long b = b0 + threadIdx.x;
    const int c = b < nb ? cnt[b] : 0;
    int total;
    const int incl = block_incl_scan(c, sh, total);
    if (b < nb) off[b] = carry + incl - c;
    carry += total;
  }
  return carry;
}

// The workgroup's packed records, staged in LDS at the byte offset `mis` that their output range has inside a dword (mis =
// (rec + byte0) & 3), so that aligned dwords of LDS are aligned dwords of the output: stage[mis, mis + nbytes) goes to
// rec[byte0, byte0 + nbytes) as head bytes, dwords, tail bytes.  The caller clips nbytes to its capacity and has synchronised.
__device__ __forceinline__ void staged_flush(const uint8_t* stage, uint8_t* rec, long byte0, int mis, int nbytes) {
  const int tid = threadIdx.x;
  const int lo = mis, hi = mis + nbytes;                     // stage bytes [lo, hi) go to out[lo, hi), out 4-byte aligned
  uint8_t* out = rec + byte0 - mis;
  const int dlo = (lo + 3) & ~3, dhi = hi & ~3;
  if (dlo <= dhi) {
    if (tid < dlo - lo) out[lo + tid] = stage[lo + tid];
    for (int d = dlo + 4 * tid; d < dhi; d += 4 * PC_THREADS)
      *reinterpret_cast<uint32_t*>(out + d) = *reinterpret_cast<const uint32_t*>(stage + d);
    if (tid < hi - dhi) out[dhi + tid] = stage[dhi + tid];
  } else {                                                   // fewer than 4 bytes inside one dword: with records of 4 bytes or more, none
    if (tid < hi - lo) out[lo + tid] = stage[lo + tid];
  }
}

// ------------------------------------------------------------------------------------------------------- entry-point checks
inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }   // NULL is aligned

// what every [N,H,W] entry point refuses: an empty extent, or more than 2^31 - 1 pixels (flat pixel indices and counts are int32)
inline bool bad_nhw(int N, int H, int W) { return N <= 0 || H <= 0 || W <= 0 || (int64_t)N * H * W > 0x7fffffffLL; }
