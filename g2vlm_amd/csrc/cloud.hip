// Point-cloud export on the device (g2vlm_utils.save_point_cloud / point_cloud_mask / estimate_intrinsics): what follows
// `recon` - fp32 pointmaps [N,H,W,3], fp32 images [N,3,H,W] and, from a train_conf_pi3 checkpoint, confidence logits [N,H,W].
//
//   g2v_cloud_mask      keep mask u8 [N,H,W]: finite world point, confidence logit above a threshold, not a depth edge
//                       (the reference's depth_edge, modeling/pi3/utils/geometry.py:339, 3x3 window, no mask).
//   g2v_cloud_compact   the kept pixels as packed 15-byte PLY records (<f4 x,y,z, u1 r,g,b) in view-major, row-major order
//                       (numpy boolean indexing's), and the kept count of every view.  Three launches: count per block of
//                       CC_BLOCK pixels, one workgroup's scan of the block counts, scatter.  Positions are integer prefix sums:
//                       the bytes do not depend on the order in which anything ran.
//   g2v_intrinsics_lsq  per view the pinhole fit u = fx X/Z + cx, v = fy Y/Z + cy over the kept pixels with Z > 0, normal
//                       equations in fp64, reduced thread -> wave -> workgroup -> a second launch in a fixed order (no atomics).
//
// All three are memory-bound.  The [...,3] fp32 layout has a 12-byte stride: it is read as 16-byte vectors over the flat dword
// stream (4 pixels = 3 vectors) wherever the address allows, and the components are picked out of the vectors.
#include <float.h>

#include "cloud_common.h"                                   // cc_colour, finite_f, the compaction's scan / count / flush, the checks
#include "common.h"
#include "g2vlm_hip.h"

namespace {

__device__ __forceinline__ bool nan_bits(uint32_t b) { return (b & 0x7fffffffu) > 0x7f800000u; }

// ------------------------------------------------------------------------------------------------------------- mask
constexpr int CM_TW = 128, CM_TH = 16, CM_THREADS = 256;   // a workgroup's tile of one view; (CM_TH + 2) x (CM_TW + 2) depths in LDS

// The dwords [d0, d1) of a [..,3] fp32 array of `total` dwords, 16 bytes at a time where the array's base allows it (the vectors
// are the ALIGNED ones that cover the span, clipped to the array, so that no load reaches outside it); f(dword index, bits) is
// called for every dword of the span exactly once.
template <class F>
__device__ __forceinline__ void cm_span(const uint32_t* a, bool vec, long total, long d0, long d1, int tid, F f) {
  const long v0 = d0 >> 2, v1 = (d1 + 3) >> 2;
  for (long v = v0 + tid; v < v1; v += CM_THREADS) {
    const long e = v << 2;
    if (vec && e + 4 <= total) {
      const u32x4 w = *reinterpret_cast<const u32x4*>(a + e);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e + k >= d0 && e + k < d1) f(e + k, w[k]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e + k >= d0 && e + k < d1) f(e + k, a[e + k]);
    }
  }
}

// grid (ceil(W / CM_TW), ceil(H / CM_TH), N)
__global__ __launch_bounds__(CM_THREADS) void cloud_mask_kernel(const uint32_t* points, const uint32_t* local, const float* conf,
                                                                 uint8_t* mask, int H, int W, int flags, float conf_min,
                                                                 float atol, float rtol, int pvec, int lvec) {
  __shared__ float z[CM_TH + 2][CM_TW + 2];                  // z[i][j]: depth of (r0 - 1 + i, c0 - 1 + j), in-bounds cells only
  __shared__ uint8_t bad[CM_TH][CM_TW];                      // a world coordinate of the pixel is not finite
  const int tid = threadIdx.x;
  const int c0 = blockIdx.x * CM_TW, r0 = blockIdx.y * CM_TH;
  const long view = (long)blockIdx.z * H * W;
  const long total = (long)gridDim.z * H * W * 3;
  const int rows = min(CM_TH, H - r0), cols = min(CM_TW, W - c0);
  const bool edge_on = (flags & (G2V_CLOUD_EDGE_ATOL | G2V_CLOUD_EDGE_RTOL)) != 0;

  if (flags & G2V_CLOUD_FINITE) {
    for (int i = tid; i < CM_TH * CM_TW; i += CM_THREADS) (&bad[0][0])[i] = 0;
    __syncthreads();
    for (int i = 0; i < rows; ++i) {
      const long p0 = view + (long)(r0 + i) * W + c0;
      // racing lanes all store the same 1
      cm_span(points, pvec != 0, total, p0 * 3, (p0 + cols) * 3, tid, [&](long d, uint32_t b) {
        if (!finite_f(__uint_as_float(b))) bad[i][(int)(d / 3 - p0)] = 1;
      });
    }
  }
  if (edge_on) {
    const int ca = max(c0 - 1, 0), cb = min(c0 + cols + 1, W);         // columns [ca, cb) of rows [ra, rb): the halo stays in the view
    const int ra = max(r0 - 1, 0), rb = min(r0 + rows + 1, H);
    for (int r = ra; r < rb; ++r) {
      const long p0 = view + (long)r * W + ca;
      cm_span(local, lvec != 0, total, p0 * 3, (p0 + (cb - ca)) * 3, tid, [&](long d, uint32_t b) {
        const long p = d / 3;
        if (d - p * 3 == 2) z[r - r0 + 1][(int)(p - p0) + ca - c0 + 1] = __uint_as_float(b);
      });
    }
  }
  __syncthreads();

  for (int i = tid; i < rows * CM_TW; i += CM_THREADS) {
    const int ty = i / CM_TW, tx = i % CM_TW;
    if (tx >= cols) continue;
    const int r = r0 + ty, c = c0 + tx;
    const long p = view + (long)r * W + c;
    bool keep = true;
    if (flags & G2V_CLOUD_FINITE) keep = bad[ty][tx] == 0;
    if (flags & G2V_CLOUD_CONF) keep = keep && (conf[p] > conf_min);   // a NaN logit fails
    if (edge_on) {
      bool has_nan = false;
      float mx = -INFINITY, mn = -INFINITY;
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          if (r + dy < 0 || r + dy >= H || c + dx < 0 || c + dx >= W) continue;
          const float v = z[ty + 1 + dy][tx + 1 + dx];
          has_nan |= nan_bits(__float_as_uint(v));
          mx = fmaxf(mx, v);
          mn = fmaxf(mn, -v);
        }
      }
      if (!has_nan) {                                        // max_pool2d hands a NaN on: diff is NaN, no comparison holds
        const float diff = mx + mn;                          // may itself be NaN (+inf + -inf): then neither test holds
        bool edge = false;
        if (flags & G2V_CLOUD_EDGE_ATOL) edge = diff > atol;
        if (flags & G2V_CLOUD_EDGE_RTOL) {
          float q = diff / z[ty + 1][tx + 1];                // correctly rounded: no fast-math in this build
          if (q != q) q = 0.f;                               // nan_to_num
          else if (q == INFINITY) q = FLT_MAX;
          else if (q == -INFINITY) q = -FLT_MAX;
          edge = edge || q > rtol;
        }
        keep = keep && !edge;
      }
    }
    mask[p] = keep ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------------------------------------- compaction
constexpr int CC_THREADS = 256, CC_PER = 4, CC_BLOCK = CC_THREADS * CC_PER;   // pixels of one view per workgroup
constexpr int CC_REC = 15;
static_assert(CC_THREADS == PC_THREADS, "cloud_common.h's scan, count and flush are written for this workgroup");

// the mask bytes of pixels [i, i + 4) of a view of hw pixels (pixels >= hw: 0), one dword where the address allows it
__device__ __forceinline__ uint32_t cc_mask4(const uint8_t* m, long i, long hw) {
  if (i + 4 <= hw && (reinterpret_cast<uintptr_t>(m + i) & 3) == 0) return *reinterpret_cast<const uint32_t*>(m + i);
  uint32_t w = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (i + k < hw) w |= (uint32_t)m[i + k] << (8 * k);
  return w;
}
__device__ __forceinline__ int cc_kept(uint32_t w, int k) { return ((w >> (8 * k)) & 0xffu) != 0; }
__device__ __forceinline__ int cc_count4(uint32_t w) { return cc_kept(w, 0) + cc_kept(w, 1) + cc_kept(w, 2) + cc_kept(w, 3); }

// grid (blocks per view, N): kept pixels of the workgroup's CC_BLOCK pixels
__global__ __launch_bounds__(CC_THREADS) void cloud_count_kernel(const uint8_t* mask, long hw, int* block_cnt) {
  __shared__ int sh[CC_THREADS / 64];
  const uint8_t* m = mask + (long)blockIdx.y * hw;
  const long i = (long)blockIdx.x * CC_BLOCK + threadIdx.x * CC_PER;
  const int kept = block_sum(cc_count4(cc_mask4(m, i, hw)), sh);
  if (threadIdx.x == 0) block_cnt[(long)blockIdx.y * gridDim.x + blockIdx.x] = kept;
}

// one workgroup: block_off[b] = kept pixels before block b (block_offset_scan), counts[n] = kept pixels of view n.
// The total is at most N H W <= 2^31 - 1.
__global__ __launch_bounds__(CC_THREADS) void cloud_scan_kernel(const int* block_cnt, int* block_off, int* counts, int N, int bpv) {
  __shared__ int sh[CC_THREADS / 64];
  block_offset_scan(block_cnt, block_off, (long)N * bpv, sh);
  for (int n = threadIdx.x; n < N; n += CC_THREADS) {
    int s = 0;
    for (int j = 0; j < bpv; ++j) s += block_cnt[(long)n * bpv + j];
    counts[n] = s;
  }
}

// grid (blocks per view, N).  The workgroup's records are staged in LDS at the byte offset its output range has inside a dword
// and written out by staged_flush.
__global__ __launch_bounds__(CC_THREADS) void cloud_scatter_kernel(const float* points, const float* colors, const uint8_t* mask,
                                                                    const int* block_off, uint8_t* rec, long max_records, long hw,
                                                                    int pvec, int cvec) {
  __shared__ int sh[CC_THREADS / 64];
  __shared__ __attribute__((aligned(16))) uint8_t stage[CC_BLOCK * CC_REC + 16];
  const int tid = threadIdx.x, n = blockIdx.y;
  const long i = (long)blockIdx.x * CC_BLOCK + tid * CC_PER;  // first of the thread's pixels inside the view
  const uint32_t w = cc_mask4(mask + (long)n * hw, i, hw);
  const int c = cc_count4(w);
  int kept;
  const int before = block_incl_scan(c, sh, kept) - c;
  if (kept == 0) return;
  const long first = block_off[(long)n * gridDim.x + blockIdx.x];       // record index of the workgroup's first record
  const long byte0 = first * CC_REC;
  const int mis = (int)((reinterpret_cast<uintptr_t>(rec) + byte0) & 3);

  if (c) {
    float xyz[CC_PER * 3], rgb[3][CC_PER];
    const long p = (long)n * hw + i;                         // flat pixel
    const float* ps = points + p * 3;
    if (pvec && i + CC_PER <= hw && (p & 3) == 0) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(ps + 4 * k);
        xyz[4 * k] = v[0]; xyz[4 * k + 1] = v[1]; xyz[4 * k + 2] = v[2]; xyz[4 * k + 3] = v[3];
      }
    } else {
#pragma unroll
      for (int k = 0; k < CC_PER * 3; ++k) xyz[k] = (i + k / 3 < hw) ? ps[k] : 0.f;
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const long q = ((long)n * 3 + ch) * hw + i;
      if (cvec && i + CC_PER <= hw && (q & 3) == 0) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(colors + q);
        rgb[ch][0] = v[0]; rgb[ch][1] = v[1]; rgb[ch][2] = v[2]; rgb[ch][3] = v[3];
      } else {
#pragma unroll
        for (int k = 0; k < CC_PER; ++k) rgb[ch][k] = (i + k < hw) ? colors[q + k] : 0.f;
      }
    }
    int slot = before;
#pragma unroll
    for (int k = 0; k < CC_PER; ++k) {
      if (!cc_kept(w, k)) continue;
      uint8_t* s = stage + mis + slot * CC_REC;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const uint32_t b = __float_as_uint(xyz[3 * k + j]);
        s[4 * j] = (uint8_t)b; s[4 * j + 1] = (uint8_t)(b >> 8); s[4 * j + 2] = (uint8_t)(b >> 16); s[4 * j + 3] = (uint8_t)(b >> 24);
      }
      s[12] = cc_colour(rgb[0][k]); s[13] = cc_colour(rgb[1][k]); s[14] = cc_colour(rgb[2][k]);
      ++slot;
    }
  }
  __syncthreads();

  long nrec = kept;                                          // records past the caller's capacity are not written
  if (first + nrec > max_records) nrec = max_records > first ? max_records - first : 0;
  staged_flush(stage, rec, byte0, mis, (int)nrec * CC_REC);
}

inline int cc_blocks_per_view(int H, int W) { return (int)(((long)H * W + CC_BLOCK - 1) / CC_BLOCK); }

// ---------------------------------------------------------------------------------------------------------- intrinsics
constexpr int CI_THREADS = 256, CI_MAX_BLOCKS = 64, CI_SUMS = 9;   // n, Sa, Saa, Su, Sau, Sb, Sbb, Sv, Sbv

inline int ci_blocks_per_view(int H, int W) {
  const long groups = ((long)H * W + 3) / 4;
  const long b = (groups + CI_THREADS - 1) / CI_THREADS;
  return (int)(b < CI_MAX_BLOCKS ? b : CI_MAX_BLOCKS);
}

__device__ __forceinline__ double wave_sum_f64(double v) {   // a fixed butterfly: the same bits on every run
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// grid (blocks per view, N): partial sums of the view's usable pixels, u and v taken about the image centre
__global__ __launch_bounds__(CI_THREADS) void cloud_intrinsics_partial_kernel(const float* local, const uint8_t* mask, int H, int W,
                                                                               double* part, int lvec) {
  __shared__ double sh[CI_THREADS / 64][CI_SUMS];
  const int tid = threadIdx.x, n = blockIdx.y;
  const long hw = (long)H * W;
  const double uc = 0.5 - 0.5 * W, vc = 0.5 - 0.5 * H;
  double s[CI_SUMS];
#pragma unroll
  for (int k = 0; k < CI_SUMS; ++k) s[k] = 0.0;
  for (long i = ((long)blockIdx.x * CI_THREADS + tid) * 4; i < hw; i += (long)gridDim.x * CI_THREADS * 4) {
    const uint32_t mw = mask ? cc_mask4(mask + (long)n * hw, i, hw) : 0x01010101u;
    if (mw == 0) continue;
    float xyz[12];
    const long p = (long)n * hw + i;
    const float* ps = local + p * 3;
    if (lvec && i + 4 <= hw && (p & 3) == 0) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(ps + 4 * k);
        xyz[4 * k] = v[0]; xyz[4 * k + 1] = v[1]; xyz[4 * k + 2] = v[2]; xyz[4 * k + 3] = v[3];
      }
    } else {
#pragma unroll
      for (int k = 0; k < 12; ++k) xyz[k] = (i + k / 3 < hw) ? ps[k] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float X = xyz[3 * k], Y = xyz[3 * k + 1], Z = xyz[3 * k + 2];
      const bool ok = i + k < hw && cc_kept(mw, k) && finite_f(X) && finite_f(Y) && finite_f(Z) && Z > 0.f;
      if (!ok) continue;
      const long pix = i + k;
      const int y = (int)(pix / W), x = (int)(pix - (long)y * W);
      const double a = (double)X / (double)Z, b = (double)Y / (double)Z, u = x + uc, v = y + vc;
      s[0] += 1.0; s[1] += a; s[2] += a * a; s[3] += u; s[4] += a * u;
      s[5] += b; s[6] += b * b; s[7] += v; s[8] += b * v;
    }
  }
#pragma unroll
  for (int k = 0; k < CI_SUMS; ++k) {
    const double r = wave_sum_f64(s[k]);
    if ((tid & 63) == 0) sh[tid >> 6][k] = r;
  }
  __syncthreads();
  if (tid < CI_SUMS) part[((long)n * gridDim.x + blockIdx.x) * CI_SUMS + tid] = ((sh[0][tid] + sh[1][tid]) + sh[2][tid]) + sh[3][tid];
}

// one wave per view: lane b takes workgroup b's partial sums (bpv <= 64), the butterfly adds them, lane 0 solves
__global__ __launch_bounds__(64) void cloud_intrinsics_solve_kernel(const double* part, int bpv, int H, int W, float* K, int* used) {
  const int n = blockIdx.x, lane = threadIdx.x;
  double s[CI_SUMS];
#pragma unroll
  for (int k = 0; k < CI_SUMS; ++k) s[k] = wave_sum_f64(lane < bpv ? part[((long)n * bpv + lane) * CI_SUMS + k] : 0.0);
  if (lane != 0) return;
  const double cnt = s[0];
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  double fx = nan, cx = nan, fy = nan, cy = nan;
  if (cnt >= 2.0) {
    // n Saa - Sa^2 = n^2 var(a) >= 0; at or below the rounding of its two terms the ratios do not vary: no fit
    const double da = cnt * s[2] - s[1] * s[1], db = cnt * s[6] - s[5] * s[5];
    if (da > 1e-10 * cnt * s[2]) {
      fx = (cnt * s[4] - s[1] * s[3]) / da;
      cx = (s[3] - fx * s[1]) / cnt + 0.5 * W;
    }
    if (db > 1e-10 * cnt * s[6]) {
      fy = (cnt * s[8] - s[5] * s[7]) / db;
      cy = (s[7] - fy * s[5]) / cnt + 0.5 * H;
    }
  }
  float* k = K + (long)n * 9;
  k[0] = (float)fx; k[1] = 0.f; k[2] = (float)cx;
  k[3] = 0.f; k[4] = (float)fy; k[5] = (float)cy;
  k[6] = 0.f; k[7] = 0.f; k[8] = 1.f;
  used[n] = (int)cnt;
}

}  // namespace

extern "C" int g2v_cloud_mask(const void* points, const void* local, const void* conf, int N, int H, int W, int flags, float conf_logit_min,
                              float edge_atol, float edge_rtol, void* mask, void* stream) {
  const int all = G2V_CLOUD_FINITE | G2V_CLOUD_CONF | G2V_CLOUD_EDGE_ATOL | G2V_CLOUD_EDGE_RTOL;
  if (bad_nhw(N, H, W) || (flags & ~all) || !mask) return G2V_ERR_ARG;
  const bool edge = (flags & (G2V_CLOUD_EDGE_ATOL | G2V_CLOUD_EDGE_RTOL)) != 0;
  if (((flags & G2V_CLOUD_FINITE) && !points) || ((flags & G2V_CLOUD_CONF) && !conf) || (edge && !local)) return G2V_ERR_ARG;
  if ((points && !aligned(points, 4)) || (local && !aligned(local, 4)) || (conf && !aligned(conf, 4))) return G2V_ERR_ARG;
  const dim3 grid((unsigned)((W + CM_TW - 1) / CM_TW), (unsigned)((H + CM_TH - 1) / CM_TH), (unsigned)N);
  if (grid.y > 65535u || grid.z > 65535u) return G2V_ERR_ARG;
  hipLaunchKernelGGL(cloud_mask_kernel, grid, dim3(CM_THREADS), 0, (hipStream_t)stream, (const uint32_t*)points, (const uint32_t*)local,
                     (const float*)conf, (uint8_t*)mask, H, W, flags, conf_logit_min, edge_atol, edge_rtol, aligned(points, 16),
                     aligned(local, 16));
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

extern "C" int64_t g2v_cloud_compact_workspace(int N, int H, int W) {
  if (bad_nhw(N, H, W)) return 0;
  return 8 * (int64_t)N * cc_blocks_per_view(H, W);
}

extern "C" int g2v_cloud_compact(const void* points, const void* colors, const void* mask, int N, int H, int W, void* records,
                                 int64_t max_records, void* counts, void* workspace, int64_t workspace_bytes, void* stream) {
  if (bad_nhw(N, H, W) || !points || !colors || !mask || !counts || !workspace || max_records < 0 || (max_records > 0 && !records))
    return G2V_ERR_ARG;
  if (workspace_bytes < g2v_cloud_compact_workspace(N, H, W) || !aligned(points, 4) || !aligned(colors, 4) || !aligned(workspace, 4) ||
      !aligned(counts, 4))
    return G2V_ERR_ARG;
  const int bpv = cc_blocks_per_view(H, W);
  if (N > 65535) return G2V_ERR_ARG;
  const long hw = (long)H * W;
  int* block_cnt = (int*)workspace;
  int* block_off = block_cnt + (long)N * bpv;
  const dim3 grid((unsigned)bpv, (unsigned)N);
  hipLaunchKernelGGL(cloud_count_kernel, grid, dim3(CC_THREADS), 0, (hipStream_t)stream, (const uint8_t*)mask, hw, block_cnt);
  G2V_CHECK_LAUNCH();
  hipLaunchKernelGGL(cloud_scan_kernel, dim3(1), dim3(CC_THREADS), 0, (hipStream_t)stream, block_cnt, block_off, (int*)counts, N, bpv);
  G2V_CHECK_LAUNCH();
  if (max_records > 0) {
    hipLaunchKernelGGL(cloud_scatter_kernel, grid, dim3(CC_THREADS), 0, (hipStream_t)stream, (const float*)points, (const float*)colors,
                       (const uint8_t*)mask, block_off, (uint8_t*)records, (long)max_records, hw, aligned(points, 16), aligned(colors, 16));
    G2V_CHECK_LAUNCH();
  }
  return G2V_OK;
}

extern "C" int64_t g2v_intrinsics_lsq_workspace(int N, int H, int W) {
  if (bad_nhw(N, H, W)) return 0;
  return 8 * (int64_t)CI_SUMS * N * ci_blocks_per_view(H, W);
}

extern "C" int g2v_intrinsics_lsq(const void* local, const void* mask, int N, int H, int W, void* K, void* used, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
  if (bad_nhw(N, H, W) || !local || !K || !used || !workspace || N > 65535) return G2V_ERR_ARG;
  if (workspace_bytes < g2v_intrinsics_lsq_workspace(N, H, W) || !aligned(local, 4) || !aligned(K, 4) || !aligned(used, 4) ||
      !aligned(workspace, 8))
    return G2V_ERR_ARG;
  const int bpv = ci_blocks_per_view(H, W);
  hipLaunchKernelGGL(cloud_intrinsics_partial_kernel, dim3((unsigned)bpv, (unsigned)N), dim3(CI_THREADS), 0, (hipStream_t)stream,
                     (const float*)local, (const uint8_t*)mask, H, W, (double*)workspace, aligned(local, 16));
  G2V_CHECK_LAUNCH();
  hipLaunchKernelGGL(cloud_intrinsics_solve_kernel, dim3((unsigned)N), dim3(64), 0, (hipStream_t)stream, (const double*)workspace, bpv, H, W,
                     (float*)K, (int*)used);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}
