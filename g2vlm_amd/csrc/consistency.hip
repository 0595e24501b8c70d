// Multi-view consistency of the exported cloud (g2vlm_utils.multiview_consistency / point_cloud_mask(min_views=...)): does any
// other view see this point?  Inputs are recon's outputs for one batch entry - points / local fp32 [N,H,W,3], camera-to-world
// poses fp32 [N,4,4] - and a pinhole K fp32 [N,3,3] per view (g2v_intrinsics_lsq's).
//
// The rule (include/g2vlm_hip.h and DESIGN.md 6k state it in full): the world point P of a source pixel (i, p) is taken into
// every other view j, q = R_j^T (P - t_j), u = fx q0/q2 + cx, v = fy q1/q2 + cy, and compared with the depth zt that j predicts
// at the pixel (floor u, floor v): it agrees if |q2 - zt| <= rtol zt and lies in front if q2 - zt < -rtol zt.  Every operation
// is an fp32 operation rounded once - contraction is switched off in cloud_common.h's to_camera, which render.hip projects with
// too, and in project() - so that a numpy restatement gives the same bytes.
//
//   consistency_plane_kernel   the depth plane fp32 [N,H,W] in the workspace: local z where the mask keeps the pixel and z is
//                              finite and > 0, NaN elsewhere (a NaN fails both compares, so the inner loop needs no validity
//                              test: one 4-byte gather per projection instead of a 12-byte point and a mask byte).  Zeroes pairs.
//   consistency_kernel         one thread per source pixel, a workgroup per 2-D tile of one view (its footprint in a target view
//                              is then compact), counts in registers, j walked in the same order by every workgroup so that
//                              the chip reads one target's plane at a time.  The sixteen constants of a view are wave-uniform
//                              loads.  pairs: ballot + popcount per wave, summed over the workgroup in LDS, one integer
//                              atomicAdd per workgroup and (i, j, class) that is not zero; integer sums do not depend on order.
#include "cloud_common.h"                                   // load_eligible, to_camera, finite_f, the entry point's checks
#include "common.h"
#include "g2vlm_hip.h"

#ifndef G2V_CONSISTENCY_TILE_W
#define G2V_CONSISTENCY_TILE_W 32           // A/B builds only (tools/bench_consistency.py): 32 x 8 against 16 x 16
#endif
#ifndef G2V_CONSISTENCY_TILE_H
#define G2V_CONSISTENCY_TILE_H 8
#endif

namespace {

constexpr int CS_TW = G2V_CONSISTENCY_TILE_W, CS_TH = G2V_CONSISTENCY_TILE_H, CS_THREADS = CS_TW * CS_TH;
constexpr int CS_MAX_VIEWS = 256, CP_THREADS = 256, CP_MAX_BLOCKS = 4096;
static_assert(CS_THREADS == 256 && (CS_TW & (CS_TW - 1)) == 0, "a tile is 256 pixels, its width a power of two");

// grid-stride over the N H W pixels and over the 2 N N pair counts
__global__ __launch_bounds__(CP_THREADS) void consistency_plane_kernel(const float* local, const uint8_t* mask, float* plane, long total,
                                                                        int* pairs, int npairs) {
  const long stride = (long)gridDim.x * CP_THREADS;
  const long first = (long)blockIdx.x * CP_THREADS + threadIdx.x;
  for (long p = first; p < total; p += stride) {
    const float z = local[p * 3 + 2];
    const bool keep = (!mask || mask[p] != 0) && finite_f(z) && z > 0.f;
    plane[p] = keep ? z : __uint_as_float(0x7fc00000u);
  }
  if (pairs)
    for (long k = first; k < npairs; k += stride) pairs[k] = 0;
}

struct Cls { bool agree, front; };

// One source point against one target view: to_camera, then the depth the view predicts at the pixel the point lands on.
// Contraction off: every * and - below is its own rounding.
__device__ __forceinline__ Cls project(float px, float py, float pz, const float* __restrict__ pose, const float* __restrict__ k,
                                       const float* __restrict__ plane, int H, int W, float rtol) {
#pragma clang fp contract(off)
  const CamPoint c = to_camera(px, py, pz, pose, k);
  Cls r = {false, false};
  if (c.q2 > 0.f && c.u >= 0.f && c.u < (float)W && c.v >= 0.f && c.v < (float)H) {   // false on NaN; only inside is u or v converted
    const int x = (int)c.u, y = (int)c.v;                    // 0 <= x < W, 0 <= y < H
    const float zt = plane[(long)y * W + x];                 // finite and > 0, or NaN
    const float tol = rtol * zt, diff = c.q2 - zt;
    r.agree = fabsf(diff) <= tol;
    r.front = diff < -tol;
  }
  return r;
}

// grid (ceil(W / CS_TW), ceil(H / CS_TH), N)
__global__ __launch_bounds__(CS_THREADS) void consistency_kernel(const float* __restrict__ points, const uint8_t* __restrict__ mask,
                                                                  const float* __restrict__ poses, const float* __restrict__ K,
                                                                  const float* __restrict__ plane, int N, int H, int W, float rtol,
                                                                  int min_agree, int max_in_front, uint8_t* agree, uint8_t* in_front,
                                                                  int* pairs, uint8_t* mask_out) {
  __shared__ int sh_pairs[CS_MAX_VIEWS * 2];
  const int tid = threadIdx.x, i = blockIdx.z;
  const int x = blockIdx.x * CS_TW + (tid & (CS_TW - 1)), y = blockIdx.y * CS_TH + tid / CS_TW;
  const bool live = x < W && y < H;
  const long hw = (long)H * W;
  const long p = (long)i * hw + (long)y * W + x;
  float px = 0.f, py = 0.f, pz = 0.f;
  bool eligible = false;
  if (live) eligible = load_eligible(points, mask, p, px, py, pz);
  if (pairs) {
    for (int k = tid; k < 2 * N; k += CS_THREADS) sh_pairs[k] = 0;
    __syncthreads();
  }
  int na = 0, nf = 0;
  if (__ballot(eligible) != 0) {                             // a wave without an eligible pixel has nothing to project
    for (int j = 0; j < N; ++j) {
      if (j == i) continue;
      Cls c = {false, false};
      if (eligible) c = project(px, py, pz, poses + j * 16, K + j * 9, plane + (long)j * hw, H, W, rtol);
      na += c.agree;
      nf += c.front;
      if (pairs) {
        const int ca = __popcll(__ballot(c.agree)), cf = __popcll(__ballot(c.front));
        if ((tid & 63) == 0) {
          if (ca) atomicAdd(&sh_pairs[2 * j], ca);
          if (cf) atomicAdd(&sh_pairs[2 * j + 1], cf);
        }
      }
    }
  }
  if (live) {
    if (agree) agree[p] = (uint8_t)na;
    if (in_front) in_front[p] = (uint8_t)nf;
    if (mask_out) mask_out[p] = (eligible && na >= min_agree && (max_in_front < 0 || nf <= max_in_front)) ? 1 : 0;
  }
  if (pairs) {
    __syncthreads();
    for (int k = tid; k < 2 * N; k += CS_THREADS) {
      const int c = sh_pairs[k];
      if (c) atomicAdd(&pairs[(long)i * N * 2 + k], c);
    }
  }
}

// the tile rows of a view are the grid's y extent, which ends at 65535: H <= 65535 CS_TH
inline bool bad_shape(int N, int H, int W) { return bad_nhw(N, H, W) || N > CS_MAX_VIEWS || H > 65535 * CS_TH; }

}  // namespace

extern "C" int64_t g2v_cloud_consistency_workspace(int N, int H, int W) {
  if (bad_shape(N, H, W)) return 0;
  return 4 * (int64_t)N * H * W;
}

extern "C" int g2v_cloud_consistency(const void* points, const void* local, const void* mask, const void* poses, const void* K,
                                     int N, int H, int W, float depth_rtol, int min_agree, int max_in_front,
                                     void* agree, void* in_front, void* pairs, void* mask_out,
                                     void* workspace, int64_t workspace_bytes, void* stream) {
  if (bad_shape(N, H, W) || !points || !local || !poses || !K || !workspace) return G2V_ERR_ARG;
  if (!(depth_rtol >= 0.f)) return G2V_ERR_ARG;              // negative or NaN
  if (!agree && !in_front && !pairs && !mask_out) return G2V_ERR_ARG;
  if (workspace_bytes < g2v_cloud_consistency_workspace(N, H, W) || !aligned(points, 4) || !aligned(local, 4) || !aligned(poses, 4) ||
      !aligned(K, 4) || !aligned(workspace, 4) || !aligned(pairs, 4))
    return G2V_ERR_ARG;
  const dim3 grid((unsigned)((W + CS_TW - 1) / CS_TW), (unsigned)((H + CS_TH - 1) / CS_TH), (unsigned)N);
  const long total = (long)N * H * W;
  const long blocks = (total + CP_THREADS - 1) / CP_THREADS;
  hipLaunchKernelGGL(consistency_plane_kernel, dim3((unsigned)(blocks < CP_MAX_BLOCKS ? blocks : CP_MAX_BLOCKS)), dim3(CP_THREADS), 0,
                     (hipStream_t)stream, (const float*)local, (const uint8_t*)mask, (float*)workspace, total, (int*)pairs, 2 * N * N);
  G2V_CHECK_LAUNCH();
  hipLaunchKernelGGL(consistency_kernel, grid, dim3(CS_THREADS), 0, (hipStream_t)stream, (const float*)points, (const uint8_t*)mask,
                     (const float*)poses, (const float*)K, (const float*)workspace, N, H, W, depth_rtol, min_agree, max_in_front,
                     (uint8_t*)agree, (uint8_t*)in_front, (int*)pairs, (uint8_t*)mask_out);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}
