// Novel-view rendering of the exported cloud (g2vlm_utils.render_point_cloud): every kept pixel's world point is projected into M
// target cameras and every target pixel keeps the nearest point that covers it - a z-buffer.  Inputs are recon's outputs for one
// batch entry - points fp32 [N,H,W,3], images fp32 [N,3,H,W], a keep mask - and the targets' camera-to-world poses fp32 [M,4,4]
// and pinhole K fp32 [M,3,3]; outputs are a colour image, a depth map and the flat index of the source pixel, per target.
//
// The rule (include/g2vlm_hip.h and DESIGN.md 6l state it in full): q = R_m^T (P - t_m), u = fx q0/q2 + cx, v = fy q1/q2 + cy by
// cloud_common.h's to_camera, as in consistency.hip - fp32, every operation rounded once, contraction switched off - and the point
// lands on the pixel ((int)u, (int)v) and on the (2 r + 1)^2 pixels around it, clipped.  A target pixel keeps the MINIMUM of the
// 64-bit keys (bits of q2 << 32 | source index: dist_key) of the points that cover it: for positive finite floats bit order is value order, so that is
// the nearest point, the lower source index among equals; the keys are distinct and the minimum is associative, so the bytes do
// not depend on the order in which anything ran.  tests/render_check.py restates the rule in numpy.
//
//   render_fill_kernel      all-ones into the M OH OW keys of the workspace (above every key a point can have)
//   render_splat_kernel     one thread per source pixel, a workgroup per 32 x 8 tile of one view (its footprint in a target is
//                           then compact), the targets walked in the same order by every workgroup so that the chip works on one
//                           target's key plane at a time; the sixteen constants of a target are wave-uniform loads.  Per covered
//                           target pixel one 64-bit atomic minimum in global memory, behind a plain load of the key that skips
//                           the atomic where the stored key is already no larger: stored keys only decrease, so a stale value is
//                           an upper bound and a skip decided on it is still right.
//   render_resolve_kernel   one thread per target pixel: the key's two words are depth and index, the colour is cc_colour of the
//                           source pixel's three channels - the bytes the PLY export writes for it.
#include "cloud_common.h"                                   // load_eligible, to_camera, dist_key, cc_colour, the entry point's checks
#include "common.h"
#include "g2vlm_hip.h"

#ifndef G2V_RENDER_TEST_FIRST
#define G2V_RENDER_TEST_FIRST 1             // A/B builds only (tools/bench_render.py): the plain load before the atomic, on / off
#endif
#ifndef G2V_RENDER_STAGES
#define G2V_RENDER_STAGES 7                 // timing builds only (tools/bench_render.py): bit 0 fill, bit 1 splat, bit 2 resolve
#endif

static_assert(G2V_RENDER_STAGES == 1 || G2V_RENDER_STAGES == 3 || G2V_RENDER_STAGES == 7, "a stage runs only behind the stages before it");

namespace {

constexpr int RS_TW = 32, RS_TH = 8, RS_THREADS = RS_TW * RS_TH;
constexpr int RF_THREADS = 256, RF_MAX_BLOCKS = 8192;
constexpr int R_MAX_RADIUS = 8, R_MAX_TARGETS = 65535;
constexpr unsigned long long R_EMPTY = ~0ull;

// grid-stride over the M OH OW keys
__global__ __launch_bounds__(RF_THREADS) void render_fill_kernel(unsigned long long* keys, long total) {
  const long stride = (long)gridDim.x * RF_THREADS;
  for (long t = (long)blockIdx.x * RF_THREADS + threadIdx.x; t < total; t += stride) keys[t] = R_EMPTY;
}

struct Hit { bool lands; int x0, y0; float depth; };

// One source point against one target camera: to_camera, then the pixel it lands on.
__device__ __forceinline__ Hit project(float px, float py, float pz, const float* __restrict__ pose, const float* __restrict__ k,
                                       int OH, int OW) {
  const CamPoint c = to_camera(px, py, pz, pose, k);
  Hit h = {false, 0, 0, c.q2};
  // false on NaN; only inside is u or v converted
  if (c.q2 > 0.f && finite_f(c.q2) && c.u >= 0.f && c.u < (float)OW && c.v >= 0.f && c.v < (float)OH) {
    h.lands = true;
    h.x0 = (int)c.u;                                         // 0 <= x0 < OW, 0 <= y0 < OH
    h.y0 = (int)c.v;
  }
  return h;
}

__device__ __forceinline__ void key_min(unsigned long long* slot, unsigned long long key) {
#if G2V_RENDER_TEST_FIRST
  if (*slot <= key) return;                                  // a plain load, may be stale: then it is too large, never too small
#endif
  atomicMin(slot, key);
}

// 1-D grid over (view, tile row, tile column): N may be large (no limit of 65535 on it)
__global__ __launch_bounds__(RS_THREADS) void render_splat_kernel(const float* __restrict__ points, const uint8_t* __restrict__ mask,
                                                                   const float* __restrict__ poses, const float* __restrict__ K,
                                                                   const int* __restrict__ skip, int H, int W, int tiles_x, int tiles_y,
                                                                   int M, int OH, int OW, int radius, unsigned long long* keys) {
  const int tid = threadIdx.x;
  const long tile = blockIdx.x;
  const int bx = (int)(tile % tiles_x), by = (int)((tile / tiles_x) % tiles_y), i = (int)(tile / ((long)tiles_x * tiles_y));
  const int x = bx * RS_TW + (tid & (RS_TW - 1)), y = by * RS_TH + tid / RS_TW;
  const long hw = (long)H * W, ohw = (long)OH * OW;
  const long p = (long)i * hw + (long)y * W + x;             // <= 2^31 - 1 where live
  float px = 0.f, py = 0.f, pz = 0.f;
  bool eligible = false;
  if (x < W && y < H) eligible = load_eligible(points, mask, p, px, py, pz);
  if (!eligible) return;                                     // a wave without an eligible pixel ends here as a whole
  for (int m = 0; m < M; ++m) {
    if (skip && skip[m] == i) continue;                      // wave-uniform
    const Hit h = project(px, py, pz, poses + (long)m * 16, K + (long)m * 9, OH, OW);
    if (!h.lands) continue;
    const unsigned long long key = dist_key(h.depth, (uint32_t)p);
    unsigned long long* plane = keys + (long)m * ohw;
    const int xa = max(h.x0 - radius, 0), xb = min(h.x0 + radius, OW - 1);
    const int ya = max(h.y0 - radius, 0), yb = min(h.y0 + radius, OH - 1);
    for (int ty = ya; ty <= yb; ++ty)
      for (int tx = xa; tx <= xb; ++tx) key_min(plane + (long)ty * OW + tx, key);
  }
}

// grid-stride over the M OH OW target pixels
__global__ __launch_bounds__(RF_THREADS) void render_resolve_kernel(const unsigned long long* __restrict__ keys, const float* __restrict__ colors,
                                                                     long total, uint32_t hw, uint32_t bg, uint8_t* __restrict__ color_out,
                                                                     float* __restrict__ depth_out, int* __restrict__ index_out) {
  const long stride = (long)gridDim.x * RF_THREADS;
  for (long t = (long)blockIdx.x * RF_THREADS + threadIdx.x; t < total; t += stride) {
    const unsigned long long key = keys[t];
    const bool hit = key != R_EMPTY;
    const uint32_t p = (uint32_t)key;
    if (depth_out) depth_out[t] = hit ? __uint_as_float((uint32_t)(key >> 32)) : 0.f;
    if (index_out) index_out[t] = hit ? (int)p : -1;
    if (color_out) {
      uint8_t r = (uint8_t)(bg >> 16), g = (uint8_t)(bg >> 8), b = (uint8_t)bg;
      if (hit) {
        const uint32_t i = p / hw, rem = p % hw;
        const float* c = colors + (long)i * 3 * hw + rem;
        r = cc_colour(c[0]); g = cc_colour(c[hw]); b = cc_colour(c[2 * hw]);
      }
      color_out[t * 3] = r; color_out[t * 3 + 1] = g; color_out[t * 3 + 2] = b;
    }
  }
}

inline bool bad_target(int M, int OH, int OW) { return bad_nhw(M, OH, OW) || M > R_MAX_TARGETS; }

}  // namespace

extern "C" int64_t g2v_cloud_render_workspace(int M, int OH, int OW) {
  if (bad_target(M, OH, OW)) return 0;
  return 8 * (int64_t)M * OH * OW;
}

extern "C" int g2v_cloud_render(const void* points, const void* colors, const void* mask, int N, int H, int W,
                                const void* poses, const void* K, const void* skip, int M, int OH, int OW,
                                int radius, int background,
                                void* color_out, void* depth_out, void* index_out,
                                void* workspace, int64_t workspace_bytes, void* stream) {
  if (bad_nhw(N, H, W) || bad_target(M, OH, OW) || !points || !poses || !K || !workspace) return G2V_ERR_ARG;
  if (radius < 0 || radius > R_MAX_RADIUS || background < 0 || background > 0xFFFFFF) return G2V_ERR_ARG;
  if (!color_out && !depth_out && !index_out) return G2V_ERR_ARG;
  if (color_out && !colors) return G2V_ERR_ARG;
  if (workspace_bytes < g2v_cloud_render_workspace(M, OH, OW) || !aligned(workspace, 8) || !aligned(points, 4) || !aligned(colors, 4) ||
      !aligned(poses, 4) || !aligned(K, 4) || !aligned(skip, 4) || !aligned(depth_out, 4) || !aligned(index_out, 4))
    return G2V_ERR_ARG;
  const long total = (long)M * OH * OW;
  const long fill_blocks = (total + RF_THREADS - 1) / RF_THREADS;
  const dim3 fill_grid((unsigned)(fill_blocks < RF_MAX_BLOCKS ? fill_blocks : RF_MAX_BLOCKS));
  const int tiles_x = (W + RS_TW - 1) / RS_TW, tiles_y = (H + RS_TH - 1) / RS_TH;
  const long tiles = (long)tiles_x * tiles_y * N;            // <= N H W: fits the grid's x extent
  unsigned long long* keys = (unsigned long long*)workspace;
  if (G2V_RENDER_STAGES & 1) {
    hipLaunchKernelGGL(render_fill_kernel, fill_grid, dim3(RF_THREADS), 0, (hipStream_t)stream, keys, total);
    G2V_CHECK_LAUNCH();
  }
  if (G2V_RENDER_STAGES & 2) {
    hipLaunchKernelGGL(render_splat_kernel, dim3((unsigned)tiles), dim3(RS_THREADS), 0, (hipStream_t)stream, (const float*)points,
                       (const uint8_t*)mask, (const float*)poses, (const float*)K, (const int*)skip, H, W, tiles_x, tiles_y, M, OH, OW,
                       radius, keys);
    G2V_CHECK_LAUNCH();
  }
  if (G2V_RENDER_STAGES & 4) {
    hipLaunchKernelGGL(render_resolve_kernel, fill_grid, dim3(RF_THREADS), 0, (hipStream_t)stream, (const unsigned long long*)keys,
                       (const float*)colors, total, (uint32_t)H * (uint32_t)W, (uint32_t)background, (uint8_t*)color_out, (float*)depth_out,
                       (int*)index_out);
    G2V_CHECK_LAUNCH();
  }
  return G2V_OK;
}
