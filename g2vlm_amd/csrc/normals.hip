// Per-pixel surface normals of a reconstruction (g2vlm_utils.estimate_normals / view_angle_mask / save_point_cloud_normals /
// save_normal_maps): every view of recon's pointmap is a regular H x W grid of 3-D points, so the cross products of the edges to a
// pixel's axis neighbours ARE its surface normal at that resolution - an image-space normal.  Inputs are points fp32 [N,H,W,3], a
// keep mask u8 [N,H,W] (NULL: all pixels), camera-to-world poses fp32 [N,4,4] (NULL: the camera is at the origin) and an optional
// longest edge.
//
// The rule (include/g2vlm_hip.h and DESIGN.md 6u state it in full; tests/normals_check.py restates it in numpy): the edges to the
// neighbours R, D, L, U at distance `step` that take part (and are no longer than max_edge), the cross products of the pairs (R,D),
// (D,L), (L,U), (U,R) that are both there, summed in that order, normalised, turned towards the camera.  fp32 with contraction
// off in normal_of(): every - * + is its own rounding, sqrt and / are correctly rounded.  Nothing but the inputs enters the
// result: no atomics, no order of execution.
//
//   normals_kernel<false>      a workgroup per 32 x 8 tile of one view, one thread per pixel, the four neighbours by plain global
//                              loads (the tile's rows are re-read by its neighbours out of the cache).  Every step.
//   normals_kernel<true>       step 1 only: the 10 x 34 points and eligibility bytes the tile touches staged in LDS first.
//   normals_count / scan / scatter   g2v_cloud_compact's three launches for 27-byte records (<f4 x,y,z; <f4 nx,ny,nz; u1 r,g,b),
//                              built from cloud_common.h's block_sum, block_offset_scan and staged_flush; cloud.hip is untouched.
#include "cloud_common.h"                                   // load_eligible, cc_colour, the scan / count / flush of a block, the checks
#include "common.h"
#include "g2vlm_hip.h"

namespace {

constexpr int NT_TW = 32, NT_TH = 8, NT_THREADS = NT_TW * NT_TH;
constexpr int NC_THREADS = 256, NC_PER = 4, NC_BLOCK = NC_THREADS * NC_PER;   // pixels of one view per workgroup
constexpr int NC_REC = 27;
static_assert(NC_THREADS == PC_THREADS, "cloud_common.h's scan, count and flush are written for this workgroup");

struct V3 { float x, y, z; };
struct Normal { bool valid; V3 n; float cos_view; V3 colour; };

// The rule for one pixel that takes part: p its point, q[k] / in[k] the point of neighbour k (R, D, L, U) and whether it lies inside
// the view and takes part (q[k] is read only as a number: what stands there for an absent neighbour does not reach the result),
// c the camera centre.
__device__ __forceinline__ Normal normal_of(V3 p, const V3 (&q)[4], const bool (&in)[4], V3 c, bool stretch, float max_edge) {
#pragma clang fp contract(off)
  V3 e[4];
  bool av[4];
  const float lim = max_edge * max_edge;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    e[k].x = q[k].x - p.x; e[k].y = q[k].y - p.y; e[k].z = q[k].z - p.z;
    av[k] = in[k];
    if (stretch) av[k] = av[k] && ((e[k].x * e[k].x + e[k].y * e[k].y) + e[k].z * e[k].z <= lim);   // `<=` is false on NaN
  }
  V3 m = {0.f, 0.f, 0.f};
  bool have = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {                              // (R,D) (D,L) (L,U) (U,R)
    const V3 a = e[k], b = e[(k + 1) & 3];
    if (!(av[k] && av[(k + 1) & 3])) continue;
    V3 x;
    x.x = a.y * b.z - a.z * b.y;
    x.y = a.z * b.x - a.x * b.z;
    x.z = a.x * b.y - a.y * b.x;
    if (have) { m.x = m.x + x.x; m.y = m.y + x.y; m.z = m.z + x.z; }
    else m = x;                                              // the sum starts from the first present product, not from +0
    have = true;
  }
  Normal r;
  r.n = {0.f, 0.f, 0.f}; r.colour = {0.f, 0.f, 0.f}; r.cos_view = 0.f;
  const float s2 = (m.x * m.x + m.y * m.y) + m.z * m.z;
  r.valid = have && finite_f(s2) && s2 > 0.f;
  if (!r.valid) return r;
  const float s = sqrtf(s2);                                 // correctly rounded, as the divisions: no fast-math in this build
  V3 n = {m.x / s, m.y / s, m.z / s};
  const V3 d = {p.x - c.x, p.y - c.y, p.z - c.z};
  const float t = (n.x * d.x + n.y * d.y) + n.z * d.z;
  if (t > 0.f) {                                             // towards the camera: a sign-bit flip, -0.0 included
    n.x = __uint_as_float(__float_as_uint(n.x) ^ 0x80000000u);
    n.y = __uint_as_float(__float_as_uint(n.y) ^ 0x80000000u);
    n.z = __uint_as_float(__float_as_uint(n.z) ^ 0x80000000u);
  }
  const float dd = (d.x * d.x + d.y * d.y) + d.z * d.z;
  float cv = fabsf(t) / sqrtf(dd);
  if (cv != cv) cv = 0.f;
  r.cos_view = cv < 1.f ? cv : 1.f;
  r.n = n;
  r.colour = {n.x * 0.5f + 0.5f, n.y * 0.5f + 0.5f, n.z * 0.5f + 0.5f};
  return r;
}

// 1-D grid over (view, tile row, tile column)
template <bool HALO>
__global__ __launch_bounds__(NT_THREADS) void normals_kernel(const float* __restrict__ points, const uint8_t* __restrict__ mask,
                                                              const float* __restrict__ poses, int H, int W, int tiles_x, int tiles_y, int step,
                                                              int stretch, float max_edge, float* __restrict__ normals, uint8_t* __restrict__ valid,
                                                              float* __restrict__ cos_view, float* __restrict__ colours) {
  const int tid = threadIdx.x;
  const long tile = blockIdx.x;
  const int bx = (int)(tile % tiles_x), by = (int)((tile / tiles_x) % tiles_y), view = (int)(tile / ((long)tiles_x * tiles_y));
  const int c0 = bx * NT_TW, r0 = by * NT_TH;
  const long hw = (long)H * W, base = (long)view * hw;
  const int tx = tid & (NT_TW - 1), ty = tid / NT_TW;
  const int x = c0 + tx, y = r0 + ty;
  const int dx[4] = {step, 0, -step, 0}, dy[4] = {0, step, 0, -step};   // R, D, L, U
  V3 p = {0.f, 0.f, 0.f}, q[4];
  bool part = false, in[4];

  if constexpr (HALO) {                                      // step == 1: pt[i][j] is pixel (r0 - 1 + i, c0 - 1 + j)
    __shared__ float pt[NT_TH + 2][NT_TW + 2][3];            // a stride of 3 dwords: no bank is hit twice by 32 neighbours
    __shared__ uint8_t el[NT_TH + 2][NT_TW + 2];
    for (int i = tid; i < (NT_TH + 2) * (NT_TW + 2); i += NT_THREADS) {
      const int hy = i / (NT_TW + 2), hx = i - hy * (NT_TW + 2);
      const int yy = r0 - 1 + hy, xx = c0 - 1 + hx;
      float a = 0.f, b = 0.f, c = 0.f;
      bool ok = false;
      if (yy >= 0 && yy < H && xx >= 0 && xx < W) ok = load_eligible(points, mask, base + (long)yy * W + xx, a, b, c);   // the halo stays inside the view
      pt[hy][hx][0] = a; pt[hy][hx][1] = b; pt[hy][hx][2] = c;
      el[hy][hx] = ok;
    }
    __syncthreads();
    if (x >= W || y >= H) return;
    p = {pt[ty + 1][tx + 1][0], pt[ty + 1][tx + 1][1], pt[ty + 1][tx + 1][2]};
    part = el[ty + 1][tx + 1] != 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int hy = ty + 1 + dy[k], hx = tx + 1 + dx[k];
      q[k] = {pt[hy][hx][0], pt[hy][hx][1], pt[hy][hx][2]};
      in[k] = el[hy][hx] != 0;
    }
  } else {
    if (x >= W || y >= H) return;
    part = load_eligible(points, mask, base + (long)y * W + x, p.x, p.y, p.z);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int yy = y + dy[k], xx = x + dx[k];
      q[k] = {0.f, 0.f, 0.f};
      in[k] = false;
      if (part && yy >= 0 && yy < H && xx >= 0 && xx < W) in[k] = load_eligible(points, mask, base + (long)yy * W + xx, q[k].x, q[k].y, q[k].z);
    }
  }

  Normal r;
  r.valid = false; r.n = {0.f, 0.f, 0.f}; r.colour = {0.f, 0.f, 0.f}; r.cos_view = 0.f;
  if (part) {
    V3 c = {0.f, 0.f, 0.f};
    if (poses) c = {poses[view * 16 + 3], poses[view * 16 + 7], poses[view * 16 + 11]};
    r = normal_of(p, q, in, c, stretch != 0, max_edge);
  }
  const long px = base + (long)y * W + x;
  if (normals) { normals[3 * px] = r.n.x; normals[3 * px + 1] = r.n.y; normals[3 * px + 2] = r.n.z; }
  if (valid) valid[px] = r.valid ? 1 : 0;
  if (cos_view) cos_view[px] = r.cos_view;
  if (colours) {
    float* o = colours + (long)view * 3 * hw + (long)y * W + x;
    o[0] = r.colour.x; o[hw] = r.colour.y; o[2 * hw] = r.colour.z;
  }
}

// ---------------------------------------------------------------------------------------------------------- compaction
// the mask bytes of pixels [i, i + 4) of a view of hw pixels (pixels >= hw: 0)
__device__ __forceinline__ uint32_t nc_mask4(const uint8_t* m, long i, long hw) {
  if (i + 4 <= hw && (reinterpret_cast<uintptr_t>(m + i) & 3) == 0) return *reinterpret_cast<const uint32_t*>(m + i);
  uint32_t w = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (i + k < hw) w |= (uint32_t)m[i + k] << (8 * k);
  return w;
}
__device__ __forceinline__ int nc_kept(uint32_t w, int k) { return ((w >> (8 * k)) & 0xffu) != 0; }
__device__ __forceinline__ int nc_count4(uint32_t w) { return nc_kept(w, 0) + nc_kept(w, 1) + nc_kept(w, 2) + nc_kept(w, 3); }

// the 12 floats of pixels [i, i + 4) of view n of a [N,H,W,3] array (pixels >= hw: 0), three 16-byte loads where the address allows
__device__ __forceinline__ void nc_load12(const float* a, long n, long i, long hw, int vec, float (&out)[NC_PER * 3]) {
  const long p = n * hw + i;
  const float* ps = a + p * 3;
  if (vec && i + NC_PER <= hw && (p & 3) == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(ps + 4 * k);
      out[4 * k] = v[0]; out[4 * k + 1] = v[1]; out[4 * k + 2] = v[2]; out[4 * k + 3] = v[3];
    }
  } else {
#pragma unroll
    for (int k = 0; k < NC_PER * 3; ++k) out[k] = (i + k / 3 < hw) ? ps[k] : 0.f;
  }
}

__device__ __forceinline__ void nc_put(uint8_t* s, float v) {
  const uint32_t b = __float_as_uint(v);
  s[0] = (uint8_t)b; s[1] = (uint8_t)(b >> 8); s[2] = (uint8_t)(b >> 16); s[3] = (uint8_t)(b >> 24);
}

// grid (blocks per view, N): kept pixels of the workgroup's NC_BLOCK pixels
__global__ __launch_bounds__(NC_THREADS) void normals_count_kernel(const uint8_t* mask, long hw, int* block_cnt) {
  __shared__ int sh[PC_WAVES];
  const long i = (long)blockIdx.x * NC_BLOCK + threadIdx.x * NC_PER;
  const int kept = block_sum(nc_count4(nc_mask4(mask + (long)blockIdx.y * hw, i, hw)), sh);
  if (threadIdx.x == 0) block_cnt[(long)blockIdx.y * gridDim.x + blockIdx.x] = kept;
}

// one workgroup: block_off[b] = kept pixels before block b, counts[n] = kept pixels of view n (at most N H W <= 2^31 - 1 in all)
__global__ __launch_bounds__(NC_THREADS) void normals_scan_kernel(const int* block_cnt, int* block_off, int* counts, int N, int bpv) {
  __shared__ int sh[PC_WAVES];
  block_offset_scan(block_cnt, block_off, (long)N * bpv, sh);
  for (int n = threadIdx.x; n < N; n += NC_THREADS) {
    int s = 0;
    for (int j = 0; j < bpv; ++j) s += block_cnt[(long)n * bpv + j];
    counts[n] = s;
  }
}

// grid (blocks per view, N): the workgroup's records, staged in LDS at the byte offset its output range has inside a dword
__global__ __launch_bounds__(NC_THREADS) void normals_scatter_kernel(const float* points, const float* normals, const float* colors,
                                                                      const uint8_t* mask, const int* block_off, uint8_t* rec, long max_records,
                                                                      long hw, int pvec, int nvec) {
  __shared__ int sh[PC_WAVES];
  __shared__ __attribute__((aligned(16))) uint8_t stage[NC_BLOCK * NC_REC + 16];
  const int tid = threadIdx.x, n = blockIdx.y;
  const long i = (long)blockIdx.x * NC_BLOCK + tid * NC_PER;  // first of the thread's pixels inside the view
  const uint32_t w = nc_mask4(mask + (long)n * hw, i, hw);
  const int c = nc_count4(w);
  int kept;
  const int before = block_incl_scan(c, sh, kept) - c;
  if (kept == 0) return;
  const long first = block_off[(long)n * gridDim.x + blockIdx.x];       // record index of the workgroup's first record
  const long byte0 = first * NC_REC;
  const int mis = (int)((reinterpret_cast<uintptr_t>(rec) + byte0) & 3);

  if (c) {
    float xyz[NC_PER * 3], nrm[NC_PER * 3];
    nc_load12(points, n, i, hw, pvec, xyz);
    nc_load12(normals, n, i, hw, nvec, nrm);
    int slot = before;
#pragma unroll
    for (int k = 0; k < NC_PER; ++k) {
      if (!nc_kept(w, k)) continue;
      uint8_t* s = stage + mis + slot * NC_REC;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        nc_put(s + 4 * j, xyz[3 * k + j]);
        nc_put(s + 12 + 4 * j, nrm[3 * k + j]);
        s[24 + j] = cc_colour(colors[((long)n * 3 + j) * hw + i + k]);   // a kept pixel lies inside the view
      }
      ++slot;
    }
  }
  __syncthreads();

  long nrec = kept;                                          // records past the caller's capacity are not written
  if (first + nrec > max_records) nrec = max_records > first ? max_records - first : 0;
  staged_flush(stage, rec, byte0, mis, (int)nrec * NC_REC);
}

inline int nc_blocks_per_view(int H, int W) { return (int)(((long)H * W + NC_BLOCK - 1) / NC_BLOCK); }

}  // namespace

extern "C" int g2v_cloud_normals(const void* points, const void* mask, const void* poses, int N, int H, int W, int step, int flags,
                                 float max_edge, void* normals, void* valid, void* cos_view, void* colors_out, void* stream) {
  const int forms = G2V_NORMALS_PLAIN | G2V_NORMALS_HALO;
  if (bad_nhw(N, H, W) || N > 65535 || step < 1 || step > G2V_NORMALS_STEP_MAX || (flags & ~(G2V_NORMALS_MAX_EDGE | forms))) return G2V_ERR_ARG;
  if ((flags & forms) == forms || ((flags & G2V_NORMALS_HALO) && step != 1)) return G2V_ERR_ARG;
  if ((flags & G2V_NORMALS_MAX_EDGE) && !(max_edge >= 0.f)) return G2V_ERR_ARG;   // negative or NaN
  if (!points || (!normals && !valid && !cos_view && !colors_out)) return G2V_ERR_ARG;
  if (!aligned(points, 4) || !aligned(poses, 4) || !aligned(normals, 4) || !aligned(cos_view, 4) || !aligned(colors_out, 4)) return G2V_ERR_ARG;
  const int tiles_x = (W + NT_TW - 1) / NT_TW, tiles_y = (H + NT_TH - 1) / NT_TH;
  const long tiles = (long)tiles_x * tiles_y * N;            // <= N H W: fits the grid's x extent
  // without a form flag: plain loads at every step (DESIGN.md 6u has the measurement that decided it)
  const bool halo = (flags & G2V_NORMALS_HALO) != 0;
  auto kernel = halo ? normals_kernel<true> : normals_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)tiles), dim3(NT_THREADS), 0, (hipStream_t)stream, (const float*)points, (const uint8_t*)mask,
                     (const float*)poses, H, W, tiles_x, tiles_y, step, flags & G2V_NORMALS_MAX_EDGE, max_edge, (float*)normals, (uint8_t*)valid,
                     (float*)cos_view, (float*)colors_out);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

extern "C" int64_t g2v_cloud_compact_normals_workspace(int N, int H, int W) {
  if (bad_nhw(N, H, W) || N > 65535) return 0;
  return 8 * (int64_t)N * nc_blocks_per_view(H, W);
}

extern "C" int g2v_cloud_compact_normals(const void* points, const void* normals, const void* colors, const void* mask, int N, int H, int W,
                                         void* records, int64_t max_records, void* counts, void* workspace, int64_t workspace_bytes,
                                         void* stream) {
  if (bad_nhw(N, H, W) || N > 65535 || !points || !normals || !colors || !mask || !counts || !workspace || max_records < 0 ||
      (max_records > 0 && !records))
    return G2V_ERR_ARG;
  if (workspace_bytes < g2v_cloud_compact_normals_workspace(N, H, W) || !aligned(points, 4) || !aligned(normals, 4) || !aligned(colors, 4) ||
      !aligned(workspace, 4) || !aligned(counts, 4))
    return G2V_ERR_ARG;
  const int bpv = nc_blocks_per_view(H, W);
  const long hw = (long)H * W;
  int* block_cnt = (int*)workspace;
  int* block_off = block_cnt + (long)N * bpv;
  const dim3 grid((unsigned)bpv, (unsigned)N);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(normals_count_kernel, grid, dim3(NC_THREADS), 0, s, (const uint8_t*)mask, hw, block_cnt);
  G2V_CHECK_LAUNCH();
  hipLaunchKernelGGL(normals_scan_kernel, dim3(1), dim3(NC_THREADS), 0, s, (const int*)block_cnt, block_off, (int*)counts, N, bpv);
  G2V_CHECK_LAUNCH();
  if (max_records > 0) {
    hipLaunchKernelGGL(normals_scatter_kernel, grid, dim3(NC_THREADS), 0, s, (const float*)points, (const float*)normals, (const float*)colors,
                       (const uint8_t*)mask, (const int*)block_off, (uint8_t*)records, (long)max_records, hw, aligned(points, 16),
                       aligned(normals, 16));
    G2V_CHECK_LAUNCH();
  }
  return G2V_OK;
}
