// Triangle-mesh export of a reconstruction (g2vlm_utils.reconstruct_mesh / save_mesh): every view of recon's pointmap is a regular
// H x W grid of 3-D points, so the pixel grid triangulated IS its surface - the "image mesh" - once the triangles that reach over a
// pixel the mask drops (depth edges, low confidence, multi-view outliers) or that stretch too far are left out.  Inputs are points
// fp32 [N,H,W,3], a keep mask u8 [N,H,W] (NULL: all pixels) and an optional longest edge.
//
// The rule (include/g2vlm_hip.h and DESIGN.md 6n state it in full; tests/mesh_check.py restates it in numpy): a quad whose four
// corners are kept is cut along its shorter diagonal (fp32 squared lengths by cloud_common.h's sq_dist3, every operation rounded
// once - contraction is switched off there and in classify() -, a tie or a NaN takes the main diagonal), a quad with three kept
// corners gives their one triangle, every triangle faces the camera.  Faces come in view-major, quad row-major order; vertices are
// the kept pixels some face references, in flat pixel order.  Every position is an integer prefix sum: the bytes do not depend on the order in which anything ran.
//
//   mesh_classify_kernel   a workgroup per 32 x 8 tile of one view, the 9 x 33 points and mask bytes its quads touch in LDS (a
//                          one-pixel halo to the right and below), one thread per quad: each quad is classified exactly once.
//                          Writes a code byte per pixel: bit k = triangle k of the pixel's quad is a face (0 where no quad is
//                          anchored: the last row and column).
//   mesh_count_kernel      flat workgroups of MC_BLOCK pixels of a view, as cloud.hip's compaction: `used` of a pixel is gathered
//                          from the code bytes of the four quads it is a corner of (no atomics), the faces of a pixel are the
//                          bits of its own code; per workgroup the number of each.
//   mesh_scan_kernel       one workgroup: exclusive sums of both block counts, and counts[n] = {vertices, faces} of view n.
//   mesh_vertex_kernel     vertex_of = block offset + rank inside the block, or -1.
//   mesh_face_kernel       the faces of a block's quads: vertex ids of the corners through vertex_of, int32 triples stored
//                          straight from registers (their slots are consecutive), the 13-byte PLY records staged in LDS at the
//                          byte offset their range has inside a dword so that the stores are aligned dwords (cloud_common.h's
//                          staged_flush, as cloud_scatter_kernel's 15-byte records).
#include "cloud_common.h"                                   // sq_dist3, the scan / count / flush of a block, the entry point's checks
#include "common.h"
#include "g2vlm_hip.h"

namespace {

constexpr int MT_TW = 32, MT_TH = 8, MT_THREADS = MT_TW * MT_TH;
constexpr int MC_THREADS = 256, MC_PER = 4, MC_BLOCK = MC_THREADS * MC_PER;   // pixels of one view per workgroup
constexpr int MF_REC = 13, MF_MAX = 2 * MC_BLOCK;                             // bytes of a face record, faces of a workgroup at most
static_assert(MC_THREADS == PC_THREADS, "cloud_common.h's scan, count and flush are written for this workgroup");

// triangle k of the quad with corners p00 p01 / p10 p11; bit k of a code byte.  0, 1: the anti diagonal's pair; 2, 3: the main one's
enum { T_A1 = 1, T_A2 = 2, T_M1 = 4, T_M2 = 8 };               // (p00,p10,p01) (p01,p10,p11) (p00,p10,p11) (p00,p11,p01)
constexpr int USES_P00 = T_A1 | T_M1 | T_M2, USES_P01 = T_A1 | T_A2 | T_M2, USES_P10 = T_A1 | T_A2 | T_M1, USES_P11 = T_A2 | T_M1 | T_M2;

struct P3 { float x, y, z; };

__device__ __forceinline__ float edge2(P3 a, P3 b) { return sq_dist3(a.x, a.y, a.z, b.x, b.y, b.z); }

// the code byte of one quad: k?? = the mask keeps the corner
__device__ __forceinline__ int classify(P3 p00, P3 p01, P3 p10, P3 p11, bool k00, bool k01, bool k10, bool k11, bool stretch,
                                        float max_edge) {
#pragma clang fp contract(off)
  const int kept = (int)k00 + (int)k01 + (int)k10 + (int)k11;
  if (kept < 3) return 0;
  const float ea = edge2(p01, p10), em = edge2(p00, p11);
  int code;
  if (kept == 4) code = ea < em ? (T_A1 | T_A2) : (T_M1 | T_M2);             // false on a tie and on NaN: the main diagonal
  else code = !k11 ? T_A1 : !k00 ? T_A2 : !k01 ? T_M1 : T_M2;
  if (stretch) {
    const float lim = max_edge * max_edge;
    // an edge that reaches a dropped corner belongs to no triangle of this code; `<=` is false on NaN
    const bool top = edge2(p00, p01) <= lim, left = edge2(p00, p10) <= lim, right = edge2(p01, p11) <= lim,
               bottom = edge2(p10, p11) <= lim, anti = ea <= lim, mdia = em <= lim;
    int ok = 0;
    if (left && anti && top) ok |= T_A1;
    if (anti && bottom && right) ok |= T_A2;
    if (left && bottom && mdia) ok |= T_M1;
    if (mdia && right && top) ok |= T_M2;
    code &= ok;
  }
  return code;
}

// 1-D grid over (view, tile row, tile column): N may be large
__global__ __launch_bounds__(MT_THREADS) void mesh_classify_kernel(const float* __restrict__ points, const uint8_t* __restrict__ mask, int H,
                                                                    int W, int tiles_x, int tiles_y, int stretch, float max_edge,
                                                                    uint8_t* __restrict__ code) {
  __shared__ float pt[MT_TH + 1][MT_TW + 1][3];              // a stride of 3 dwords: no bank is hit twice by 32 neighbours
  __shared__ uint8_t kp[MT_TH + 1][MT_TW + 1];
  const int tid = threadIdx.x;
  const long tile = blockIdx.x;
  const int bx = (int)(tile % tiles_x), by = (int)((tile / tiles_x) % tiles_y), view = (int)(tile / ((long)tiles_x * tiles_y));
  const int c0 = bx * MT_TW, r0 = by * MT_TH;
  const long base = (long)view * H * W;
  for (int i = tid; i < (MT_TH + 1) * (MT_TW + 1); i += MT_THREADS) {
    const int ty = i / (MT_TW + 1), tx = i - ty * (MT_TW + 1);
    const int y = r0 + ty, x = c0 + tx;
    float a = 0.f, b = 0.f, c = 0.f;
    uint8_t k = 0;
    if (y < H && x < W) {                                    // the halo stays inside the view
      const long p = base + (long)y * W + x;
      k = mask ? (mask[p] != 0) : 1;
      a = points[p * 3]; b = points[p * 3 + 1]; c = points[p * 3 + 2];
    }
    pt[ty][tx][0] = a; pt[ty][tx][1] = b; pt[ty][tx][2] = c;
    kp[ty][tx] = k;
  }
  __syncthreads();
  const int tx = tid & (MT_TW - 1), ty = tid / MT_TW;
  const int x = c0 + tx, y = r0 + ty;
  if (x >= W || y >= H) return;
  int cd = 0;
  if (x < W - 1 && y < H - 1) {
    const P3 p00 = {pt[ty][tx][0], pt[ty][tx][1], pt[ty][tx][2]}, p01 = {pt[ty][tx + 1][0], pt[ty][tx + 1][1], pt[ty][tx + 1][2]},
             p10 = {pt[ty + 1][tx][0], pt[ty + 1][tx][1], pt[ty + 1][tx][2]},
             p11 = {pt[ty + 1][tx + 1][0], pt[ty + 1][tx + 1][1], pt[ty + 1][tx + 1][2]};
    cd = classify(p00, p01, p10, p11, kp[ty][tx] != 0, kp[ty][tx + 1] != 0, kp[ty + 1][tx] != 0, kp[ty + 1][tx + 1] != 0, stretch != 0,
                  max_edge);
  }
  code[base + (long)y * W + x] = (uint8_t)cd;
}

// is pixel (y, x) of the view whose code bytes are `cv` a corner of some face?  Its four quads are anchored at (y, x), (y, x - 1),
// (y - 1, x), (y - 1, x - 1); the code of a pixel in the last row or column is 0.
__device__ __forceinline__ int used_of(const uint8_t* __restrict__ cv, int y, int x, int W) {
  const long q = (long)y * W + x;
  int u = cv[q] & USES_P00;
  if (x > 0) u |= cv[q - 1] & USES_P01;
  if (y > 0) u |= cv[q - W] & USES_P10;
  if (x > 0 && y > 0) u |= cv[q - W - 1] & USES_P11;
  return u != 0;
}

// grid (blocks per view, N): used bytes of the workgroup's MC_BLOCK pixels and the number of its vertices and faces
__global__ __launch_bounds__(MC_THREADS) void mesh_count_kernel(const uint8_t* __restrict__ code, int H, int W, uint8_t* __restrict__ used,
                                                                 int* __restrict__ cnt_v, int* __restrict__ cnt_f) {
  __shared__ int sh[2][MC_THREADS / 64];
  const long hw = (long)H * W;
  const uint8_t* cv = code + (long)blockIdx.y * hw;
  const long i = (long)blockIdx.x * MC_BLOCK + threadIdx.x * MC_PER;
  int nv = 0, nf = 0;
  if (i < hw) {
    int y = (int)(i / W), x = (int)(i - (long)y * W);
#pragma unroll
    for (int k = 0; k < MC_PER; ++k) {
      if (i + k >= hw) break;
      const int u = used_of(cv, y, x, W);
      used[(long)blockIdx.y * hw + i + k] = (uint8_t)u;
      nv += u;
      nf += __popc((unsigned)cv[i + k]);
      if (++x == W) { x = 0; ++y; }
    }
  }
  // Two sums in one butterfly and behind one barrier.  cloud_common.h's block_sum sums one value and has no barrier in front, so two
  // calls would need a barrier more and run their butterflies one after the other: that form was +0.3 / +0.6 us on count_only
  // (profiles/cloud_common_ab.json, "mesh_count_kernel_with_block_sum_twice"), so this kernel keeps the parent's code.
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    nv += __shfl_xor(nv, o, 64);
    nf += __shfl_xor(nf, o, 64);
  }
  if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = nv; sh[1][threadIdx.x >> 6] = nf; }
  __syncthreads();
  if (threadIdx.x < 2) {
    int* out = threadIdx.x == 0 ? cnt_v : cnt_f;
    const int* s = sh[threadIdx.x];
    out[(long)blockIdx.y * gridDim.x + blockIdx.x] = s[0] + s[1] + s[2] + s[3];
  }
}

// one workgroup: off[b] = the sum of cnt before block b (block_offset_scan), for the vertex and the face counts in turn;
// counts[n] = {vertices, faces} of view n.  Both totals are at most 2^31 - 1 (the entry point's limits).
__global__ __launch_bounds__(MC_THREADS) void mesh_scan_kernel(const int* cnt_v, const int* cnt_f, int* off_v, int* off_f, int* counts, int N,
                                                                int bpv) {
  __shared__ int sh[MC_THREADS / 64];
  const long nb = (long)N * bpv;
  block_offset_scan(cnt_v, off_v, nb, sh);
  block_offset_scan(cnt_f, off_f, nb, sh);
  for (int n = threadIdx.x; n < N; n += MC_THREADS) {
    int v = 0, f = 0;
    for (int j = 0; j < bpv; ++j) {
      v += cnt_v[(long)n * bpv + j];
      f += cnt_f[(long)n * bpv + j];
    }
    counts[2 * n] = v;
    counts[2 * n + 1] = f;
  }
}

// grid (blocks per view, N)
__global__ __launch_bounds__(MC_THREADS) void mesh_vertex_kernel(const uint8_t* __restrict__ used, long hw, const int* __restrict__ off_v,
                                                                  int* __restrict__ vertex_of) {
  __shared__ int sh[MC_THREADS / 64];
  const long i = (long)blockIdx.x * MC_BLOCK + threadIdx.x * MC_PER;
  const long p = (long)blockIdx.y * hw + i;
  int u[MC_PER], c = 0;
#pragma unroll
  for (int k = 0; k < MC_PER; ++k) {
    u[k] = (i + k < hw) ? (used[p + k] != 0) : 0;
    c += u[k];
  }
  int total;
  int id = off_v[(long)blockIdx.y * gridDim.x + blockIdx.x] + block_incl_scan(c, sh, total) - c;
#pragma unroll
  for (int k = 0; k < MC_PER; ++k)
    if (i + k < hw) vertex_of[p + k] = u[k] ? id++ : -1;
}

// grid (blocks per view, N): the faces of the quads anchored at the workgroup's pixels
__global__ __launch_bounds__(MC_THREADS) void mesh_face_kernel(const uint8_t* __restrict__ code, const int* __restrict__ vertex_of, int H, int W,
                                                                const int* __restrict__ off_f, int* __restrict__ faces,
                                                                uint8_t* __restrict__ rec, long max_faces) {
  __shared__ int sh[MC_THREADS / 64];
  __shared__ __attribute__((aligned(16))) uint8_t stage[MF_MAX * MF_REC + 16];
  const int tid = threadIdx.x;
  const long hw = (long)H * W;
  const long i = (long)blockIdx.x * MC_BLOCK + tid * MC_PER;
  const long p = (long)blockIdx.y * hw + i;
  int cd[MC_PER], c = 0;
#pragma unroll
  for (int k = 0; k < MC_PER; ++k) {
    cd[k] = (i + k < hw) ? code[p + k] : 0;
    c += __popc((unsigned)cd[k]);
  }
  int nfaces;
  const int before = block_incl_scan(c, sh, nfaces) - c;
  if (nfaces == 0) return;
  const long first = off_f[(long)blockIdx.y * gridDim.x + blockIdx.x];  // index of the workgroup's first face
  const long byte0 = first * MF_REC;
  const int mis = rec ? (int)((reinterpret_cast<uintptr_t>(rec) + byte0) & 3) : 0;

  int slot = before;
#pragma unroll
  for (int k = 0; k < MC_PER; ++k) {
    if (cd[k] == 0) continue;
    // a quad is anchored here: the pixel is in neither the last row nor the last column, so all four corners are in the view
    const long q = p + k;
    const int v00 = vertex_of[q], v01 = vertex_of[q + 1], v10 = vertex_of[q + W], v11 = vertex_of[q + W + 1];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (!(cd[k] & (1 << t))) continue;
      const int a = (t == 1) ? v01 : v00;
      const int b = (t == 3) ? v11 : v10;
      const int cc = (t == 0) ? v01 : (t == 3) ? v01 : v11;
      if (faces && first + slot < max_faces) {
        int* f = faces + (first + slot) * 3;
        f[0] = a; f[1] = b; f[2] = cc;
      }
      if (rec) {
        uint8_t* s = stage + mis + slot * MF_REC;
        s[0] = 3;
        const uint32_t w[3] = {(uint32_t)a, (uint32_t)b, (uint32_t)cc};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          s[1 + 4 * j] = (uint8_t)w[j]; s[2 + 4 * j] = (uint8_t)(w[j] >> 8); s[3 + 4 * j] = (uint8_t)(w[j] >> 16);
          s[4 + 4 * j] = (uint8_t)(w[j] >> 24);
        }
      }
      ++slot;
    }
  }
  if (!rec) return;
  __syncthreads();

  long nrec = nfaces;                                        // records past the caller's capacity are not written
  if (first + nrec > max_faces) nrec = max_faces > first ? max_faces - first : 0;
  staged_flush(stage, rec, byte0, mis, (int)nrec * MF_REC);
}

inline int blocks_per_view(int H, int W) { return (int)(((long)H * W + MC_BLOCK - 1) / MC_BLOCK); }

// N*H*W <= 2^31 - 1 keeps every vertex id in int32 (g2v_cloud_compact's limit), 2 N (H-1) (W-1) <= 2^31 - 1 every face count;
// N is the grid's y extent
inline bool bad_shape(int N, int H, int W) {
  if (bad_nhw(N, H, W) || N > 65535) return true;
  return 2 * (int64_t)N * (H - 1) * (W - 1) > 0x7fffffffLL;
}

struct Layout { int64_t cnt_v, cnt_f, off_v, off_f, vertex_of, code, used, bytes; };
inline Layout layout(int N, int H, int W) {
  const int64_t nb = (int64_t)N * blocks_per_view(H, W), nhw = (int64_t)N * H * W;
  Layout l;
  l.cnt_v = 0; l.cnt_f = 4 * nb; l.off_v = 8 * nb; l.off_f = 12 * nb;
  l.vertex_of = 16 * nb;
  l.code = l.vertex_of + 4 * nhw;
  l.used = l.code + nhw;
  l.bytes = l.used + nhw;
  return l;
}

}  // namespace

extern "C" int64_t g2v_cloud_mesh_workspace(int N, int H, int W) {
  if (bad_shape(N, H, W)) return 0;
  return layout(N, H, W).bytes;
}

extern "C" int g2v_cloud_mesh(const void* points, const void* mask, int N, int H, int W, int flags, float max_edge, void* used,
                              void* vertex_of, void* faces, void* face_records, int64_t max_faces, void* counts, void* workspace,
                              int64_t workspace_bytes, void* stream) {
  if (bad_shape(N, H, W) || !points || !counts || !workspace || (flags & ~G2V_MESH_MAX_EDGE) || max_faces < 0) return G2V_ERR_ARG;
  if ((flags & G2V_MESH_MAX_EDGE) && !(max_edge >= 0.f)) return G2V_ERR_ARG;   // negative or NaN
  if (workspace_bytes < g2v_cloud_mesh_workspace(N, H, W) || !aligned(points, 4) || !aligned(workspace, 4) || !aligned(counts, 4) ||
      !aligned(vertex_of, 4) || !aligned(faces, 4))
    return G2V_ERR_ARG;
  const Layout l = layout(N, H, W);
  uint8_t* ws = (uint8_t*)workspace;
  int *cnt_v = (int*)(ws + l.cnt_v), *cnt_f = (int*)(ws + l.cnt_f), *off_v = (int*)(ws + l.off_v), *off_f = (int*)(ws + l.off_f);
  int* vof = vertex_of ? (int*)vertex_of : (int*)(ws + l.vertex_of);
  uint8_t* code = ws + l.code;
  uint8_t* use = used ? (uint8_t*)used : ws + l.used;
  const bool want_faces = max_faces > 0 && (faces || face_records);
  const int bpv = blocks_per_view(H, W);
  const int tiles_x = (W + MT_TW - 1) / MT_TW, tiles_y = (H + MT_TH - 1) / MT_TH;
  const long tiles = (long)tiles_x * tiles_y * N;            // <= N H W: fits the grid's x extent
  const dim3 grid((unsigned)bpv, (unsigned)N);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(mesh_classify_kernel, dim3((unsigned)tiles), dim3(MT_THREADS), 0, s, (const float*)points, (const uint8_t*)mask, H, W,
                     tiles_x, tiles_y, flags & G2V_MESH_MAX_EDGE, max_edge, code);
  G2V_CHECK_LAUNCH();
  hipLaunchKernelGGL(mesh_count_kernel, grid, dim3(MC_THREADS), 0, s, (const uint8_t*)code, H, W, use, cnt_v, cnt_f);
  G2V_CHECK_LAUNCH();
  hipLaunchKernelGGL(mesh_scan_kernel, dim3(1), dim3(MC_THREADS), 0, s, (const int*)cnt_v, (const int*)cnt_f, off_v, off_f, (int*)counts, N,
                     bpv);
  G2V_CHECK_LAUNCH();
  if (vertex_of || want_faces) {
    hipLaunchKernelGGL(mesh_vertex_kernel, grid, dim3(MC_THREADS), 0, s, (const uint8_t*)use, (long)H * W, (const int*)off_v, vof);
    G2V_CHECK_LAUNCH();
  }
  if (want_faces) {
    hipLaunchKernelGGL(mesh_face_kernel, grid, dim3(MC_THREADS), 0, s, (const uint8_t*)code, (const int*)vof, H, W, (const int*)off_f,
                       (int*)faces, (uint8_t*)face_records, (long)max_faces);
    G2V_CHECK_LAUNCH();
  }
  return G2V_OK;
}
