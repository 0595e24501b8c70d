// FP8 (OCP e4m3fn) weight-only forms of the decode step's persistent-grid GEMVs (decode_layer.hip, decode_batch.hip).
//
// W[n][k] = e4m3(Wq[n][k]) * wscale[n] with wscale[n] a power of two (g2vlm_amd/quant.py), so every weight is exactly a bf16
// value and the kernels below are, up to the order of the fp32 partial sums, the bf16 kernels on the dequantised matrix: the
// same grid (256 blocks, every wave an equal contiguous share of the rows), the same issue order (activation side first,
// every load of a batch before anything waits), the same fused RMSNorm / SwiGLU / bias / residual with the same rounding
// points.  What changes is the weight stream: a 16-byte non-temporal load now carries 16 consecutive k, so a lane owns two
// 16-byte activation words per chunk and a row costs half the registers - the batches are deeper (12 rows at K <= 2048, two
// rows at K = 8960 where the bf16 kernel holds one), and the batched kernel pairs rows so that no pass of a wave is half empty.
// Conversion: v_cvt_scalef32_pk_bf16_fp8 with scale 1.0 turns a byte pair into the packed bf16 pair v_dot2c_f32_bf16 takes
// (every e4m3 value is a normal bf16 number): 8 conversions + 8 dot2c per 16-byte load, converted once per weight word
// whatever the number of scenes.  The row's scale multiplies the finished fp32 row sum once, before the bias and the
// rounding: a power of two commutes with every rounding of the sum, so this IS the sum over the dequantised weights.
#include "common.h"
#include "decode_util.h"
#include "decode_dispatch.h"
#include "g2vlm_hip.h"

namespace {

__device__ __forceinline__ uint32_t cvt8_lo(uint32_t w) {      // bytes 0, 1 of w -> packed bf16 pair
  const bf2_t v = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, false);
  return *reinterpret_cast<const uint32_t*>(&v);
}
__device__ __forceinline__ uint32_t cvt8_hi(uint32_t w) {      // bytes 2, 3
  const bf2_t v = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, true);
  return *reinterpret_cast<const uint32_t*>(&v);
}

// Qwen2RMSNorm of 16 consecutive elements of the fp32 residual row -> 8 packed bf16 pairs (rounding points of gemv_pg_kernel)
__device__ __forceinline__ void norm_pack16(const f32x4 (&a)[4], const f32x4 (&nw)[4], float rstd, uint32_t (&p)[8]) {
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int e = 0; e < 2; ++e)
      p[2 * q + e] = pack_bf16x2(__fmul_rn(nw[q][2 * e], __fmul_rn(a[q][2 * e], rstd)), __fmul_rn(nw[q][2 * e + 1], __fmul_rn(a[q][2 * e + 1], rstd)));
}

// sum of squares of the fp32 residual row, in the lane layout and the order of the bf16 kernels (lane l: 8-element chunks
// l, l + 64, l + 128): rstd, and with it the normalised bf16 row, is bit-identical to gemv_pg_kernel's / gemv_pgb_kernel's.
// The row is read a second time for this (6 KB, the same cache lines as the 16-element fragments).
struct NormRow { f32x4 a[3][2]; };
__device__ __forceinline__ void norm_row_load(NormRow& r, const float* xf, int lane, int K) {
  const int nch8 = K >> 3;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int c = min(lane + 64 * j, nch8 - 1);
    r.a[j][0] = *reinterpret_cast<const f32x4*>(xf + 8 * c);
    r.a[j][1] = *reinterpret_cast<const f32x4*>(xf + 8 * c + 4);
  }
}
__device__ __forceinline__ float norm_row_rstd(const NormRow& r, int lane, int K, float eps) {
  const int nch8 = K >> 3;
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    if (lane + 64 * j < nch8) {
#pragma unroll
      for (int e = 0; e < 4; ++e) ss += r.a[j][0][e] * r.a[j][0][e] + r.a[j][1][e] * r.a[j][1][e];
    }
  }
  ss = wave_sum_dpp(ss);
  return 1.0f / sqrtf(ss / (float)K + eps);
}

// ---- batch 1 ---------------------------------------------------------------------------------------------------------------
// gemv_pg_kernel (decode_layer.hip) with e4m3 weights.  KCH = ceil(K / 1024) chunk steps per lane (a chunk is 16 k);
// RB = units per batch.  Lane l takes chunks l, l + 64, ...; chunks past K / 16 multiply a zero activation.
template <int XMODE, bool ACT, int KCH, int RB>
__global__ __launch_bounds__(512) void gemv_pg8_kernel(const void* xin, const float* norm_w, float eps, const uint8_t* W, const float* wscale,
                                                       const __bf16* bias, __bf16* out, float* res, int N, int K, int uq, int ur) {
  constexpr int ROWS = ACT ? 2 * RB : RB;
  const int lane = threadIdx.x & 63;
  const int nwb = blockDim.x >> 6;
  const int gw = blockIdx.x * nwb + (threadIdx.x >> 6);
  const int lo = gw * uq + min(gw, ur), hi = lo + uq + (gw < ur ? 1 : 0);
  if (lo >= hi) return;
  const int nch = K >> 4;
  auto row_of = [&](int u, int half) { return ACT ? 32 * (u >> 4) + (u & 15) + 16 * half : u; };
  // the RB row sums of a batch are reduced together (reduce_transpose, V - 1 exchange-adds instead of 11 instructions per
  // row): lane l ends up with unit number l >> SH
  constexpr int VP = g2v_pow2_ge(RB), SH = 6 - g2v_log2(VP);
  const int vi = lane >> SH;
  const bool rep = (lane & ((1 << SH) - 1)) == 0 && vi < RB;

  u32x4 ww[ROWS][KCH];
  unsigned short bnext = 0;
  float rnext = 0.f, snext = 1.f, snext2 = 1.f;               // the finishing lane's row scale (ACT: gate and up rows)
  auto issue = [&](int u0) {
    const int nrow = min(RB, hi - u0);                      // wave-uniform
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      if (r < nrow) {
#pragma unroll
        for (int h = 0; h < (ACT ? 2 : 1); ++h) {
          const u32x4* wp = reinterpret_cast<const u32x4*>(W + (size_t)row_of(u0 + r, h) * K);
#pragma unroll
          for (int j = 0; j < KCH; ++j) ww[(ACT ? 2 * r + h : r)][j] = __builtin_nontemporal_load(wp + min(lane + 64 * j, nch - 1));
        }
      }
    }
    const int u = min(u0 + vi, hi - 1);
    snext = wscale[row_of(u, 0)];
    if constexpr (ACT) {
      snext2 = wscale[row_of(u, 1)];
    } else {
      if (bias) bnext = reinterpret_cast<const unsigned short*>(bias)[u];
      if (res) rnext = res[u];
    }
  };

  uint32_t xp[KCH][8];
  if constexpr (XMODE == 0) {
    u32x4 xv[KCH][2];
#pragma unroll
    for (int j = 0; j < KCH; ++j) {
      const int c = min(lane + 64 * j, nch - 1);
      xv[j][0] = reinterpret_cast<const u32x4*>(xin)[2 * c];
      xv[j][1] = reinterpret_cast<const u32x4*>(xin)[2 * c + 1];
    }
    issue(lo);
#pragma unroll
    for (int j = 0; j < KCH; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) xp[j][e] = lane + 64 * j < nch ? xv[j][e >> 2][e & 3] : 0u;
  } else {
    const float* xf = reinterpret_cast<const float*>(xin);
    f32x4 a[KCH][4], nwv[KCH][4];
    NormRow nr;
    norm_row_load(nr, xf, lane, K);
#pragma unroll
    for (int j = 0; j < KCH; ++j) {
      const int c = min(lane + 64 * j, nch - 1);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        a[j][q] = *reinterpret_cast<const f32x4*>(xf + 16 * c + 4 * q);
        nwv[j][q] = *reinterpret_cast<const f32x4*>(norm_w + 16 * c + 4 * q);
      }
    }
    issue(lo);
    const float rstd = norm_row_rstd(nr, lane, K, eps);
#pragma unroll
    for (int j = 0; j < KCH; ++j) {
      uint32_t p[8];
      norm_pack16(a[j], nwv[j], rstd, p);
#pragma unroll
      for (int e = 0; e < 8; ++e) xp[j][e] = lane + 64 * j < nch ? p[e] : 0u;
    }
  }

  for (int u0 = lo; u0 < hi; u0 += RB) {
    const int nrow = min(RB, hi - u0);
    if constexpr (KCH > 4) {                                 // long rows: one batch fills the register file, no look-ahead
      if (u0 > lo) issue(u0);
    }
    const float bcur = __uint_as_float((uint32_t)bnext << 16), rcur = rnext, scur = snext, scur2 = snext2;
    float acc[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      acc[r] = 0.f;
      if ((ACT ? r / 2 : r) < nrow) {
#pragma unroll
        for (int j = 0; j < KCH; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            acc[r] = dot2(cvt8_lo(ww[r][j][e]), xp[j][2 * e], acc[r]);
            acc[r] = dot2(cvt8_hi(ww[r][j][e]), xp[j][2 * e + 1], acc[r]);
          }
      }
    }
    if constexpr (KCH <= 4) {
      if (u0 + RB < hi) issue(u0 + RB);                    // next batch in flight under this batch's reduction
    }
    float va[VP], vb[ACT ? VP : 1];
#pragma unroll
    for (int i = 0; i < VP; ++i) {
      va[i] = i < RB ? acc[ACT ? 2 * i : i] : 0.f;
      if constexpr (ACT) vb[i] = i < RB ? acc[2 * i + 1] : 0.f;
    }
    float v = reduce_transpose<VP>(va, lane);
    if constexpr (ACT) {
      const float u = reduce_transpose<VP>(vb, lane);
      if (rep && vi < nrow) out[u0 + vi] = f2bf(bfround(siluf_(bfround(__fmul_rn(v, scur)))) * bfround(__fmul_rn(u, scur2)));
    } else {
      if (rep && vi < nrow) {
        const int n = u0 + vi;
        v = bfround(__fmul_rn(v, scur) + bcur);
        if (res) res[n] = rcur + v;
        else out[n] = f2bf(v);
      }
    }
  }
}

// ---- B <= 8 scenes, K <= 1536 --------------------------------------------------------------------------------------------------
// gemv_pgb_kernel (decode_batch.hip) with e4m3 weights: the B rows are normalised once per block into an LDS strip (fused-norm
// form), a weight word is converted once and multiplied with the NB scenes' activation words.
// A row of K <= 1536 is at most 96 chunks: one and a half passes of a wave.  With B = 8 the kernel is bound by its VALU work
// (72 instructions per 16-byte word), so a half-empty pass is a third of the time wasted; a unit is therefore a PAIR of rows
// (rows 2u, 2u + 1; for ACT the gate row and the up row of one output) streamed in three full passes:
//   slot 0: row A, chunk lane        slot 1: lanes 0-31 row A, lanes 32-63 row B, chunk 64 + (lane & 31)        slot 2: row B, chunk lane
// Slot 1 is accumulated first and handed to row A's sum in the low half-wave and to row B's in the high one.
template <int XMODE, bool ACT, int NB, int RB>
__global__ __launch_bounds__(512) void gemv_pgb8_kernel(const void* xin, const float* norm_w, float eps, const uint8_t* W, const float* wscale,
                                                        const __bf16* bias, __bf16* out, float* res, int B, int N, int K, int uq, int ur) {
  static_assert(NB * RB <= 32, "the batch's values are reduced together");
  __shared__ __attribute__((aligned(16))) uint32_t sx[XMODE == 1 ? NB * 768 : 4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const bool upper = lane >= 32;
  // wave w of block b is wave number w * 256 + b of the grid: when there are fewer units than waves (qkv, o: one pair for
  // every second wave) every CU still gets its share, on as many SIMDs as it has units
  const int gw = w * gridDim.x + blockIdx.x;
  const int lo = gw * uq + min(gw, ur), hi = lo + uq + (gw < ur ? 1 : 0);   // may be empty: the wave still stages its x row
  const int nch = K >> 4;
  const int No = ACT ? N / 2 : N;
  // rows of unit u; an odd N leaves the last unit without its second row: it re-reads the first (never stored)
  auto row_of = [&](int u, int half) { return ACT ? 32 * (u >> 4) + (u & 15) + 16 * half : min(2 * u + half, N - 1); };
  constexpr int NV = NB * RB, VP = g2v_pow2_ge(NV), SH = 6 - g2v_log2(VP);
  const int vi = lane >> SH;
  const bool rep = (lane & ((1 << SH) - 1)) == 0 && vi < NV;
  const int lb = vi / RB, lr = vi - lb * RB;               // the (scene, unit) this lane finishes
  const int c0 = min(lane, nch - 1), c1 = min(64 + (lane & 31), nch - 1);
  const bool live0 = lane < nch, live1 = 64 + (lane & 31) < nch;

  u32x4 ww[RB][3];
  unsigned short bnext[2] = {0, 0};
  float rnext[2] = {0.f, 0.f}, snext[2] = {1.f, 1.f};
  auto issue = [&](int u0) {
    const int nrow = min(RB, hi - u0);
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      if (r < nrow) {
        const u32x4* wa = reinterpret_cast<const u32x4*>(W + (size_t)row_of(u0 + r, 0) * K);
        const u32x4* wb = reinterpret_cast<const u32x4*>(W + (size_t)row_of(u0 + r, 1) * K);
        ww[r][0] = __builtin_nontemporal_load(wa + c0);
        ww[r][1] = __builtin_nontemporal_load((upper ? wb : wa) + c1);
        ww[r][2] = __builtin_nontemporal_load(wb + c0);
      }
    }
    const int u = min(u0 + lr, hi - 1), b = min(lb, B - 1);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int n = row_of(u, h);
      snext[h] = wscale[n];
      if constexpr (!ACT) {
        if (bias) bnext[h] = reinterpret_cast<const unsigned short*>(bias)[n];
        if (res) rnext[h] = res[(size_t)b * N + n];
      }
    }
  };

  uint32_t xp[NB][2][8];
  if constexpr (XMODE == 0) {
    if (lo >= hi) return;                                    // nothing below synchronises
    u32x4 xv[NB][2][2];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const u32x4* xr = reinterpret_cast<const u32x4*>(reinterpret_cast<const __bf16*>(xin) + (size_t)min(b, B - 1) * K);
      xv[b][0][0] = xr[2 * c0]; xv[b][0][1] = xr[2 * c0 + 1];
      xv[b][1][0] = xr[2 * c1]; xv[b][1][1] = xr[2 * c1 + 1];
    }
    if (lo < hi) issue(lo);
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        xp[b][0][e] = live0 ? xv[b][0][e >> 2][e & 3] : 0u;
        xp[b][1][e] = live1 ? xv[b][1][e >> 2][e & 3] : 0u;
      }
  } else {
    // wave b normalises row b into the strip (rows past B: the last row again, never stored) in the lane layout and order
    // of gemv_pgb_kernel - 8-element chunks lane, lane + 64, lane + 128 - so rstd and the normalised bf16 row are that
    // kernel's bit for bit; the strip is the row in order, whatever layout wrote it
    const int nch8 = K >> 3;
    const float* xf = reinterpret_cast<const float*>(xin) + (size_t)min(w, B - 1) * K;
    NormRow nr;
    f32x4 nwv[3][2];
    if (w < NB) {
      norm_row_load(nr, xf, lane, K);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int c = min(lane + 64 * j, nch8 - 1);
        nwv[j][0] = *reinterpret_cast<const f32x4*>(norm_w + 8 * c);
        nwv[j][1] = *reinterpret_cast<const f32x4*>(norm_w + 8 * c + 4);
      }
    }
    if (lo < hi) issue(lo);
    if (w < NB) {
      const float rstd = norm_row_rstd(nr, lane, K, eps);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        if (lane + 64 * j < nch8) {
          u32x4 p;
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            p[e] = pack_bf16x2(__fmul_rn(nwv[j][0][2 * e], __fmul_rn(nr.a[j][0][2 * e], rstd)),
                               __fmul_rn(nwv[j][0][2 * e + 1], __fmul_rn(nr.a[j][0][2 * e + 1], rstd)));
            p[2 + e] = pack_bf16x2(__fmul_rn(nwv[j][1][2 * e], __fmul_rn(nr.a[j][1][2 * e], rstd)),
                                   __fmul_rn(nwv[j][1][2 * e + 1], __fmul_rn(nr.a[j][1][2 * e + 1], rstd)));
          }
          *reinterpret_cast<u32x4*>(&sx[w * 768 + 4 * (lane + 64 * j)]) = p;
        }
      }
    }
    __syncthreads();
    if (lo < hi) {                                           // a wave without rows reads nothing back
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const uint32_t* s0 = &sx[b * 768 + 8 * c0];
        const uint32_t* s1 = &sx[b * 768 + 8 * c1];
        const u32x4 v0 = *reinterpret_cast<const u32x4*>(s0), v1 = *reinterpret_cast<const u32x4*>(s0 + 4);
        const u32x4 v2 = *reinterpret_cast<const u32x4*>(s1), v3 = *reinterpret_cast<const u32x4*>(s1 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          xp[b][0][e] = live0 ? v0[e] : 0u;
          xp[b][0][4 + e] = live0 ? v1[e] : 0u;
          xp[b][1][e] = live1 ? v2[e] : 0u;
          xp[b][1][4 + e] = live1 ? v3[e] : 0u;
        }
      }
    }
  }

  for (int u0 = lo; u0 < hi; u0 += RB) {
    const int nrow = min(RB, hi - u0);
    const float bcur[2] = {__uint_as_float((uint32_t)bnext[0] << 16), __uint_as_float((uint32_t)bnext[1] << 16)};
    const float rcur[2] = {rnext[0], rnext[1]}, scur[2] = {snext[0], snext[1]};
    float accA[NB][RB], accB[NB][RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      if (r < nrow) {
        float m[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) m[b] = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {                        // slot 1 first: the shared pass
          const uint32_t wl = cvt8_lo(ww[r][1][e]), wh = cvt8_hi(ww[r][1][e]);   // once per weight word, not per scene
#pragma unroll
          for (int b = 0; b < NB; ++b) {
            m[b] = dot2(wl, xp[b][1][2 * e], m[b]);
            m[b] = dot2(wh, xp[b][1][2 * e + 1], m[b]);
          }
        }
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          accA[b][r] = upper ? 0.f : m[b];
          accB[b][r] = upper ? m[b] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const uint32_t al = cvt8_lo(ww[r][0][e]), ah = cvt8_hi(ww[r][0][e]);
          const uint32_t bl = cvt8_lo(ww[r][2][e]), bh = cvt8_hi(ww[r][2][e]);
#pragma unroll
          for (int b = 0; b < NB; ++b) {
            accA[b][r] = dot2(al, xp[b][0][2 * e], accA[b][r]);
            accA[b][r] = dot2(ah, xp[b][0][2 * e + 1], accA[b][r]);
            accB[b][r] = dot2(bl, xp[b][0][2 * e], accB[b][r]);
            accB[b][r] = dot2(bh, xp[b][0][2 * e + 1], accB[b][r]);
          }
        }
      } else {
#pragma unroll
        for (int b = 0; b < NB; ++b) { accA[b][r] = 0.f; accB[b][r] = 0.f; }
      }
    }
    if (u0 + RB < hi) issue(u0 + RB);                        // next batch in flight under this batch's reductions
    float va[VP], vb[VP];
#pragma unroll
    for (int i = 0; i < VP; ++i) {
      va[i] = i < NV ? accA[i / RB][i % RB] : 0.f;
      vb[i] = i < NV ? accB[i / RB][i % RB] : 0.f;
    }
    const float sa = reduce_transpose<VP>(va, lane), sb = reduce_transpose<VP>(vb, lane);
    if (rep && lb < B && lr < nrow) {
      if constexpr (ACT) {
        out[(size_t)lb * No + u0 + lr] = f2bf(bfround(siluf_(bfround(__fmul_rn(sa, scur[0])))) * bfround(__fmul_rn(sb, scur[1])));
      } else {
        const int n = 2 * (u0 + lr);
        const float v0 = bfround(__fmul_rn(sa, scur[0]) + bcur[0]), v1 = bfround(__fmul_rn(sb, scur[1]) + bcur[1]);
        if (res) {
          res[(size_t)lb * N + n] = rcur[0] + v0;
          if (n + 1 < N) res[(size_t)lb * N + n + 1] = rcur[1] + v1;
        } else {
          out[(size_t)lb * N + n] = f2bf(v0);
          if (n + 1 < N) out[(size_t)lb * N + n + 1] = f2bf(v1);
        }
      }
    }
  }
}

// ---- B <= 8 scenes, long K -------------------------------------------------------------------------------------------------------
// gemv_pgk_kernel (decode_batch.hip) with e4m3 weights.  A block has one wave per 1024 elements of K (S = ceil(K / 1024)
// waves: 9 at K = 8960, against 8 waves of 1120 with a third of their load slots empty), so a wave's slice is ONE 16-byte
// weight load per lane and row and 8 activation registers per scene; block `blk` owns rows [blk per, (blk + 1) per) and
// streams them R at a time (8 rows up to four scenes, 4 rows at eight: R x NB <= 32 values are reduced together; the bf16
// kernel holds 6 rows).  A weight word is converted once for all scenes.  Partial sums meet in LDS, added in wave order.
constexpr int PGK8_SMAX = 12;
template <int NB>
__global__ __launch_bounds__(64 * PGK8_SMAX) void gemv_pgk8_kernel(const __bf16* x, const uint8_t* W, const float* wscale, const __bf16* bias,
                                                                    __bf16* out, float* res, int B, int N, int K, int per) {
  constexpr int R = NB == 8 ? 4 : 8;
  __shared__ float part[PGK8_SMAX][NB][R];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, tid = threadIdx.x, S = blockDim.x >> 6;
  const int nch = K >> 4;
  const int c = 64 * w + lane;
  const bool live = c < nch;
  const int cc = min(c, nch - 1);
  const int row_lo = blockIdx.x * per, row_hi = min(row_lo + per, N);
  uint32_t xp[NB][8];
  u32x4 ww[R];
  auto issue = [&](int r0) {
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (r0 + r < row_hi) ww[r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(W + (size_t)(r0 + r) * K) + cc);
  };
  {
    u32x4 xv[NB][2];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const u32x4* xr = reinterpret_cast<const u32x4*>(x + (size_t)min(b, B - 1) * K);
      xv[b][0] = xr[2 * cc];
      xv[b][1] = xr[2 * cc + 1];
    }
    if (row_lo < row_hi) issue(row_lo);
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int e = 0; e < 8; ++e) xp[b][e] = live ? xv[b][e >> 2][e & 3] : 0u;
  }
  for (int r0 = row_lo; r0 < row_hi; r0 += R) {
    float acc[NB][R];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int r = 0; r < R; ++r) acc[b][r] = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (r0 + r < row_hi) {                                 // block-uniform
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const uint32_t wl = cvt8_lo(ww[r][e]), wh = cvt8_hi(ww[r][e]);
#pragma unroll
          for (int b = 0; b < NB; ++b) {
            acc[b][r] = dot2(wl, xp[b][2 * e], acc[b][r]);
            acc[b][r] = dot2(wh, xp[b][2 * e + 1], acc[b][r]);
          }
        }
      }
    }
    if (r0 + R < row_hi) issue(r0 + R);                      // next batch in flight under the reduction
    {
      constexpr int NV = NB * R, VP = g2v_pow2_ge(NV), SH = 6 - g2v_log2(VP);
      float va[VP];
#pragma unroll
      for (int i = 0; i < VP; ++i) va[i] = i < NV ? acc[i / R][i % R] : 0.f;
      const float s = reduce_transpose<VP>(va, lane);
      const int vi = lane >> SH;
      if ((lane & ((1 << SH) - 1)) == 0 && vi < NV) part[w][vi / R][vi - (vi / R) * R] = s;
    }
    __syncthreads();
    if (tid < NB * R) {
      const int b = tid / R, r = tid - b * R, n = r0 + r;
      if (b < B && n < row_hi) {
        float s = 0.f;
        for (int k = 0; k < S; ++k) s += part[k][b][r];
        const float v = bfround(__fmul_rn(s, wscale[n]) + (bias ? bf2f(bias[n]) : 0.f));
        if (res) res[(size_t)b * N + n] += v;
        else out[(size_t)b * N + n] = f2bf(v);
      }
    }
    __syncthreads();
  }
}

template <int XMODE, bool ACT, int KCH>
int pg8_launch(const pg::Plan& p, hipStream_t s, const void* x, const float* nw, float eps, const uint8_t* W, const float* ws, const __bf16* bias,
               __bf16* out, float* res, int N, int K) {
  pg::with_rb<true, 0, ACT, (KCH > 4)>(p.rb, [&](auto rb) {
    hipLaunchKernelGGL((gemv_pg8_kernel<XMODE, ACT, KCH, decltype(rb)::value>), dim3(256), dim3(p.threads), 0, s, x, nw, eps, W, ws, bias, out,
                       res, N, K, p.uq, p.ur);
  });
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

template <int XMODE, bool ACT, int NB>
int pgb8_launch(const pg::Plan& p, hipStream_t s, const void* x, const float* nw, float eps, const uint8_t* W, const float* ws,
                const __bf16* bias, __bf16* out, float* res, int B, int N, int K) {
  pg::with_rb<true, NB, ACT, false>(p.rb, [&](auto rb) {
    hipLaunchKernelGGL((gemv_pgb8_kernel<XMODE, ACT, NB, decltype(rb)::value>), dim3(256), dim3(512), 0, s, x, nw, eps, W, ws, bias, out, res, B,
                       N, K, p.uq, p.ur);
  });
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

}  // namespace

// g2v_gemv_pg with W[n][k] = e4m3(Wq[n][k]) * wscale[n]: Wq uint8 [N, K] (OCP e4m3fn codes), wscale f32 [N] (powers of two).
// Every other argument, every fused form and every argument error as g2v_gemv_pg; K % 16 == 0, K <= 9216.
extern "C" int g2v_gemv_pg_fp8(const void* x, const void* norm_w, float eps, const void* Wq, const void* wscale, const void* bias, void* out,
                               void* res, int N, int K, int act, void* stream) {
  if (!x || !Wq || !wscale || (!out && !res) || (act && (!out || res))) return G2V_ERR_ARG;
  pg::Plan p;
  if (const int rc = pg::plan(0, N, K, act != 0, norm_w != nullptr, true, p)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const float *nwp = (const float*)norm_w, *wsp = (const float*)wscale;
  const uint8_t* Wp = (const uint8_t*)Wq;
  const __bf16* bp = (const __bf16*)bias;
  if (norm_w) {
    if (act) return pg8_launch<1, true, 2>(p, s, x, nwp, eps, Wp, wsp, bp, (__bf16*)out, (float*)res, N, K);
    return pg8_launch<1, false, 2>(p, s, x, nwp, eps, Wp, wsp, bp, (__bf16*)out, (float*)res, N, K);
  }
  if (p.kch == 2) return pg8_launch<0, false, 2>(p, s, x, nwp, eps, Wp, wsp, bp, (__bf16*)out, (float*)res, N, K);
  return pg8_launch<0, false, 9>(p, s, x, nwp, eps, Wp, wsp, bp, (__bf16*)out, (float*)res, N, K);
}

// g2v_gemv_pg_batch with e4m3 weights (Wq, wscale as g2v_gemv_pg_fp8): B = 1..8 rows, K % 16 == 0, K <= 12288.
extern "C" int g2v_gemv_pg_batch_fp8(const void* x, const void* norm_w, float eps, const void* Wq, const void* wscale, const void* bias,
                                     void* out, void* res, int B, int N, int K, int act, void* stream) {
  if (!x || !Wq || !wscale || (!out && !res) || (act && (!out || res)) || B <= 0) return G2V_ERR_ARG;
  pg::Plan p;
  if (const int rc = pg::plan(B, N, K, act != 0, norm_w != nullptr, true, p)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const uint8_t* Wp = (const uint8_t*)Wq;
  const float *nwp = (const float*)norm_w, *wsp = (const float*)wscale;
  const __bf16* bp = (const __bf16*)bias;
  __bf16* op = (__bf16*)out;
  float* rp = (float*)res;
  if (p.form == 3)                                           // 2..12 waves
    return pg::with_nb(p.nb, [&](auto nb) {
      hipLaunchKernelGGL(gemv_pgk8_kernel<decltype(nb)::value>, dim3(256), dim3(p.threads), 0, s, (const __bf16*)x, Wp, wsp, bp, op, rp, B, N, K, p.per);
      G2V_CHECK_LAUNCH();
      return G2V_OK;
    });
  return pg::with_nb(p.nb, [&](auto nb) {
    constexpr int NB = decltype(nb)::value;
    if (norm_w && act) return pgb8_launch<1, true, NB>(p, s, x, nwp, eps, Wp, wsp, bp, op, rp, B, N, K);
    if (norm_w) return pgb8_launch<1, false, NB>(p, s, x, nwp, eps, Wp, wsp, bp, op, rp, B, N, K);
    return pgb8_launch<0, false, NB>(p, s, x, nwp, eps, Wp, wsp, bp, op, rp, B, N, K);
  });
}
