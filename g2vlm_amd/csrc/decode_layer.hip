// Batch-1 decode step, second generation: every kernel is sized to the chip instead of to the problem.
//
// The step (reference modeling/g2vlm/g2vlm.py:1086-1135: 28 x {q/k/v/o/gate/up/down Linear at M = 1, flash_attn_varlen_func
// with q_len 1} + lm_head) is HBM-bound: 3.09 GB of weights + 28 672 B x Lk of K/V per token.  One CU can pull about
// 1/256 of the HBM rate (MI355X guide: ~10 B/clk/CU), so a kernel streams at the full rate only while ALL 256 CUs hold an
// equal share of its bytes.  The first-generation kernels (decode.hip) size their grids by the problem - 86 workgroups for
// the split-KV attention at Lk = 11 k, 2240 / 768 / 1024 row blocks for the GEMVs - and run at 0.6-3.6 TB/s.  Here:
//   * GEMV: a persistent grid of 256 blocks; the N rows are cut into 256 x NW equal contiguous shares, one per wave.
//     A wave covers the whole K of its rows (lane l takes 16-byte chunks l, l + 64, ...): no LDS, no barrier, the
//     activation vector (normalised on the fly for the fused RMSNorm form) lives in registers for the wave's lifetime.
//   * attention: 256 blocks per scene, each an equal share of ONE kv head's keys; the 4 waves of a block merge their
//     online-softmax partials through LDS, so the combine reads 128 partials per head instead of 172.
// Tried and dropped (profiles/r02d_*): pulling the next Linear's weights into the 256 MiB Infinity Cache under the
// latency-bound kernels.  From the Infinity Cache the 55 MB gate/up GEMV takes 10.4 us instead of 12.1 (a bare read of the
// 55 MB takes 9.9): these kernels are bound by launch ramp and per-CU load throughput, not by HBM, and a prefetch branch in the
// step's graph serialises (+0.6 ms per token).
#include "common.h"
#include "decode_util.h"
#include "decode_attn_pg.h"
#include "decode_dispatch.h"
#include "g2vlm_hip.h"

#ifdef G2V_STAMPS
static unsigned long long* g_stamp_buf = nullptr;
extern "C" int g2v_debug_stamps(void* buf) { g_stamp_buf = (unsigned long long*)buf; return 0; }
#endif

namespace {

// ---- persistent GEMV ---------------------------------------------------------------------------------------------------
// XMODE 0: x bf16[K].   XMODE 1: x = bf16(w_norm * (res * rsqrt(mean(res^2) + eps)))  (Qwen2RMSNorm of the fp32 residual stream).
// ACT: W is a gate/up matrix interleaved per 16 rows (weights.interleave_gate_up); a unit is the pair (gate row, up row) of
//      one output and the kernel writes bf16(bf16(silu(g)) * u).  Otherwise a unit is one row: out[n] = bf16(W[n].x + bias)
//      or res[n] += that.
// KCH = ceil(K / 512) chunk steps per lane; RB = units per batch (all of a batch's loads are issued before the first FMA).
// The activation is kept packed (bf16 pairs) and multiplied with v_dot2c_f32_bf16: 8 FLOP-pairs per 16-byte load cost 4
// instructions, so even K = 8960 (18 chunk steps, 72 registers of x) leaves the wave waiting on memory, not on the VALU.
template <int XMODE, bool ACT, int KCH, int RB>
__global__ __launch_bounds__(512) void gemv_pg_kernel(const void* xin, const float* norm_w, float eps, const __bf16* W,
                                                      const __bf16* bias, __bf16* out, float* res, int N, int K, int uq, int ur G2V_STAMP_ARG) {
  constexpr int ROWS = ACT ? 2 * RB : RB;
  G2V_STAMP_RT(10);
  G2V_STAMP(0);
  const int lane = threadIdx.x & 63;
  const int nwb = blockDim.x >> 6;
  // wave gw of nw takes units [gw uq + min(gw, ur), +uq (+1 if gw < ur)): U = nw uq + ur, split by the host (no division here)
  const int gw = blockIdx.x * nwb + (threadIdx.x >> 6);
  const int lo = gw * uq + min(gw, ur), hi = lo + uq + (gw < ur ? 1 : 0);
  if (lo >= hi) return;
  const int nch = K >> 3;
  auto row_of = [&](int u, int half) { return ACT ? 32 * (u >> 4) + (u & 15) + 16 * half : u; };

  // Every load of the wave's first batch - weights, bias / residual words, activation, norm weights - is issued before
  // anything waits: the kernel is ONE memory round trip, a reduction and a store (a second dependent round trip, e.g.
  // the norm weights fetched behind the rstd reduction, costs ~1 us on a 4 us kernel)
  u32x4 ww[ROWS][KCH];
  unsigned short bnext = 0;                                 // raw bf16 bits: converting at load time would wait for the load
  float rnext = 0.f;
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
    if constexpr (!ACT) {
      const int n = min(u0 + lane, hi - 1);
      if (bias) bnext = reinterpret_cast<const unsigned short*>(bias)[n];
      if (res) rnext = res[n];
    }
  };

  // activation fragment: chunk lane + 64 j, j < KCH (chunks past K/8 are zero).  Its loads go out FIRST: vmcnt retires in
  // issue order, so the norm's reduction can run on them while the (younger) weight loads are still in flight.
  uint32_t xp[KCH][4];
  if constexpr (XMODE == 0) {
    u32x4 xv[KCH];
#pragma unroll
    for (int j = 0; j < KCH; ++j) xv[j] = reinterpret_cast<const u32x4*>(xin)[min(lane + 64 * j, nch - 1)];
    issue(lo);
    G2V_STAMP(1);
#pragma unroll
    for (int j = 0; j < KCH; ++j) {
#pragma unroll
      for (int e = 0; e < 4; ++e) xp[j][e] = lane + 64 * j < nch ? xv[j][e] : 0u;
    }
  } else {
    const float* xf = reinterpret_cast<const float*>(xin);
    f32x4 a[KCH][2], nwv[KCH][2];
#pragma unroll
    for (int j = 0; j < KCH; ++j) {
      const int c = min(lane + 64 * j, nch - 1);
      a[j][0] = *reinterpret_cast<const f32x4*>(xf + 8 * c);
      a[j][1] = *reinterpret_cast<const f32x4*>(xf + 8 * c + 4);
      nwv[j][0] = *reinterpret_cast<const f32x4*>(norm_w + 8 * c);
      nwv[j][1] = *reinterpret_cast<const f32x4*>(norm_w + 8 * c + 4);
    }
    issue(lo);
    G2V_STAMP(1);
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < KCH; ++j) {
      if (lane + 64 * j < nch) {
#pragma unroll
        for (int e = 0; e < 4; ++e) ss += a[j][0][e] * a[j][0][e] + a[j][1][e] * a[j][1][e];
      }
    }
    ss = wave_sum_dpp(ss);
    const float rstd = 1.0f / sqrtf(ss / (float)K + eps);
#pragma unroll
    for (int j = 0; j < KCH; ++j) {
      const bool live = lane + 64 * j < nch;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const uint32_t p0 = pack_bf16x2(__fmul_rn(nwv[j][0][2 * e], __fmul_rn(a[j][0][2 * e], rstd)),
                                        __fmul_rn(nwv[j][0][2 * e + 1], __fmul_rn(a[j][0][2 * e + 1], rstd)));
        const uint32_t p1 = pack_bf16x2(__fmul_rn(nwv[j][1][2 * e], __fmul_rn(a[j][1][2 * e], rstd)),
                                        __fmul_rn(nwv[j][1][2 * e + 1], __fmul_rn(a[j][1][2 * e + 1], rstd)));
        xp[j][e] = live ? p0 : 0u;
        xp[j][2 + e] = live ? p1 : 0u;
      }
    }
  }

  G2V_STAMP(2);
  for (int u0 = lo; u0 < hi; u0 += RB) {
    const int nrow = min(RB, hi - u0);
    if constexpr (KCH > 8) {                                 // long rows: one batch fills the register file, no look-ahead
      if (u0 > lo) issue(u0);
    }
    const float bcur = __uint_as_float((uint32_t)bnext << 16), rcur = rnext;
    float acc[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      acc[r] = 0.f;
      if ((ACT ? r / 2 : r) < nrow) {
#pragma unroll
        for (int j = 0; j < KCH; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[r] = dot2(ww[r][j][e], xp[j][e], acc[r]);
      }
    }
    if constexpr (KCH <= 8) {
      if (u0 + RB < hi) issue(u0 + RB);                    // next batch in flight under this batch's reduction
    }
    if (u0 == lo) G2V_STAMP(3);
#pragma unroll
    for (int r = 0; r < ROWS; ++r) acc[r] = wave_sum_dpp(acc[r]);
    if (u0 == lo) G2V_STAMP(4);
    if constexpr (ACT) {
      float v = 0.f;
#pragma unroll
      for (int r = 0; r < RB; ++r)
        if (lane == r) v = bfround(siluf_(bfround(acc[2 * r]))) * bfround(acc[2 * r + 1]);
      if (lane < nrow) out[u0 + lane] = f2bf(v);
    } else {
      float v = 0.f;
#pragma unroll
      for (int r = 0; r < RB; ++r)
        if (lane == r) v = acc[r];
      if (lane < nrow) {
        const int n = u0 + lane;
        v = bfround(v + bcur);
        if (res) res[n] = rcur + v;
        else out[n] = f2bf(v);
      }
    }
  }
  G2V_STAMP(5);
  G2V_STAMP_RT(11);
}

// ---- persistent split-KV attention (head_dim 128), q/k-norm + mRoPE + cache append folded in ------------------------------
// grid (NBH, Hkv, scenes).  The key axis is cut by the cache CAPACITY, not by the current length: block (b, kvh, z) owns
// keys [b S, (b+1) S), S = ceil(cap / NBH), of kv head kvh and its 4 waves a quarter each, so every address is known at
// launch and ALL loads of the kernel - the wave's first 32-key batch of K and V, the step's q / k / v rows, the RoPE row,
// the norm weights and the length word - leave together: one memory round trip, then arithmetic, then one store.  Keys at
// or past the length are masked after the fact: their scores to -inf, their V rows to zero (cache rows past the length
// may hold anything, NaN included).  With the cache sized in 4096-row buckets 75-100 % of the blocks have keys.
//
// A wave runs alone on its SIMD, so every dependent LDS round trip or cross-lane shuffle is exposed latency (the first
// form of this kernel - scores by 16x16 MFMA, softmax by 16-lane shuffles, P.V by fp32 FMAs fed from an LDS strip - spent
// 17 000 of its 26 000 cycles in such chains, profiles/r02d_decode_stamps.txt).  This form is the prefill kernel's
// (attn.hip) at M = the kv head's G <= 8 query heads:
//   S^T[key][head] = K . Q^T on mfma_f32_32x32x16_bf16 (A = 32 K rows straight from global, B = the normalised query heads
//   from a wave-private LDS strip, columns past G duplicate head G - 1): a lane owns ONE head and 16 of the batch's 32 keys in
//   registers, so the softmax is in-register plus one v_permlane32_swap; the S accumulator is the B operand of
//   O^T += V^T . P^T (guide §3, permuted-k order); V^T fragments come by ds_read_b64_tr_b16 from the V batch staged in LDS in
//   the dual-use image of attn.hip (written with ds_write_b128 from the coalesced loads).  16 MFMAs per 32 keys, no shuffle.
// The four waves' (m, l, o) are merged through LDS and ONE partial per (query head, block) goes to the workspace:
// ws[((z Hq + head) NBH + b) 130 + {m, l, o[128]}].  The arithmetic of the new token's q / k (norm, rotation, rounding) is
// qknorm_mrope_cache_kernel's (norm_rope.hip), its 16-lane sum in the same order (v_add with DPP row_ror 8, 4, 2, 1 == the
// xor butterfly 8, 4, 2, 1): the appended K row and the scores are bit-identical to the separate kernels.
__global__ __launch_bounds__(256, 2) void decode_attn_pg_kernel(AttnArgs a G2V_STAMP_ARG) {
  __shared__ AttnLds lds;
  decode_attn_pg_body<KvBf16>(a, lds, blockIdx.x, blockIdx.y, blockIdx.z, gridDim.x, threadIdx.x G2V_STAMP_PASS_DEV);
}

template <int XMODE, bool ACT, int KCH>
int gemv_pg_launch(const pg::Plan& p, hipStream_t s, const void* x, const float* nw, float eps, const __bf16* W, const __bf16* bias,
                   __bf16* out, float* res, int N, int K) {
  pg::with_rb<false, 0, ACT, (KCH > 8)>(p.rb, [&](auto rb) {
    hipLaunchKernelGGL((gemv_pg_kernel<XMODE, ACT, KCH, decltype(rb)::value>), dim3(256), dim3(p.threads), 0, s, x, nw, eps, W, bias, out,
                       res, N, K, p.uq, p.ur G2V_STAMP_PASS);
  });
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

}  // namespace

// y = W[N,K] . x, batch-1 decode form (reference g2vlm.py:1086-1125, every nn.Linear of the und expert at q_len 1).
//   norm_w != NULL: x is the fp32 residual stream and Qwen2RMSNorm(norm_w, eps) is applied on the fly (modeling_qwen2_vl.py:496-501);
//                   else x is bf16[K].
//   act != 0: W = gate/up interleaved per 16 rows, N = 2F rows; out bf16[F] = bf16(bf16(silu(g)) * u) (modeling_qwen2_vl.py:519-521).
//   res != NULL: res[n] (f32) += bf16(y[n] + bias[n]); else out[n] = that.
// K % 8 == 0, K <= 9216.  The grid is 256 blocks whatever N: see the header of this file; block size and batch depth: decode_dispatch.h.
extern "C" int g2v_gemv_pg(const void* x, const void* norm_w, float eps, const void* W, const void* bias, void* out, void* res, int N,
                           int K, int act, void* stream) {
  if (!x || !W || (!out && !res) || (act && (!out || res))) return G2V_ERR_ARG;
  pg::Plan p;
  if (const int rc = pg::plan(0, N, K, act != 0, norm_w != nullptr, false, p)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const float* nwp = (const float*)norm_w;
  const __bf16 *Wp = (const __bf16*)W, *bp = (const __bf16*)bias;
  if (norm_w) {
    if (act) return gemv_pg_launch<1, true, 3>(p, s, x, nwp, eps, Wp, bp, (__bf16*)out, (float*)res, N, K);
    return gemv_pg_launch<1, false, 3>(p, s, x, nwp, eps, Wp, bp, (__bf16*)out, (float*)res, N, K);
  }
  if (p.kch == 3) return gemv_pg_launch<0, false, 3>(p, s, x, nwp, eps, Wp, bp, (__bf16*)out, (float*)res, N, K);
  return gemv_pg_launch<0, false, 18>(p, s, x, nwp, eps, Wp, bp, (__bf16*)out, (float*)res, N, K);
}

// What the four persistent-grid GEMV entry points would launch for a shape, decided by the code they launch with
// (decode_dispatch.h) and without a device.  B == 0: g2v_gemv_pg / g2v_gemv_pg_fp8; B = 1..8: the batched ones.
// out = {form (1 gemv_pg*, 2 gemv_pgb*, 3 gemv_pgk*), threads per block, RB (form 3: R), KCH (form 3: CW in bf16, S in e4m3)}.
extern "C" int g2v_gemv_pg_route(int B, int N, int K, int act, int norm, int fp8, int32_t out[4]) {
  pg::Plan p;
  if (!out) return G2V_ERR_ARG;
  if (const int rc = pg::plan(B, N, K, act != 0, norm != 0, fp8 != 0, p)) return rc;
  out[0] = p.form; out[1] = p.threads; out[2] = p.rb; out[3] = p.kch;
  return G2V_OK;
}

extern "C" int64_t g2v_decode_attn_pg_workspace(int Hq, int Hkv, int batch) {
  if (Hq <= 0 || Hkv <= 0 || Hkv > 128 || batch <= 0) return 0;
  return (int64_t)batch * Hq * (256 / Hkv > 128 ? 128 : 256 / Hkv) * 130 * 4;
}

// The decode step's attention, persistent-grid form of g2v_decode_attn_fused (same arguments, same results up to the order
// of the fp32 partial sums): see decode_attn_pg_kernel.  workspace >= g2v_decode_attn_pg_workspace(Hq, Hkv, batch) bytes.
extern "C" int g2v_decode_attn_pg(const void* qkv, const void* q_norm_w, const void* k_norm_w, float eps, int und_rounding,
                                  const void* cos, const void* sin, void* k_cache, void* v_cache, void* out, const void* Lk_dev,
                                  int batch, int64_t scene_rows, int max_len, int Hq, int Hkv, float scale, void* workspace,
                                  void* stream) {
  if (!qkv || !q_norm_w || !k_norm_w || !cos || !sin || !k_cache || !v_cache || !out || !workspace || !Lk_dev || batch <= 0 ||
      batch > 65535 || max_len <= 0 || scene_rows < max_len || Hq <= 0 || Hkv <= 0 || Hkv > 128 || Hq % Hkv || Hq / Hkv > GMAX)
    return G2V_ERR_ARG;
  const int nbh = decode_attn_pg_nbh(Hkv, batch);
  AttnArgs a{(const __bf16*)qkv, (const float*)q_norm_w, (const float*)k_norm_w, (const float*)cos, (const float*)sin, eps, und_rounding,
             k_cache, v_cache, (float*)workspace, (const int*)Lk_dev, Hq, Hkv, scale, (long)scene_rows, max_len, (max_len + nbh - 1) / nbh,
             ((max_len + nbh - 1) / nbh + 3) / 4, nullptr, nullptr};
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(decode_attn_pg_kernel, dim3(nbh, Hkv, batch), dim3(256), 0, s, a G2V_STAMP_PASS);
  G2V_CHECK_LAUNCH();
  hipLaunchKernelGGL(decode_combine_pg_kernel, dim3(Hq, batch), dim3(1024), 0, s, (const float*)workspace, (__bf16*)out, nbh);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}
