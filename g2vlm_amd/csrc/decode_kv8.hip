// FP8 (OCP e4m3fn) KV cache of the persistent-grid decode step: the cache rows are read as one byte per element plus one fp32
// power-of-two scale per (row, kv head) - 132 bytes against 256.  The encoding is g2vlm_amd/quant.py's, applied per cache row and
// kv head:   scale = 2^ceil(log2(amax / 448))  (a zero row: 1),   code = RNE_e4m3fn(x / scale).
// code * scale is exactly a bf16 value, so everything here is the bf16 kernel family on dequant(quant(row)):
//   * kv_quant_e4m3_kernel    bf16 rows -> codes + scales (the copy-in of a prefilled cache),
//   * kv_dequant_e4m3_kernel  codes + scales -> bf16 rows, exact (the copy-out of the appended rows),
//   * decode_attn_pg_kv8_kernel: decode_attn_pg_body (decode_attn_pg.h) instantiated with the cache-format policy KvE4m3 below:
//     8-byte K / V loads, converted in registers by v_cvt_scalef32_pk_bf16_fp8 with the row's scale as the scale operand (a
//     lane's K fragment is one key, each of its V staging loads one row: one scale each).  After the conversion the registers
//     hold the dequantised bf16 rows; everything else is the one body the bf16 kernel has.  The new token's K row (after
//     norm and rotation, bf16-rounded as there) and V row are quantised in the kernel, written to cache row Lk - 1 as codes +
//     scale, and enter this step's scores and P.V as their DEQUANTISED values: a later step reads what this step used.
// The workspace, the block count rule and the combine kernel are g2v_decode_attn_pg's.
#include "common.h"
#include "decode_util.h"
#include "decode_attn_pg.h"
#include "g2vlm_hip.h"

namespace {

// 2^ceil(log2(amax / 448)) from the float's bits: for amax = m 2^E, m in [1, 2), amax / 448 = (m / 1.75) 2^(E - 8), so the
// exponent is E - 8 if m <= 1.75 and E - 7 otherwise; clamped to a normal fp32 number as the host quantiser clamps it.
__device__ __forceinline__ float kv8_scale(float amax) {
  const uint32_t b = __float_as_uint(amax);
  const int e = max((int)(b >> 23) - ((b & 0x7fffffu) <= 0x600000u ? 8 : 7), 1);
  return amax > 0.f ? __uint_as_float((uint32_t)e << 23) : 1.0f;
}
__device__ __forceinline__ float kv8_inv(float scale) {        // 1 / scale, exact: scale = 2^(e - 127), 1 <= e <= 247
  return __uint_as_float((254u << 23) - __float_as_uint(scale));
}
// four values (already divided by the scale: |x| <= 448, so no NaN code) -> four e4m3fn codes, round to nearest even
__device__ __forceinline__ uint32_t kv8_pack4(float a, float b, float c, float d) {
  int r = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  r = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, r, true);
  return (uint32_t)r;
}
__device__ __forceinline__ uint32_t kv8_lo(uint32_t w, float s) {      // bytes 0, 1 of w times s -> packed bf16 pair
  const bf2_t v = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, s, false);
  return *reinterpret_cast<const uint32_t*>(&v);
}
__device__ __forceinline__ uint32_t kv8_hi(uint32_t w, float s) {      // bytes 2, 3
  const bf2_t v = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, s, true);
  return *reinterpret_cast<const uint32_t*>(&v);
}
__device__ __forceinline__ u32x4 kv8_deq8(u32x2 c, float s) {          // 8 codes -> 8 bf16
  return u32x4{kv8_lo(c[0], s), kv8_hi(c[0], s), kv8_lo(c[1], s), kv8_hi(c[1], s)};
}
__device__ __forceinline__ float absbits(float x) { return __uint_as_float(__float_as_uint(x) & 0x7fffffffu); }

// 8 bf16 of one (row, head) per lane, 16 lanes per (row, head): amax over the 16 lanes, the scale, the lane's 8 codes
__device__ __forceinline__ u32x2 kv8_quant8(u32x4 v, float& scale) {
  float x[8];
#pragma unroll
  for (int e = 0; e < 4; ++e) { x[2 * e] = bits2f_lo(v[e]); x[2 * e + 1] = bits2f_hi(v[e]); }
  float am = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) am = fmaxf(am, absbits(x[e]));
  am = row16_max(am);
  scale = kv8_scale(am);
  const float inv = kv8_inv(scale);
  return u32x2{kv8_pack4(x[0] * inv, x[1] * inv, x[2] * inv, x[3] * inv), kv8_pack4(x[4] * inv, x[5] * inv, x[6] * inv, x[7] * inv)};
}

// src bf16 [n, 128] (n = rows * Hkv) -> codes uint8 [n, 128], scales f32 [n].  256 threads = 16 (row, head) items.
__global__ __launch_bounds__(256) void kv_quant_e4m3_kernel(const __bf16* src, long n, uint8_t* codes, float* scales) {
  const long item = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int j = threadIdx.x & 15;
  const long it = item < n ? item : n - 1;                  // every lane of a 16-lane row takes part in the reduction
  const u32x4 v = *reinterpret_cast<const u32x4*>(src + it * 128 + 8 * j);
  float s;
  const u32x2 c = kv8_quant8(v, s);
  if (item < n) {
    *reinterpret_cast<u32x2*>(codes + item * 128 + 8 * j) = c;
    if (j == 0) scales[item] = s;
  }
}

__global__ __launch_bounds__(256) void kv_dequant_e4m3_kernel(const uint8_t* codes, const float* scales, long n, __bf16* out) {
  const long item = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int j = threadIdx.x & 15;
  if (item >= n) return;
  const u32x2 c = *reinterpret_cast<const u32x2*>(codes + item * 128 + 8 * j);
  *reinterpret_cast<u32x4*>(out + item * 128 + 8 * j) = kv8_deq8(c, scales[item]);
}

// Cache-format policy of decode_attn_pg_body (decode_attn_pg.h: KvBf16 is its bf16 twin), e4m3 codes + one scale per (row, kv head).
// The batch stays in registers as codes - half the registers of the bf16 kernel's, and what is live across the softmax while the
// next batch loads - and becomes bf16 fragments by v_cvt_scalef32_pk_bf16_fp8 right before its MFMAs.
struct KvE4m3 {
  uint8_t *krows, *vrows;                                    // row 0 of this kv head: codes, 128 bytes per (row, head)
  float *ksc, *vsc;                                          // and its scales
  int Hkv, last_row, lane;
  u32x2 kq[8], vq[8], vnq;                                   // K of key r32 / V of rows 4 i + fg / the new V row, as codes
  float ksl, vsl[8], vns;                                    // their scales
  uint32_t kn0, kn1; float kns;                              // the new K row: lane j's codes of elements 4 j .., 64 + 4 j .., its scale
  __device__ __forceinline__ KvE4m3(const void* kc, const void* vc, float* ks, float* vs, const size_t row0, const int kvh, const int Hkv_,
                                    const int last_row_, const int lane_)
      : krows((uint8_t*)kc + (row0 * Hkv_ + kvh) * 128), vrows((uint8_t*)vc + (row0 * Hkv_ + kvh) * 128), ksc(ks + row0 * Hkv_ + kvh),
        vsc(vs + row0 * Hkv_ + kvh), Hkv(Hkv_), last_row(last_row_), lane(lane_) {}
  __device__ __forceinline__ void load_batch(const int k0) {
    const int rk = min(k0 + (lane & 31), last_row);
    const uint8_t* kp = krows + 8 * (lane >> 5) + (size_t)rk * Hkv * 128;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) kq[ks] = *reinterpret_cast<const u32x2*>(kp + 16 * ks);
    ksl = ksc[(size_t)rk * Hkv];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int rv = min(k0 + 4 * i + (lane >> 4), last_row);
      vq[i] = *reinterpret_cast<const u32x2*>(vrows + 8 * (lane & 15) + (size_t)rv * Hkv * 128);
      vsl[i] = vsc[(size_t)rv * Hkv];
    }
  }
  template <class F>
  __device__ __forceinline__ void with_k_bf16(const bool new_batch, const int local, const __bf16* knew, F&& f) {   // see KvBf16
    if (new_batch) {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (4 * i + (lane >> 4) == local) { vq[i] = vnq; vsl[i] = vns; }
    }
    bf16x8 k[8];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const u32x4 kv = kv8_deq8(kq[ks], ksl);
      k[ks] = *reinterpret_cast<const bf16x8*>(&kv);
    }
    if (new_batch && (lane & 31) == local) {                 // the strip holds the new K row as its dequantised value
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) k[ks] = *reinterpret_cast<const bf16x8*>(knew + 16 * ks);
    }
    f(k);
  }
  __device__ __forceinline__ u32x4 v_bf16(const int i) const { return kv8_deq8(vq[i], vsl[i]); }
  // the new token's rows are quantised here and enter this step's scores and P.V as their DEQUANTISED values
  __device__ __forceinline__ void set_new_v(const u32x4 v) { vnq = kv8_quant8(v, vns); }
  __device__ __forceinline__ void quant_k(u32x2& p0, u32x2& p1, const bool isq) {      // every group computes, the k row's group keeps
    float am = 0.f;
#pragma unroll
    for (int e = 0; e < 2; ++e)
      am = fmaxf(fmaxf(am, fmaxf(absbits(bits2f_lo(p0[e])), absbits(bits2f_hi(p0[e])))), fmaxf(absbits(bits2f_lo(p1[e])), absbits(bits2f_hi(p1[e]))));
    am = row16_max(am);
    kns = kv8_scale(am);
    const float inv = kv8_inv(kns);
    kn0 = kv8_pack4(bits2f_lo(p0[0]) * inv, bits2f_hi(p0[0]) * inv, bits2f_lo(p0[1]) * inv, bits2f_hi(p0[1]) * inv);
    kn1 = kv8_pack4(bits2f_lo(p1[0]) * inv, bits2f_hi(p1[0]) * inv, bits2f_lo(p1[1]) * inv, bits2f_hi(p1[1]) * inv);
    if (!isq) {
      p0 = u32x2{kv8_lo(kn0, kns), kv8_hi(kn0, kns)};
      p1 = u32x2{kv8_lo(kn1, kns), kv8_hi(kn1, kns)};
    }
  }
  __device__ __forceinline__ void store_k(const int row, u32x2, u32x2) const {
    uint8_t* krow = krows + (size_t)row * Hkv * 128 + 4 * (lane & 15);
    *reinterpret_cast<uint32_t*>(krow) = kn0;
    *reinterpret_cast<uint32_t*>(krow + 64) = kn1;
    if ((lane & 15) == 0) ksc[(size_t)row * Hkv] = kns;
  }
  __device__ __forceinline__ void store_v(const int row) const {                 // lanes fg == 0
    *reinterpret_cast<u32x2*>(vrows + (size_t)row * Hkv * 128 + 8 * (lane & 15)) = vnq;
    if ((lane & 15) == 0) vsc[(size_t)row * Hkv] = vns;
  }
};

__global__ __launch_bounds__(256, 2) void decode_attn_pg_kv8_kernel(AttnArgs a G2V_STAMP_ARG) {
  __shared__ AttnLds lds;
  decode_attn_pg_body<KvE4m3>(a, lds, blockIdx.x, blockIdx.y, blockIdx.z, gridDim.x, threadIdx.x G2V_STAMP_PASS_DEV);
}

}  // namespace

extern "C" int g2v_kv_quant_e4m3(const void* src, int64_t rows, int Hkv, void* codes, void* scales, void* stream) {
  if (!src || !codes || !scales || rows <= 0 || Hkv <= 0 || Hkv > 128 || rows * Hkv > ((int64_t)1 << 34)) return G2V_ERR_ARG;
  const int64_t n = rows * Hkv;
  hipLaunchKernelGGL(kv_quant_e4m3_kernel, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, (hipStream_t)stream, (const __bf16*)src, (long)n,
                     (uint8_t*)codes, (float*)scales);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

extern "C" int g2v_kv_dequant_e4m3(const void* codes, const void* scales, int64_t rows, int Hkv, void* out, void* stream) {
  if (!codes || !scales || !out || rows <= 0 || Hkv <= 0 || Hkv > 128 || rows * Hkv > ((int64_t)1 << 34)) return G2V_ERR_ARG;
  const int64_t n = rows * Hkv;
  hipLaunchKernelGGL(kv_dequant_e4m3_kernel, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)codes,
                     (const float*)scales, (long)n, (__bf16*)out);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

// g2v_decode_attn_pg on an e4m3 cache: k_cache / v_cache are codes uint8 [batch, scene_rows, Hkv, 128], k_scale / v_scale the
// fp32 power-of-two scales [batch, scene_rows, Hkv].  Same workspace, same block count rule, same argument errors, same combine.
extern "C" int g2v_decode_attn_pg_kv8(const void* qkv, const void* q_norm_w, const void* k_norm_w, float eps, int und_rounding,
                                      const void* cos, const void* sin, void* k_cache, void* v_cache, void* k_scale, void* v_scale,
                                      void* out, const void* Lk_dev, int batch, int64_t scene_rows, int max_len, int Hq, int Hkv,
                                      float scale, void* workspace, void* stream) {
  if (!qkv || !q_norm_w || !k_norm_w || !cos || !sin || !k_cache || !v_cache || !k_scale || !v_scale || !out || !workspace || !Lk_dev ||
      batch <= 0 || batch > 65535 || max_len <= 0 || scene_rows < max_len || Hq <= 0 || Hkv <= 0 || Hkv > 128 || Hq % Hkv || Hq / Hkv > GMAX)
    return G2V_ERR_ARG;
  const int nbh = decode_attn_pg_nbh(Hkv, batch);
  AttnArgs a{(const __bf16*)qkv, (const float*)q_norm_w, (const float*)k_norm_w, (const float*)cos, (const float*)sin, eps, und_rounding,
             k_cache, v_cache, (float*)workspace, (const int*)Lk_dev, Hq, Hkv, scale,
             (long)scene_rows, max_len, (max_len + nbh - 1) / nbh, ((max_len + nbh - 1) / nbh + 3) / 4, (float*)k_scale, (float*)v_scale};
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(decode_attn_pg_kv8_kernel, dim3(nbh, Hkv, batch), dim3(256), 0, s, a G2V_STAMP_PASS_NONE);
  G2V_CHECK_LAUNCH();
  hipLaunchKernelGGL(decode_combine_pg_kernel, dim3(Hq, batch), dim3(1024), 0, s, (const float*)workspace, (__bf16*)out, nbh);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}
