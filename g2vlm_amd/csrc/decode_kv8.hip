// FP8 (OCP e4m3fn) KV cache of the persistent-grid decode step: the cache rows are read as one byte per element plus one fp32
// power-of-two scale per (row, kv head) - 132 bytes against 256.  The encoding is g2vlm_amd/quant.py's, applied per cache row and
// kv head:   scale = 2^ceil(log2(amax / 448))  (a zero row: 1),   code = RNE_e4m3fn(x / scale).
// code * scale is exactly a bf16 value, so everything here is the bf16 kernel family on dequant(quant(row)):
//   * kv_quant_e4m3_kernel    bf16 rows -> codes + scales (the copy-in of a prefilled cache),
//   * kv_dequant_e4m3_kernel  codes + scales -> bf16 rows, exact (the copy-out of the appended rows),
//   * decode_attn_pg_kv8_kernel: decode_attn_pg_body (decode_attn_pg.h) with 8-byte K / V loads, converted in registers by
//     v_cvt_scalef32_pk_bf16_fp8 with the row's scale as the scale operand (a lane's K fragment is one key, each of its V
//     staging loads one row: one scale each).  After the conversion the registers hold the dequantised bf16 rows; the LDS
//     image, the transposed reads, the MFMAs, the softmax and the merge are the bf16 kernel's.  The new token's K row (after
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

struct Attn8Args {
  const __bf16* qkv; const float* qw; const float* kw; const float* cs; const float* sn; float eps; int und_rounding;
  uint8_t* kc; uint8_t* vc; float* ksc; float* vsc; float* ws; const int* Lk_dev; int Hq, Hkv; float scale; long scene_rows; int cap, S, SW;
};

// decode_attn_pg_body<false, false, 4> on an e4m3 cache: see the header of this file for what differs.
__global__ __launch_bounds__(256, 2) void decode_attn_pg_kv8_kernel(Attn8Args a) {
  __shared__ AttnLds lds;
  auto& sq = lds.sq; auto& sv = lds.sv; auto& wm = lds.wm; auto& wl = lds.wl; auto& wo = lds.wo;
  const int bx = blockIdx.x, kvh = blockIdx.y, z = blockIdx.z, NBH = gridDim.x, tid = threadIdx.x;
  const int Hq = a.Hq, Hkv = a.Hkv, G = Hq / Hkv;
  const __bf16* q = a.qkv + (size_t)z * (Hq + 2 * Hkv) * 128;
  uint8_t* kc = a.kc + (size_t)z * a.scene_rows * Hkv * 128;
  uint8_t* vc = a.vc + (size_t)z * a.scene_rows * Hkv * 128;
  float* ksc = a.ksc + (size_t)z * a.scene_rows * Hkv + kvh;
  float* vsc = a.vsc + (size_t)z * a.scene_rows * Hkv + kvh;
  const int lane = tid & 63, w = tid >> 6;
  {
  const int r32 = lane & 31, hh = lane >> 5;                 // MFMA 32x32: row / column index, k half
  const int fr = lane & 15, fg = lane >> 4;
  const int row_stride = Hkv * 128;                          // elements = bytes
  const int S = a.S, SW = a.SW;                             // keys per block / per wave, by capacity
  const int wlo = bx * S + w * SW;
  const int wcap = min(min(wlo + SW, (bx + 1) * S), a.cap);   // end of this wave's range if the cache were full
  const int last_row = a.cap - 1;
  const uint8_t* kbase = kc + kvh * 128 + 8 * hh;           // A operand: lane (r32, hh) takes K[key r32][16 ks + 8 hh ..]
  const uint8_t* vbase = vc + kvh * 128 + 8 * fr;           // staging: lane (fg, fr) takes V[row 4 i + fg][8 fr ..]

  // ---- every load first, the step's own rows before the cache; rows are clamped to the cache block (always mapped), what
  // lies past the length is masked below
  const int j = lane & 15;
  u32x2 x0r[3], x1r[3];
#pragma unroll
  for (int ps = 0; ps < 3; ++ps) {
    const int item = min(4 * ps + (lane >> 4), G);          // G = the new token's k row
    const int src = 2 * ((item < G ? kvh * G + item : Hq + kvh) * 128 + 4 * j);      // byte offset into the step's qkv row
    x0r[ps] = xch_load<false, u32x2>(q, src);
    x1r[ps] = xch_load<false, u32x2>(q, src + 128);
  }
  const u32x4 vnew = xch_load<false, u32x4>(q, 2 * ((Hq + Hkv + kvh) * 128 + 8 * fr));
  const float* cs = a.cs + (size_t)z * 128;
  const float* sn = a.sn + (size_t)z * 128;
  const f32x4 qw0 = *reinterpret_cast<const f32x4*>(a.qw + 4 * j), qw1 = *reinterpret_cast<const f32x4*>(a.qw + 64 + 4 * j);
  const f32x4 kw0 = *reinterpret_cast<const f32x4*>(a.kw + 4 * j), kw1 = *reinterpret_cast<const f32x4*>(a.kw + 64 + 4 * j);
  const f32x4 c0 = *reinterpret_cast<const f32x4*>(cs + 4 * j), c1 = *reinterpret_cast<const f32x4*>(cs + 64 + 4 * j);
  const f32x4 s0 = *reinterpret_cast<const f32x4*>(sn + 4 * j), s1 = *reinterpret_cast<const f32x4*>(sn + 64 + 4 * j);
  u32x2 kq[8], vq[8];                                        // the batch as codes: half the registers of the bf16 kernel's
  float ksl, vsl[8];                                         // the scale of this lane's key / of its eight V rows
  auto load_batch = [&](int k0) {
    const int rk = min(k0 + r32, last_row);
    const uint8_t* kp = kbase + (size_t)rk * row_stride;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) kq[ks] = *reinterpret_cast<const u32x2*>(kp + 16 * ks);
    ksl = ksc[(size_t)rk * Hkv];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int rv = min(k0 + 4 * i + fg, last_row);
      vq[i] = *reinterpret_cast<const u32x2*>(vbase + (size_t)rv * row_stride);
      vsl[i] = vsc[(size_t)rv * Hkv];
    }
  };
  load_batch(wlo);
  const int Lk = a.Lk_dev[z];

  const int whi = min(wcap, Lk);                            // the wave's real range is [wlo, whi)
  const bool has_new = wlo < whi && whi == Lk;              // it ends with the new token's row (wave-uniform)

  // ---- the new token's V row, quantised (every wave; only the wave that owns the row stores it)
  float vns;
  const u32x2 vnq = kv8_quant8(vnew, vns);

  // ---- q / k norm + rotation of the step's rows: every wave, unconditionally; the k row is quantised and its DEQUANTISED
  // value goes to the strip
#pragma unroll
  for (int ps = 0; ps < 3; ++ps) {
    if (4 * ps < G + 1) {                                   // uniform over the launch
      const int c = 4 * ps + (lane >> 4);
      const int item = min(c, G);                           // what this group loaded above
      const bool isq = item < G;
      const u32x2 a0 = x0r[ps], a1 = x1r[ps];
      float x0[4] = {bits2f_lo(a0[0]), bits2f_hi(a0[0]), bits2f_lo(a0[1]), bits2f_hi(a0[1])};
      float x1[4] = {bits2f_lo(a1[0]), bits2f_hi(a1[0]), bits2f_lo(a1[1]), bits2f_hi(a1[1])};
      float ss = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) ss += x0[e] * x0[e] + x1[e] * x1[e];
      ss = row16_sum(ss);
      const float rstd = 1.0f / sqrtf(ss / 128.f + a.eps);
      const f32x4 w0 = isq ? qw0 : kw0, w1 = isq ? qw1 : kw1;
      float o0[4], o1[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float n0 = __fmul_rn(x0[e], rstd), n1 = __fmul_rn(x1[e], rstd);
        if (a.und_rounding) { n0 = bfround(n0); n1 = bfround(n1); }
        n0 = __fmul_rn(w0[e], n0); n1 = __fmul_rn(w1[e], n1);
        o0[e] = __fadd_rn(__fmul_rn(n0, c0[e]), __fmul_rn(-n1, s0[e]));
        o1[e] = __fadd_rn(__fmul_rn(n1, c1[e]), __fmul_rn(n0, s1[e]));
      }
      u32x2 p0 = {pack_bf16x2(o0[0], o0[1]), pack_bf16x2(o0[2], o0[3])}, p1 = {pack_bf16x2(o1[0], o1[1]), pack_bf16x2(o1[2], o1[3])};
      // quantise the bf16-rounded row (computed by every group, used by the one that holds the k row)
      float am = 0.f;
#pragma unroll
      for (int e = 0; e < 2; ++e)
        am = fmaxf(fmaxf(am, fmaxf(absbits(bits2f_lo(p0[e])), absbits(bits2f_hi(p0[e])))), fmaxf(absbits(bits2f_lo(p1[e])), absbits(bits2f_hi(p1[e]))));
      am = row16_max(am);
      const float ksn = kv8_scale(am), inv = kv8_inv(ksn);
      const uint32_t q0 = kv8_pack4(bits2f_lo(p0[0]) * inv, bits2f_hi(p0[0]) * inv, bits2f_lo(p0[1]) * inv, bits2f_hi(p0[1]) * inv);
      const uint32_t q1 = kv8_pack4(bits2f_lo(p1[0]) * inv, bits2f_hi(p1[0]) * inv, bits2f_lo(p1[1]) * inv, bits2f_hi(p1[1]) * inv);
      if (!isq) {
        p0 = u32x2{kv8_lo(q0, ksn), kv8_hi(q0, ksn)};
        p1 = u32x2{kv8_lo(q1, ksn), kv8_hi(q1, ksn)};
      }
      if (c <= G) {                                          // strip rows 0..G (row G is only read by the wave that owns the new row)
        *reinterpret_cast<u32x2*>(&sq[w][item][4 * j]) = p0;
        *reinterpret_cast<u32x2*>(&sq[w][item][64 + 4 * j]) = p1;
      }
      if (c == G && has_new) {                               // the new token's K row -> cache row Lk - 1 of this scene
        uint8_t* krow = kc + (size_t)(Lk - 1) * row_stride + kvh * 128 + 4 * j;
        *reinterpret_cast<uint32_t*>(krow) = q0;
        *reinterpret_cast<uint32_t*>(krow + 64) = q1;
        if (j == 0) ksc[(size_t)(Lk - 1) * Hkv] = ksn;
      }
    }
  }
  float m_run = -INFINITY, l_run = 0.f;                      // this lane's head (column r32), raw-score units / its half's keys
  f32x16 O[4];                                               // O^T[d = 32 blk + row][head r32]
#pragma unroll
  for (int d = 0; d < 4; ++d)
#pragma unroll
    for (int e = 0; e < 16; ++e) O[d][e] = 0.f;
  const float c2 = a.scale * 1.4426950408889634f;            // p = 2^((s - m) c2)

  if (wlo < whi) {
    __builtin_amdgcn_s_waitcnt(0xC07F);                      // the strip is written and read by this wave only
    __builtin_amdgcn_wave_barrier();
    bf16x8 qf[8];                                            // B operand: Q^T[d = 16 ks + 8 hh + j][head r32]
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(&sq[w][min(r32, G - 1)][16 * ks + 8 * hh]);
    if (has_new && fg == 0) {
      *reinterpret_cast<u32x2*>(vc + (size_t)(Lk - 1) * row_stride + kvh * 128 + 8 * fr) = vnq;
      if (fr == 0) vsc[(size_t)(Lk - 1) * Hkv] = vns;
    }
    char* sV = sv[w];
    // V^T fragment addresses (attn.hip): row 16 s + 8 jj + 4 hh + tq, chunk 4 d + t_ch -> v_lb[jj] + 2048 (2 s + jj) + 512 d
    const int tq = (lane & 15) >> 2, tp = lane & 3;
    const int t_ch = 2 * ((lane >> 4) & 1) + (tp >> 1);
    int v_lb[2];
    v_lb[0] = 64 * (4 * hh + tq) + 16 * (t_ch ^ hh) + 8 * (tp & 1);
    v_lb[1] = v_lb[0] ^ 32;

    for (int k0 = wlo; k0 < whi; k0 += KB) {
      const int nk = min(KB, whi - k0);
      const bool new_batch = has_new && k0 + nk == whi;     // the batch that ends with the new row: the loads above read
      const int new_local = Lk - 1 - k0;                     // whatever the cache row held BEFORE this step
      if (new_batch) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if (4 * i + fg == new_local) { vq[i] = vnq; vsl[i] = vns; }
      }
      // ---- V batch -> bf16 -> LDS image (rows at or past nk as zeros: 0 x NaN must not reach the MFMA)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int row = 4 * i + fg;
        const u32x4 val = row < nk ? kv8_deq8(vq[i], vsl[i]) : u32x4{0u, 0u, 0u, 0u};
        *reinterpret_cast<u32x4*>(sV + v_img_off(row, fr)) = val;
      }
      // ---- K batch -> bf16
      bf16x8 kf[8];
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        const u32x4 kv = kv8_deq8(kq[ks], ksl);
        kf[ks] = *reinterpret_cast<const bf16x8*>(&kv);
      }
      if (new_batch && r32 == new_local) {
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) kf[ks] = *reinterpret_cast<const bf16x8*>(&sq[w][G][16 * ks + 8 * hh]);
      }
      // ---- S^T = K . Q^T: register e of lane (r32, hh) is S[key (e & 3) + 8 (e >> 2) + 4 hh][head r32]
      f32x16 Sx;
#pragma unroll
      for (int e = 0; e < 16; ++e) Sx[e] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) Sx = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], qf[ks], Sx, 0, 0, 0);
      if (k0 + KB < whi) {                                   // next batch's codes and scales under this batch's softmax and P.V
        load_batch(k0 + KB);
      }
      float rmax = -INFINITY;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int key = (e & 3) + 8 * (e >> 2) + 4 * hh;
        Sx[e] = key < nk ? Sx[e] : -INFINITY;
        rmax = fmaxf(rmax, Sx[e]);
      }
      {
        auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(rmax), __float_as_uint(rmax), false, false);
        rmax = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
      }
      const float m_new = fmaxf(m_run, rmax);                // finite: nk >= 1
      if (k0 > wlo) {                                        // wave-uniform: a second batch rescales what the first left
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c2);
        l_run *= alpha;
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
          for (int e = 0; e < 16; ++e) O[d][e] *= alpha;
      }
      m_run = m_new;
      const float mc = m_new * c2;
      float psum = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float pv = __builtin_amdgcn_exp2f(fmaf(Sx[e], c2, -mc));      // masked keys: exp2(-inf) = 0
        Sx[e] = pv;
        psum += pv;
      }
      l_run += psum;
      bf16x8 pf[2];
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) pf[s2][jj] = f2bf(Sx[8 * s2 + jj]);
      // ---- O^T += V^T . P^T
      __builtin_amdgcn_s_waitcnt(0xC07F);                    // this wave's V stores have landed (wave-private image)
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int s2 = i >> 2, d = i & 3;
        union { struct { s16x4 a, b; } s; bf16x8 v; } uu;
        uu.s.a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(sV + v_lb[0] + 2048 * (2 * s2) + 512 * d));
        uu.s.b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(sV + v_lb[1] + 2048 * (2 * s2 + 1) + 512 * d));
        O[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(uu.v, pf[s2], O[d], 0, 0, 0);
      }
      __builtin_amdgcn_wave_barrier();                       // the reads are issued before the next batch's stores (same wave, in order)
    }
  }
  // ---- the wave's result to LDS: lanes r32 < G hold head r32; the two halves hold disjoint d rows and partial l
  {
    auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(l_run), __float_as_uint(l_run), false, false);
    const float l_tot = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
    if (r32 < G) {
      if (hh == 0) { wm[w][r32] = m_run * a.scale; wl[w][r32] = l_tot; }      // natural-log units, as the combine expects
#pragma unroll
      for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *reinterpret_cast<f32x4*>(&wo[w][r32][32 * d + 8 * g + 4 * hh]) = f32x4{O[d][4 * g], O[d][4 * g + 1], O[d][4 * g + 2], O[d][4 * g + 3]};
    }
  }
  }
  __syncthreads();
  // ---- merge the four waves: one partial per (head, block)
  for (int idx = tid; idx < G * 128; idx += 256) {
    const int h = idx >> 7, d = idx & 127;
    float M = fmaxf(fmaxf(wm[0][h], wm[1][h]), fmaxf(wm[2][h], wm[3][h]));
    float L = 0.f, Ov = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float f = wm[k][h] == -INFINITY ? 0.f : __expf(wm[k][h] - M);
      L = fmaf(wl[k][h], f, L);
      Ov = fmaf(wo[k][h][d], f, Ov);
    }
    float* o = a.ws + (((size_t)z * Hq + kvh * G + h) * NBH + bx) * 130;
    if (d == 0) { o[0] = M; o[1] = L; }
    o[2 + d] = Ov;
  }
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
  Attn8Args a{(const __bf16*)qkv, (const float*)q_norm_w, (const float*)k_norm_w, (const float*)cos, (const float*)sin, eps, und_rounding,
              (uint8_t*)k_cache, (uint8_t*)v_cache, (float*)k_scale, (float*)v_scale, (float*)workspace, (const int*)Lk_dev, Hq, Hkv, scale,
              (long)scene_rows, max_len, (max_len + nbh - 1) / nbh, ((max_len + nbh - 1) / nbh + 3) / 4};
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(decode_attn_pg_kv8_kernel, dim3(nbh, Hkv, batch), dim3(256), 0, s, a);
  G2V_CHECK_LAUNCH();
  hipLaunchKernelGGL(decode_combine_pg_kernel, dim3(Hq, batch), dim3(1024), 0, s, (const float*)workspace, (__bf16*)out, nbh);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}
