// Split-KV decode attention of the persistent-grid step: ONE core for the bf16 cache (decode_layer.hip), the e4m3 cache
// (decode_kv8.hip) and the shared-prefix blocks (decode_shared.hip), and the kernel that merges its partials.
//   norm_rope_row      q / k RMS-norm + rotation of one 16-lane row
//   attn_batch_step    one 32-key batch on a wave's running (m, l, O): V -> LDS image, S^T = K.Q^T, prefetch, softmax, O^T += V^T.P^T
//   wave_result_to_lds, merge_waves   the wave's (m, l, o) to LDS, the four waves' to one 130-word partial per column
//   KvBf16             the cache-format policy of a bf16 cache (KvE4m3: decode_kv8.hip): the batch in registers, its loads, its bf16
//                      operands, and the quantisation and store of the new token's rows
//   decode_attn_pg_body<Fmt>          the kernel body on a per-scene cache with the append of the new token's rows
#pragma once
#include "common.h"
#include "decode_util.h"

namespace {

constexpr int KB = 32, GMAX = 8;

// Blocks per (scene, kv head) of g2v_decode_attn_pg and g2v_decode_attn_pg_kv8 = partials per head (2..128: the combine reads
// <= 128).  256 blocks per scene for one or two scenes; from three scenes on fewer, longer shares (>= 512 blocks in all, >= 8
// per kv head) - at B = 8 a block with 96 keys spends its life in the prologue (3.0 TB/s), one with 384 keys streams three
// batches per wave behind it
inline int decode_attn_pg_nbh(int Hkv, int batch) {
  const int nbh1 = 256 / Hkv > 128 ? 128 : 256 / Hkv;
  const int nbhb = 512 / (Hkv * batch) < 8 ? 8 : 512 / (Hkv * batch);
  return nbhb < nbh1 ? nbhb : nbh1;
}

// kc / vc: bf16 rows, or e4m3 codes with ksc / vsc their per-(row, kv head) scales.  The scales come last: the bf16 kernels never
// read them, and every field they do read keeps the offset (and the scalar loads) it had before the two formats shared this struct.
struct AttnArgs {
  const __bf16* qkv; const float* qw; const float* kw; const float* cs; const float* sn; float eps; int und_rounding;
  void* kc; void* vc; float* ws; const int* Lk_dev; int Hq, Hkv; float scale; long scene_rows; int cap, S, SW;
  float* ksc; float* vsc;
};

// byte offset of 16-byte chunk `ch` of row `row` in the dual-use LDS image (attn.hip lds_off, guide T10 layout (a))
__device__ __forceinline__ int v_img_off(int row, int ch) {
  return 2048 * (row >> 3) + 512 * (ch >> 2) + 64 * (row & 7) + 16 * ((ch & 3) ^ ((row >> 2) & 3));
}

// LDS of one workgroup of the attention (4 waves): 58.4 KB
struct AttnLds {
  __attribute__((aligned(16))) __bf16 sq[4][GMAX + 1][128];   // per wave: normalised q heads + the new k
  __attribute__((aligned(16))) char sv[4][KB * 256];           // per wave: the V batch, dual-use image
  float wm[4][GMAX], wl[4][GMAX];
  __attribute__((aligned(16))) float wo[4][GMAX][128];
};

// RMS-norm + rotation of one row of 128 held by 16 lanes: lane j has elements 4 j .. 4 j + 3 (a0) and 64 + 4 j .. (a1), the
// weights and the RoPE row likewise.  The arithmetic is meant to be qknorm_mrope_cache_kernel's (norm_rope.hip); that the two
// agree bit for bit (the tests compare the appended K row with torch.equal) also rests on how the compiler contracts THAT
// kernel's rotation, which its source does not pin.
__device__ __forceinline__ void norm_rope_row(const u32x2 a0, const u32x2 a1, const f32x4 w0, const f32x4 w1, const f32x4 c0, const f32x4 c1,
                                              const f32x4 s0, const f32x4 s1, const float eps, const int und_rounding, u32x2& p0, u32x2& p1) {
  float x0[4] = {bits2f_lo(a0[0]), bits2f_hi(a0[0]), bits2f_lo(a0[1]), bits2f_hi(a0[1])};
  float x1[4] = {bits2f_lo(a1[0]), bits2f_hi(a1[0]), bits2f_lo(a1[1]), bits2f_hi(a1[1])};
  float ss = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) ss += x0[e] * x0[e] + x1[e] * x1[e];
  ss = row16_sum(ss);
  const float rstd = 1.0f / sqrtf(ss / 128.f + eps);
  float o0[4], o1[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float n0 = __fmul_rn(x0[e], rstd), n1 = __fmul_rn(x1[e], rstd);
    if (und_rounding) { n0 = bfround(n0); n1 = bfround(n1); }
    n0 = __fmul_rn(w0[e], n0); n1 = __fmul_rn(w1[e], n1);
    // The rotation, with its contractions written out: __fmul_rn / __fadd_rn do not keep the compiler from fusing, and which
    // sums it fused depended on how it had vectorised the code around them.  This is what the compiler made of the three
    // inline copies this function replaces (elements 0..2 fused onto the first product, element 3 with both products
    // rounded; read from their assembly); two builds are compared bit for bit (tools/decode_attn_ab.py), so it is pinned.
    if (e < 3) {
      o0[e] = fmaf(n0, c0[e], __fmul_rn(-n1, s0[e]));
      o1[e] = fmaf(n1, c1[e], __fmul_rn(n0, s1[e]));
    } else {
#pragma clang fp contract(off)
      o0[e] = n0 * c0[e] + -n1 * s0[e];
      o1[e] = n1 * c1[e] + n0 * s1[e];
    }
  }
  p0 = u32x2{pack_bf16x2(o0[0], o0[1]), pack_bf16x2(o0[2], o0[3])};
  p1 = u32x2{pack_bf16x2(o1[0], o1[1]), pack_bf16x2(o1[2], o1[3])};
}

// A wave's running online softmax: lane (r32, hh) holds column r32 (a query head), raw-score units, its half's keys
struct AttnAcc {
  float m = -INFINITY, l = 0.f;
  f32x16 O[4];                                               // O^T[d = 32 blk + row][column r32]
  __device__ __forceinline__ AttnAcc() {
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
      for (int e = 0; e < 16; ++e) O[d][e] = 0.f;
  }
};

// V^T fragment addresses (attn.hip): row 16 s + 8 jj + 4 hh + tq, chunk 4 d + t_ch -> v_lb[jj] + 2048 (2 s + jj) + 512 d
__device__ __forceinline__ void v_frag_base(const int lane, int (&v_lb)[2]) {
  const int hh = lane >> 5, tq = (lane & 15) >> 2, tp = lane & 3;
  const int t_ch = 2 * ((lane >> 4) & 1) + (tp >> 1);
  v_lb[0] = 64 * (4 * hh + tq) + 16 * (t_ch ^ hh) + 8 * (tp & 1);
  v_lb[1] = v_lb[0] ^ 32;
}

// One batch of nk <= 32 keys: kf = the lane's K fragments (A operand: key r32, elements 16 ks + 8 hh ..), vchunk(i) = its V
// staging chunk i (row 4 i + fg, elements 8 fr ..), qf = the B operand Q^T[d = 16 ks + 8 hh + j][column r32], sV the wave-private image.
// `prefetch` issues the next batch's loads: after the QK MFMAs (the batch's registers are free: the MFMAs have issued, the LDS stores
// have read the V chunks), under this batch's softmax and P.V.
template <class VChunk, class Prefetch>
__device__ __forceinline__ void attn_batch_step(AttnAcc& s, const bf16x8 (&kf)[8], VChunk&& vchunk, const bf16x8 (&qf)[8], const int nk,
                                                const bool first, const float c2, char* sV, const int (&v_lb)[2], const int lane,
                                                Prefetch&& prefetch) {
  const int hh = lane >> 5, fr = lane & 15, fg = lane >> 4;
  // ---- V batch -> LDS image (rows at or past nk as zeros: 0 x NaN must not reach the MFMA)
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int row = 4 * i + fg;
    const u32x4 val = row < nk ? vchunk(i) : u32x4{0u, 0u, 0u, 0u};
    *reinterpret_cast<u32x4*>(sV + v_img_off(row, fr)) = val;
  }
  // ---- S^T = K . Q^T: register e of lane (r32, hh) is S[key (e & 3) + 8 (e >> 2) + 4 hh][column r32]
  f32x16 Sx;
#pragma unroll
  for (int e = 0; e < 16; ++e) Sx[e] = 0.f;
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) Sx = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], qf[ks], Sx, 0, 0, 0);
  prefetch();
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
  const float m_new = fmaxf(s.m, rmax);                      // finite: nk >= 1
  if (!first) {                                              // wave-uniform: a second batch rescales what the first left
    const float alpha = __builtin_amdgcn_exp2f((s.m - m_new) * c2);
    s.l *= alpha;
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
      for (int e = 0; e < 16; ++e) s.O[d][e] *= alpha;
  }
  s.m = m_new;
  const float mc = m_new * c2;
  float psum = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const float pv = __builtin_amdgcn_exp2f(fmaf(Sx[e], c2, -mc));      // masked keys: exp2(-inf) = 0
    Sx[e] = pv;
    psum += pv;
  }
  s.l += psum;
  bf16x8 pf[2];
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) pf[s2][jj] = f2bf(Sx[8 * s2 + jj]);
  // ---- O^T += V^T . P^T
  __builtin_amdgcn_s_waitcnt(0xC07F);                        // this wave's V stores have landed (wave-private image)
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int s2 = i >> 2, d = i & 3;
    union { struct { s16x4 a, b; } s; bf16x8 v; } uu;
    uu.s.a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(sV + v_lb[0] + 2048 * (2 * s2) + 512 * d));
    uu.s.b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(sV + v_lb[1] + 2048 * (2 * s2 + 1) + 512 * d));
    s.O[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(uu.v, pf[s2], s.O[d], 0, 0, 0);
  }
  __builtin_amdgcn_wave_barrier();                           // the reads are issued before the next batch's stores (same wave, in order)
}

// The wave's result to its rows wm / wl / wo of LDS: lanes r32 < ncol hold column r32; the two halves hold disjoint d rows
// and partial l.  m in natural-log units, as the combine expects.
__device__ __forceinline__ void wave_result_to_lds(const AttnAcc& s, const float scale, const int ncol, const int lane, float* wm, float* wl,
                                                   float (*wo)[128]) {
  const int r32 = lane & 31, hh = lane >> 5;
  auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(s.l), __float_as_uint(s.l), false, false);
  const float l_tot = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
  if (r32 < ncol) {
    if (hh == 0) { wm[r32] = s.m * scale; wl[r32] = l_tot; }
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<f32x4*>(&wo[r32][32 * d + 8 * g + 4 * hh]) = f32x4{s.O[d][4 * g], s.O[d][4 * g + 1], s.O[d][4 * g + 2], s.O[d][4 * g + 3]};
  }
}

// Merge the four waves: one partial {m, l, o[128]} per column, at partial(column) in the workspace
template <int NC, class Partial>
__device__ __forceinline__ void merge_waves(const int tid, const int ncol, const float (&wm)[4][NC], const float (&wl)[4][NC],
                                            const float (&wo)[4][NC][128], Partial&& partial) {
  for (int idx = tid; idx < ncol * 128; idx += 256) {
    const int c = idx >> 7, d = idx & 127;
    float M = fmaxf(fmaxf(wm[0][c], wm[1][c]), fmaxf(wm[2][c], wm[3][c]));
    float L = 0.f, Ov = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float f = wm[k][c] == -INFINITY ? 0.f : __expf(wm[k][c] - M);
      L = fmaf(wl[k][c], f, L);
      Ov = fmaf(wo[k][c][d], f, Ov);
    }
    float* o = partial(c);
    if (d == 0) { o[0] = M; o[1] = L; }
    o[2 + d] = Ov;
  }
}

// Cache-format policy, bf16 rows: a lane's share of a 32-key batch IS its MFMA operands.  kc / vc: the scene's (or the
// prefix's) rows [.., Hkv, 128].  Rows are clamped to last_row (always mapped); what lies past the length is masked by the step.
struct KvBf16 {
  __bf16 *krows, *vrows;                                     // row 0 of this kv head (a read-only prefix too: store_k / store_v are
                                                             // for the caller that owns the rows, decode_attn_pg_body)
  int row_stride, last_row, lane;
  bf16x8 kf[8];                                              // A operand: lane (r32, hh) takes K[key r32][16 ks + 8 hh ..]
  u32x4 vv[8], vnew;                                         // staging: lane (fg, fr) takes V[row 4 i + fg][8 fr ..]
  __device__ __forceinline__ KvBf16(const void* kc, const void* vc, const float*, const float*, const size_t row0, const int kvh, const int Hkv,
                                    const int last_row_, const int lane_)
      : krows((__bf16*)kc + (row0 * Hkv + kvh) * 128), vrows((__bf16*)vc + (row0 * Hkv + kvh) * 128), row_stride(Hkv * 128),
        last_row(last_row_), lane(lane_) {}
  __device__ __forceinline__ void load_batch(const int k0) {
    const __bf16* kp = krows + 8 * (lane >> 5) + (size_t)min(k0 + (lane & 31), last_row) * row_stride;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) kf[ks] = *reinterpret_cast<const bf16x8*>(kp + 16 * ks);
#pragma unroll
    for (int i = 0; i < 8; ++i)
      vv[i] = *reinterpret_cast<const u32x4*>(vrows + 8 * (lane & 15) + (size_t)min(k0 + 4 * i + (lane >> 4), last_row) * row_stride);
  }
  // The batch as bf16 operands: f(K fragments) and V chunk i.  Here both are the registers themselves (a copy of the batch
  // costs this kernel its last free registers); KvE4m3 converts each where it is used.  new_batch (wave-uniform): the batch
  // ends with the new token's row, at batch row `local`; the loads read whatever the cache row held BEFORE this step, so
  // the new V row and the new K row (knew: its row of the strip, this lane's k half) are put in first.
  template <class F>
  __device__ __forceinline__ void with_k_bf16(const bool new_batch, const int local, const __bf16* knew, F&& f) {
    if (new_batch) {
      if ((lane & 31) == local) {
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) kf[ks] = *reinterpret_cast<const bf16x8*>(knew + 16 * ks);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (4 * i + (lane >> 4) == local) vv[i] = vnew;
    }
    f(kf);
  }
  __device__ __forceinline__ u32x4 v_bf16(const int i) const { return vv[i]; }
  // the new token's rows: V as loaded (lane fr: elements 8 fr ..), K after norm and rotation (lane j: p0 = elements 4 j ..,
  // p1 = 64 + 4 j ..).  quant_k leaves in p0 / p1 what the strip (this step's scores) gets.
  __device__ __forceinline__ void set_new_v(const u32x4 v) { vnew = v; }
  __device__ __forceinline__ void quant_k(u32x2&, u32x2&, bool) {}
  __device__ __forceinline__ void store_k(const int row, const u32x2 p0, const u32x2 p1) const {
    __bf16* krow = krows + (size_t)row * row_stride + 4 * (lane & 15);
    *reinterpret_cast<u32x2*>(krow) = p0;
    *reinterpret_cast<u32x2*>(krow + 64) = p1;
  }
  __device__ __forceinline__ void store_v(const int row) const {                 // lanes fg == 0
    *reinterpret_cast<u32x4*>(vrows + (size_t)row * row_stride + 8 * (lane & 15)) = vnew;
  }
};

// The body of the kernel for block (bx of NBH, kv head kvh, scene z) of 4 waves, on a cache of format Fmt.
template <class Fmt>
__device__ __forceinline__ void decode_attn_pg_body(const AttnArgs& a, AttnLds& lds, const int bx, const int kvh, const int z, const int NBH,
                                                    const int tid G2V_STAMP_ARG) {
  G2V_STAMP_RT(10);
  G2V_STAMP(0);
  const int Hq = a.Hq, Hkv = a.Hkv, G = Hq / Hkv;
  const __bf16* q = a.qkv + (size_t)z * (Hq + 2 * Hkv) * 128;
  const int lane = tid & 63, w = tid >> 6;
  const int r32 = lane & 31, hh = lane >> 5;                 // MFMA 32x32: row / column index, k half
  const int fr = lane & 15, fg = lane >> 4;
  const int S = a.S, SW = a.SW;                             // keys per block / per wave, by capacity (host: ceil(cap / NBH), ceil(S / 4))
  const int wlo = bx * S + w * SW;
  const int wcap = min(min(wlo + SW, (bx + 1) * S), a.cap);   // end of this wave's range if the cache were full
  Fmt kv(a.kc, a.vc, a.ksc, a.vsc, (size_t)z * a.scene_rows, kvh, Hkv, a.cap - 1, lane);

  // ---- every load first, the step's own rows before the cache (vmcnt retires in issue order: the norms below run while
  // K / V are in flight).  Rows are clamped to the cache block (always mapped); what lies past the length is masked below.
  const int j = lane & 15;
  u32x2 x0r[3], x1r[3];
#pragma unroll
  for (int ps = 0; ps < 3; ++ps) {
    const int item = min(4 * ps + (lane >> 4), G);          // G = the new token's k row
    const __bf16* src = q + (item < G ? kvh * G + item : Hq + kvh) * 128 + 4 * j;
    x0r[ps] = *reinterpret_cast<const u32x2*>(src);
    x1r[ps] = *reinterpret_cast<const u32x2*>(src + 64);
  }
  const u32x4 vnew = *reinterpret_cast<const u32x4*>(q + (Hq + Hkv + kvh) * 128 + 8 * fr);
  const float* cs = a.cs + (size_t)z * 128;
  const float* sn = a.sn + (size_t)z * 128;
  const f32x4 qw0 = *reinterpret_cast<const f32x4*>(a.qw + 4 * j), qw1 = *reinterpret_cast<const f32x4*>(a.qw + 64 + 4 * j);
  const f32x4 kw0 = *reinterpret_cast<const f32x4*>(a.kw + 4 * j), kw1 = *reinterpret_cast<const f32x4*>(a.kw + 64 + 4 * j);
  const f32x4 c0 = *reinterpret_cast<const f32x4*>(cs + 4 * j), c1 = *reinterpret_cast<const f32x4*>(cs + 64 + 4 * j);
  const f32x4 s0 = *reinterpret_cast<const f32x4*>(sn + 4 * j), s1 = *reinterpret_cast<const f32x4*>(sn + 64 + 4 * j);
  kv.load_batch(wlo);
  const int Lk = a.Lk_dev[z];
  G2V_STAMP(1);

  const int whi = min(wcap, Lk);                            // the wave's real range is [wlo, whi)
  const bool has_new = wlo < whi && whi == Lk;              // it ends with the new token's row (wave-uniform)

  // ---- q / k norm + rotation of the step's rows: every wave, unconditionally (the loads above must not end up behind the
  // wait for the length word; only the STORES of the new rows depend on it)
  kv.set_new_v(vnew);
#pragma unroll
  for (int ps = 0; ps < 3; ++ps) {
    if (4 * ps < G + 1) {                                   // uniform over the launch
      const int c = 4 * ps + (lane >> 4);
      const int item = min(c, G);                           // what this group loaded above
      const bool isq = item < G;
      u32x2 p0, p1;
      norm_rope_row(x0r[ps], x1r[ps], isq ? qw0 : kw0, isq ? qw1 : kw1, c0, c1, s0, s1, a.eps, a.und_rounding, p0, p1);
      kv.quant_k(p0, p1, isq);
      if (c <= G) {                                          // strip rows 0..G (row G is only read by the wave that owns the new row)
        *reinterpret_cast<u32x2*>(&lds.sq[w][item][4 * j]) = p0;
        *reinterpret_cast<u32x2*>(&lds.sq[w][item][64 + 4 * j]) = p1;
      }
      if (c == G && has_new) kv.store_k(Lk - 1, p0, p1);    // the new token's K row -> cache row Lk - 1 of this scene
    }
  }
  G2V_STAMP(2);
  AttnAcc acc;
  const float c2 = a.scale * 1.4426950408889634f;            // p = 2^((s - m) c2)

  if (wlo < whi) {
    __builtin_amdgcn_s_waitcnt(0xC07F);                      // the strip is written and read by this wave only
    __builtin_amdgcn_wave_barrier();
    bf16x8 qf[8];                                            // columns past G duplicate head G - 1
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(&lds.sq[w][min(r32, G - 1)][16 * ks + 8 * hh]);
    if (has_new && fg == 0) kv.store_v(Lk - 1);
    char* sV = lds.sv[w];
    int v_lb[2];
    v_frag_base(lane, v_lb);

#pragma nounroll                                             // nor peel the first batch off: one copy of the step per kernel
    for (int k0 = wlo; k0 < whi; k0 += KB) {
      const int nk = min(KB, whi - k0);
      kv.with_k_bf16(has_new && k0 + nk == whi, Lk - 1 - k0, &lds.sq[w][G][8 * hh], [&](bf16x8 (&kf)[8]) {
        attn_batch_step(acc, kf, [&](int i) { return kv.v_bf16(i); }, qf, nk, k0 == wlo, c2, sV, v_lb, lane,
                        [&] { if (k0 + KB < whi) kv.load_batch(k0 + KB); });
      });
      if (k0 == wlo) G2V_STAMP(3);
    }
  }
  G2V_STAMP(4);
  wave_result_to_lds(acc, a.scale, G, lane, lds.wm[w], lds.wl[w], lds.wo[w]);
  G2V_STAMP(5);
  __syncthreads();
  G2V_STAMP(6);
  float* o = a.ws + (((size_t)z * Hq + kvh * G) * NBH + bx) * 130;             // ws[((z Hq + head) NBH + bx) 130 + {m, l, o[128]}]
  merge_waves(tid, G, lds.wm, lds.wl, lds.wo, [&](int h) { return o + h * NBH * 130; });
  G2V_STAMP(7);
  G2V_STAMP_RT(11);
}

// out[z][h][d] = sum_b O_b e^(m_b - M) / sum_b l_b e^(m_b - M) over the NBH <= 128 block partials of a head.
// grid (Hq, scenes); 1024 threads = 128 d x 8 groups of 16 consecutive partials.  All loads of a thread - the (m, l) pair
// of partial `tid` and its 16 O words - are issued before the first use (one memory round trip; a loop of dependent loads
// over the partials made this kernel 11.7 us, as long as the attention itself); reductions by DPP / readlane, the 16 weights
// of a group by four 16-byte LDS reads.
__global__ __launch_bounds__(1024) void decode_combine_pg_kernel(const float* ws, __bf16* out, int NBH) {
  __shared__ float sm[2];
  __shared__ __attribute__((aligned(16))) float sf[128];
  __shared__ float sL[2], sO[8][128];
  const int h = blockIdx.x, z = blockIdx.y, tid = threadIdx.x, d = tid & 127, g = tid >> 7;
  const float* p = ws + ((size_t)z * gridDim.x + h) * NBH * 130;
  float ov[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) ov[k] = p[min(16 * g + k, NBH - 1) * 130 + 2 + d];
  float m = -INFINITY, l = 0.f;
  if (tid < NBH) { m = p[tid * 130]; l = p[tid * 130 + 1]; }
  if (tid < 128) {                                          // waves 0 and 1 hold the (m, l) pairs
    float mx = row16_max(m);
    mx = fmaxf(fmaxf(readlane_f(mx, 0), readlane_f(mx, 16)), fmaxf(readlane_f(mx, 32), readlane_f(mx, 48)));
    if ((tid & 63) == 0) sm[tid >> 6] = mx;
  }
  __syncthreads();
  const float M = fmaxf(sm[0], sm[1]);
  if (tid < 128) {
    const float f = m == -INFINITY ? 0.f : __expf(m - M);
    sf[tid] = f;
    const float lw = wave_sum_dpp(l * f);
    if ((tid & 63) == 0) sL[tid >> 6] = lw;
  }
  __syncthreads();
  float O = 0.f;
#pragma unroll
  for (int k4 = 0; k4 < 4; ++k4) {
    const f32x4 f4 = *reinterpret_cast<const f32x4*>(&sf[16 * g + 4 * k4]);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (16 * g + 4 * k4 + e < NBH) O = fmaf(ov[4 * k4 + e], f4[e], O);
  }
  sO[g][d] = O;
  __syncthreads();
  if (g == 0) {
    const float Lt = sL[0] + sL[1];
    float Ot = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) Ot += sO[k][d];
    out[((size_t)z * gridDim.x + h) * 128 + d] = f2bf(Ot / Lt);
  }
}

}  // namespace
