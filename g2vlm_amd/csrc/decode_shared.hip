// Decode attention over a prefix shared by B query slots (several questions about one scene).
//
// The step of slot z attends to the shared prefix rows [0, prefix_len) followed by its own suffix rows [0, suffix_len[z]).
// g2v_decode_attn_pg over B copies of the prefix reads B x the prefix bytes per step; here they are read once per column
// group.  decode_attn_pg_body (decode_attn_pg.h) puts the G <= 8 query heads of a kv head into the 32 columns of a
// mfma_f32_32x32x16_bf16 and duplicates head G - 1 into the rest; the prefix blocks below fill those columns with the
// (slot, head) pairs of floor(32 / G) slots instead, so one K / V batch in registers serves all of them.  More slots than
// that take further column groups: separate workgroups over the same prefix rows, whose repeated reads come from the
// Infinity Cache (a second group held in registers would cost 64 more accumulators and its Q fragments per wave).
//
// One launch holds both kinds of workgroup (prefix first, as they are the long ones):
//   * prefix blocks (pb, kvh, group): 4 waves, each a contiguous range of SWP (a multiple of 32) prefix rows; the partial of
//     every (slot, head) column goes to the workspace as block nbs + pb of that head;
//   * suffix blocks (bx, kvh, z): decode_attn_pg_body as it is, over slot z's suffix block with the capacity split of
//     suffix_max_len; they normalise / rotate the step's q / k, append the new K / V row and write blocks [0, nbs).
// decode_combine_pg_kernel then merges the nbs + nbp <= 128 partials of each (slot, head): ws [B][Hq][nbs + nbp][130].
#include "common.h"
#include "decode_util.h"
#include "decode_attn_pg.h"
#include "g2vlm_hip.h"

#ifdef G2V_STAMPS
#define G2V_SHARED_NO_STAMPS , (unsigned long long*)nullptr
#else
#define G2V_SHARED_NO_STAMPS
#endif

namespace {

constexpr int NCOL = 32;                                     // MFMA columns of a prefix block: (slot, head) pairs

struct PrefixArgs {
  const __bf16* qkv; const float* qw; const float* kw; const float* cs; const float* sn; float eps; int und_rounding;
  const __bf16* kp; const __bf16* vp; float* ws; int B, Hq, Hkv; float scale;
  int prefix_len, SWP, NBP, SPG, NGRP, NBS, NBH;             // rows per wave, blocks per kv head, slots per group, groups, ...
};

// LDS of a prefix block (4 waves): 73 KB.  The V images are dead once the key loop is over: the per-wave results overlay them.
struct PrefixLds {
  __attribute__((aligned(16))) __bf16 sq[NCOL][128];           // normalised, rotated q of every column
  float wm[4][NCOL], wl[4][NCOL];
  union {
    __attribute__((aligned(16))) char sv[4][KB * 256];         // per wave: the V batch, dual-use image (attn.hip)
    __attribute__((aligned(16))) float wo[4][NCOL][128];
  } u;
};

__device__ __forceinline__ void prefix_block(const PrefixArgs& a, PrefixLds& lds, const int pb, const int kvh, const int grp, const int tid) {
  const int Hq = a.Hq, Hkv = a.Hkv, G = Hq / Hkv;
  const int z0 = grp * a.SPG, ns = min(a.SPG, a.B - z0), ncol = ns * G;
  const int lane = tid & 63, w = tid >> 6;
  const int r32 = lane & 31, hh = lane >> 5;
  const int fr = lane & 15, fg = lane >> 4;
  const int row_stride = Hkv * 128;
  const int wlo = pb * 4 * a.SWP + w * a.SWP;
  const int whi = min(wlo + a.SWP, a.prefix_len);
  const int last_row = a.prefix_len - 1;                     // rows at or past prefix_len may hold anything: never loaded
  const __bf16* kbase = a.kp + kvh * 128 + 8 * hh;
  const __bf16* vbase = a.vp + kvh * 128 + 8 * fr;

  // ---- every load first: the q rows of this wave's 8 columns (2 passes of 4), then the first K / V batch
  const int j = lane & 15;
  u32x2 x0r[2], x1r[2];
  f32x4 c0[2], c1[2], s0[2], s1[2];
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {
    const int c = min(8 * w + 4 * ps + (lane >> 4), ncol - 1);           // columns past the group's duplicate its last one
    const int z = z0 + c / G, h = kvh * G + c % G;
    const __bf16* q = a.qkv + (size_t)z * (Hq + 2 * Hkv) * 128;
    const int src = 2 * (h * 128 + 4 * j);
    x0r[ps] = *reinterpret_cast<const u32x2*>(reinterpret_cast<const char*>(q) + src);
    x1r[ps] = *reinterpret_cast<const u32x2*>(reinterpret_cast<const char*>(q) + src + 128);
    const float* cs = a.cs + (size_t)z * 128;
    const float* sn = a.sn + (size_t)z * 128;
    c0[ps] = *reinterpret_cast<const f32x4*>(cs + 4 * j); c1[ps] = *reinterpret_cast<const f32x4*>(cs + 64 + 4 * j);
    s0[ps] = *reinterpret_cast<const f32x4*>(sn + 4 * j); s1[ps] = *reinterpret_cast<const f32x4*>(sn + 64 + 4 * j);
  }
  const f32x4 qw0 = *reinterpret_cast<const f32x4*>(a.qw + 4 * j), qw1 = *reinterpret_cast<const f32x4*>(a.qw + 64 + 4 * j);
  bf16x8 kf[8];
  u32x4 vv[8];
  auto load_batch = [&](int k0) {
    const __bf16* kp = kbase + (size_t)min(k0 + r32, last_row) * row_stride;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) kf[ks] = *reinterpret_cast<const bf16x8*>(kp + 16 * ks);
#pragma unroll
    for (int i = 0; i < 8; ++i) vv[i] = *reinterpret_cast<const u32x4*>(vbase + (size_t)min(k0 + 4 * i + fg, last_row) * row_stride);
  };
  if (wlo < whi) load_batch(wlo);

  // ---- q norm + rotation: decode_attn_pg_body's arithmetic (qknorm_mrope_cache_kernel's), column by column
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {
    const int c = 8 * w + 4 * ps + (lane >> 4);
    const u32x2 a0 = x0r[ps], a1 = x1r[ps];
    float x0[4] = {bits2f_lo(a0[0]), bits2f_hi(a0[0]), bits2f_lo(a0[1]), bits2f_hi(a0[1])};
    float x1[4] = {bits2f_lo(a1[0]), bits2f_hi(a1[0]), bits2f_lo(a1[1]), bits2f_hi(a1[1])};
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) ss += x0[e] * x0[e] + x1[e] * x1[e];
    ss = row16_sum(ss);
    const float rstd = 1.0f / sqrtf(ss / 128.f + a.eps);
    float o0[4], o1[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float n0 = __fmul_rn(x0[e], rstd), n1 = __fmul_rn(x1[e], rstd);
      if (a.und_rounding) { n0 = bfround(n0); n1 = bfround(n1); }
      n0 = __fmul_rn(qw0[e], n0); n1 = __fmul_rn(qw1[e], n1);
      o0[e] = __fadd_rn(__fmul_rn(n0, c0[ps][e]), __fmul_rn(-n1, s0[ps][e]));
      o1[e] = __fadd_rn(__fmul_rn(n1, c1[ps][e]), __fmul_rn(n0, s1[ps][e]));
    }
    *reinterpret_cast<u32x2*>(&lds.sq[c][4 * j]) = u32x2{pack_bf16x2(o0[0], o0[1]), pack_bf16x2(o0[2], o0[3])};
    *reinterpret_cast<u32x2*>(&lds.sq[c][64 + 4 * j]) = u32x2{pack_bf16x2(o1[0], o1[1]), pack_bf16x2(o1[2], o1[3])};
  }
  __syncthreads();                                           // every wave reads all 32 columns

  float m_run = -INFINITY, l_run = 0.f;                      // this lane's column r32, raw-score units / its half's keys
  f32x16 O[4];                                               // O^T[d = 32 blk + row][column r32]
#pragma unroll
  for (int d = 0; d < 4; ++d)
#pragma unroll
    for (int e = 0; e < 16; ++e) O[d][e] = 0.f;
  const float c2 = a.scale * 1.4426950408889634f;            // p = 2^((s - m) c2)

  if (wlo < whi) {
    bf16x8 qf[8];                                            // B operand: Q^T[d = 16 ks + 8 hh + j][column r32]
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(&lds.sq[r32][16 * ks + 8 * hh]);
    char* sV = lds.u.sv[w];
    const int tq = (lane & 15) >> 2, tp = lane & 3;
    const int t_ch = 2 * ((lane >> 4) & 1) + (tp >> 1);
    int v_lb[2];
    v_lb[0] = 64 * (4 * hh + tq) + 16 * (t_ch ^ hh) + 8 * (tp & 1);
    v_lb[1] = v_lb[0] ^ 32;

    for (int k0 = wlo; k0 < whi; k0 += KB) {
      const int nk = min(KB, whi - k0);
      // ---- V batch -> LDS image (rows at or past nk as zeros)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int row = 4 * i + fg;
        const u32x4 val = row < nk ? vv[i] : u32x4{0u, 0u, 0u, 0u};
        *reinterpret_cast<u32x4*>(sV + v_img_off(row, fr)) = val;
      }
      // ---- S^T = K . Q^T: register e of lane (r32, hh) is S[key (e & 3) + 8 (e >> 2) + 4 hh][column r32]
      f32x16 Sx;
#pragma unroll
      for (int e = 0; e < 16; ++e) Sx[e] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) Sx = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], qf[ks], Sx, 0, 0, 0);
      if (k0 + KB < whi) load_batch(k0 + KB);                // next batch's K / V under this batch's softmax and P.V
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
      const float m_new = fmaxf(m_run, rmax);
      if (k0 > wlo) {
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
        const float pv = __builtin_amdgcn_exp2f(fmaf(Sx[e], c2, -mc));
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
      __builtin_amdgcn_s_waitcnt(0xC07F);
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int s2 = i >> 2, d = i & 3;
        union { struct { s16x4 a, b; } s; bf16x8 v; } uu;
        uu.s.a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(sV + v_lb[0] + 2048 * (2 * s2) + 512 * d));
        uu.s.b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(sV + v_lb[1] + 2048 * (2 * s2 + 1) + 512 * d));
        O[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(uu.v, pf[s2], O[d], 0, 0, 0);
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
  __syncthreads();                                           // the V images are free: the results overlay them
  {
    auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(l_run), __float_as_uint(l_run), false, false);
    const float l_tot = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
    if (r32 < ncol) {
      if (hh == 0) { lds.wm[w][r32] = m_run * a.scale; lds.wl[w][r32] = l_tot; }
#pragma unroll
      for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *reinterpret_cast<f32x4*>(&lds.u.wo[w][r32][32 * d + 8 * g + 4 * hh]) = f32x4{O[d][4 * g], O[d][4 * g + 1], O[d][4 * g + 2], O[d][4 * g + 3]};
    }
  }
  __syncthreads();
  // ---- merge the four waves (decode_attn_pg_body's merge): one partial per (slot, head) column, block nbs + pb of its head
  for (int idx = tid; idx < ncol * 128; idx += 256) {
    const int c = idx >> 7, d = idx & 127;
    float M = fmaxf(fmaxf(lds.wm[0][c], lds.wm[1][c]), fmaxf(lds.wm[2][c], lds.wm[3][c]));
    float L = 0.f, Ov = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float f = lds.wm[k][c] == -INFINITY ? 0.f : __expf(lds.wm[k][c] - M);
      L = fmaf(lds.wl[k][c], f, L);
      Ov = fmaf(lds.u.wo[k][c][d], f, Ov);
    }
    const int z = z0 + c / G, h = kvh * G + c % G;
    float* o = a.ws + (((size_t)z * Hq + h) * a.NBH + a.NBS + pb) * 130;
    if (d == 0) { o[0] = M; o[1] = L; }
    o[2 + d] = Ov;
  }
}

__global__ __launch_bounds__(256, 2) void decode_attn_shared_kernel(AttnArgs sa, PrefixArgs pa G2V_STAMP_ARG) {
  __shared__ union { AttnLds s; PrefixLds p; } lds;
  int id = blockIdx.x;
  const int np = pa.NBP * pa.Hkv * pa.NGRP;
  if (id < np) {
    prefix_block(pa, lds.p, id % pa.NBP, (id / pa.NBP) % pa.Hkv, id / (pa.NBP * pa.Hkv), threadIdx.x);
    return;
  }
  id -= np;
  decode_attn_pg_body<false, false, 4>(sa, lds.s, id % pa.NBS, (id / pa.NBS) % pa.Hkv, id / (pa.NBS * pa.Hkv), pa.NBH,
                                       threadIdx.x G2V_STAMP_PASS_DEV);
}

struct SharedPlan { int G, spg, ngrp, nbs, nbp, swp; };

bool shared_plan(int Hq, int Hkv, int batch, int prefix_len, int suffix_max_len, SharedPlan& p) {
  if (Hq <= 0 || Hkv <= 0 || Hkv > 128 || Hq % Hkv || Hq / Hkv > GMAX || batch < 1 || batch > 64 || prefix_len < 1 ||
      suffix_max_len < 1)
    return false;
  p.G = Hq / Hkv;
  p.spg = NCOL / p.G < batch ? NCOL / p.G : batch;
  p.ngrp = (batch + p.spg - 1) / p.spg;
  // suffix: a block per 256 capacity rows (a question and its answer: one or two); prefix: ~512 workgroups over all groups
  // (2 per CU), each wave a whole number of 32-row batches, and nbs + nbp <= 128 partials per head for the combine
  p.nbs = (suffix_max_len + 255) / 256;
  if (p.nbs > 16) p.nbs = 16;
  int target = 512 / (Hkv * p.ngrp);
  if (target < 8) target = 8;
  if (target > 128 - p.nbs) target = 128 - p.nbs;
  const long per_block = ((long)prefix_len + target - 1) / target;
  p.swp = (int)(32 * ((per_block + 127) / 128));
  p.nbp = (int)(((long)prefix_len + 4L * p.swp - 1) / (4L * p.swp));
  return true;
}

}  // namespace

extern "C" int64_t g2v_decode_attn_shared_workspace(int Hq, int Hkv, int batch, int prefix_len, int suffix_max_len) {
  SharedPlan p;
  if (!shared_plan(Hq, Hkv, batch, prefix_len, suffix_max_len, p)) return 0;
  return (int64_t)batch * Hq * 128 * 130 * 4;                // the combine's 128 partials per head, whatever the lengths
}

extern "C" int g2v_decode_attn_shared(const void* qkv, const void* q_norm_w, const void* k_norm_w, float eps, int und_rounding,
                                      const void* cos, const void* sin, const void* k_prefix, const void* v_prefix, int prefix_len,
                                      void* k_suffix, void* v_suffix, const void* suffix_len_dev, int batch, int64_t suffix_rows,
                                      int suffix_max_len, int Hq, int Hkv, float scale, void* out, void* workspace, void* stream) {
  if (!qkv || !q_norm_w || !k_norm_w || !cos || !sin || !k_prefix || !v_prefix || !k_suffix || !v_suffix || !suffix_len_dev ||
      !out || !workspace)
    return G2V_ERR_ARG;
  SharedPlan p;
  if (!shared_plan(Hq, Hkv, batch, prefix_len, suffix_max_len, p) || suffix_rows < suffix_max_len) return G2V_ERR_ARG;
  const int nbh = p.nbs + p.nbp;
  const int S = (suffix_max_len + p.nbs - 1) / p.nbs;
  AttnArgs sa{(const __bf16*)qkv, (const float*)q_norm_w, (const float*)k_norm_w, (const float*)cos, (const float*)sin, eps, und_rounding,
              (__bf16*)k_suffix, (__bf16*)v_suffix, (float*)workspace, (const int*)suffix_len_dev, Hq, Hkv, scale, (long)suffix_rows,
              suffix_max_len, S, (S + 3) / 4};
  PrefixArgs pa{(const __bf16*)qkv, (const float*)q_norm_w, (const float*)k_norm_w, (const float*)cos, (const float*)sin, eps, und_rounding,
                (const __bf16*)k_prefix, (const __bf16*)v_prefix, (float*)workspace, batch, Hq, Hkv, scale,
                prefix_len, p.swp, p.nbp, p.spg, p.ngrp, p.nbs, nbh};
  const int blocks = p.nbp * Hkv * p.ngrp + p.nbs * Hkv * batch;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(decode_attn_shared_kernel, dim3(blocks), dim3(256), 0, s, sa, pa G2V_SHARED_NO_STAMPS);
  G2V_CHECK_LAUNCH();
  hipLaunchKernelGGL(decode_combine_pg_kernel, dim3(Hq, batch), dim3(1024), 0, s, (const float*)workspace, (__bf16*)out, nbh);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}
