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
//   * prefix blocks (pb, kvh, group): 4 waves, each a contiguous range of SWP (a multiple of 32) prefix rows, built from the
//     same pieces as that body (norm_rope_row, attn_batch_step, wave_result_to_lds, merge_waves); the partial of every
//     (slot, head) column goes to the workspace as block nbs + pb of that head;
//   * suffix blocks (bx, kvh, z): decode_attn_pg_body<KvBf16> as it is, over slot z's suffix block with the capacity split of
//     suffix_max_len; they normalise / rotate the step's q / k, append the new K / V row and write blocks [0, nbs).
// decode_combine_pg_kernel then merges the nbs + nbp <= 128 partials of each (slot, head): ws [B][Hq][nbs + nbp][130].
#include "common.h"
#include "decode_util.h"
#include "decode_attn_pg.h"
#include "g2vlm_hip.h"

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

// A prefix block: the key loop, the wave result and the merge are decode_attn_pg.h's on 32 columns; its own are the q strip of
// (slot, head) columns shared by the four waves, the results overlaying the V images, and no append.
__device__ __forceinline__ void prefix_block(const PrefixArgs& a, PrefixLds& lds, const int pb, const int kvh, const int grp, const int tid) {
  const int Hq = a.Hq, Hkv = a.Hkv, G = Hq / Hkv;
  const int z0 = grp * a.SPG, ns = min(a.SPG, a.B - z0), ncol = ns * G;
  const int lane = tid & 63, w = tid >> 6;
  const int r32 = lane & 31, hh = lane >> 5;
  const int wlo = pb * 4 * a.SWP + w * a.SWP;
  const int whi = min(wlo + a.SWP, a.prefix_len);
  KvBf16 kv(a.kp, a.vp, nullptr, nullptr, 0, kvh, Hkv, a.prefix_len - 1, lane);   // rows at or past prefix_len may hold anything: never loaded

  // ---- every load first: the q rows of this wave's 8 columns (2 passes of 4), then the first K / V batch
  const int j = lane & 15;
  u32x2 x0r[2], x1r[2];
  f32x4 c0[2], c1[2], s0[2], s1[2];
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {
    const int c = min(8 * w + 4 * ps + (lane >> 4), ncol - 1);           // columns past the group's duplicate its last one
    const int z = z0 + c / G, h = kvh * G + c % G;
    const __bf16* src = a.qkv + (size_t)z * (Hq + 2 * Hkv) * 128 + h * 128 + 4 * j;
    x0r[ps] = *reinterpret_cast<const u32x2*>(src);
    x1r[ps] = *reinterpret_cast<const u32x2*>(src + 64);
    const float* cs = a.cs + (size_t)z * 128;
    const float* sn = a.sn + (size_t)z * 128;
    c0[ps] = *reinterpret_cast<const f32x4*>(cs + 4 * j); c1[ps] = *reinterpret_cast<const f32x4*>(cs + 64 + 4 * j);
    s0[ps] = *reinterpret_cast<const f32x4*>(sn + 4 * j); s1[ps] = *reinterpret_cast<const f32x4*>(sn + 64 + 4 * j);
  }
  const f32x4 qw0 = *reinterpret_cast<const f32x4*>(a.qw + 4 * j), qw1 = *reinterpret_cast<const f32x4*>(a.qw + 64 + 4 * j);
  if (wlo < whi) kv.load_batch(wlo);

  // ---- q norm + rotation, column by column
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {
    const int c = 8 * w + 4 * ps + (lane >> 4);
    u32x2 p0, p1;
    norm_rope_row(x0r[ps], x1r[ps], qw0, qw1, c0[ps], c1[ps], s0[ps], s1[ps], a.eps, a.und_rounding, p0, p1);
    *reinterpret_cast<u32x2*>(&lds.sq[c][4 * j]) = p0;
    *reinterpret_cast<u32x2*>(&lds.sq[c][64 + 4 * j]) = p1;
  }
  __syncthreads();                                           // every wave reads all 32 columns

  AttnAcc acc;
  const float c2 = a.scale * 1.4426950408889634f;            // p = 2^((s - m) c2)
  if (wlo < whi) {
    bf16x8 qf[8];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(&lds.sq[r32][16 * ks + 8 * hh]);
    int v_lb[2];
    v_frag_base(lane, v_lb);
    for (int k0 = wlo; k0 < whi; k0 += KB) {
      kv.with_k_bf16(false, 0, nullptr, [&](bf16x8 (&kf)[8]) {      // no new row in a prefix
        attn_batch_step(acc, kf, [&](int i) { return kv.v_bf16(i); }, qf, min(KB, whi - k0), k0 == wlo, c2, lds.u.sv[w], v_lb, lane,
                        [&] { if (k0 + KB < whi) kv.load_batch(k0 + KB); });
      });
    }
  }
  __syncthreads();                                           // the V images are free: the results overlay them
  wave_result_to_lds(acc, a.scale, ncol, lane, lds.wm[w], lds.wl[w], lds.u.wo[w]);
  __syncthreads();
  // one partial per (slot, head) column, block nbs + pb of its head
  merge_waves(tid, ncol, lds.wm, lds.wl, lds.u.wo, [&](int c) {
    const int z = z0 + c / G, h = kvh * G + c % G;
    return a.ws + (((size_t)z * Hq + h) * a.NBH + a.NBS + pb) * 130;
  });
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
  decode_attn_pg_body<KvBf16>(sa, lds.s, id % pa.NBS, (id / pa.NBS) % pa.Hkv, id / (pa.NBS * pa.Hkv), pa.NBH,
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
              k_suffix, v_suffix, (float*)workspace, (const int*)suffix_len_dev, Hq, Hkv, scale, (long)suffix_rows,
              suffix_max_len, S, (S + 3) / 4, nullptr, nullptr};
  PrefixArgs pa{(const __bf16*)qkv, (const float*)q_norm_w, (const float*)k_norm_w, (const float*)cos, (const float*)sin, eps, und_rounding,
                (const __bf16*)k_prefix, (const __bf16*)v_prefix, (float*)workspace, batch, Hq, Hkv, scale,
                prefix_len, p.swp, p.nbp, p.spg, p.ngrp, p.nbs, nbh};
  const int blocks = p.nbp * Hkv * p.ngrp + p.nbs * Hkv * batch;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(decode_attn_shared_kernel, dim3(blocks), dim3(256), 0, s, sa, pa G2V_STAMP_PASS_NONE);
  G2V_CHECK_LAUNCH();
  hipLaunchKernelGGL(decode_combine_pg_kernel, dim3(Hq, batch), dim3(1024), 0, s, (const float*)workspace, (__bf16*)out, nbh);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}
