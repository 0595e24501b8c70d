// Host-side plan of the persistent-grid GEMVs (decode_layer.hip, decode_batch.hip, decode_fp8.hip): the one place that
// decides which kernel instantiation, block size and batch depth serve a shape.  g2v_gemv_pg, g2v_gemv_pg_fp8,
// g2v_gemv_pg_batch and g2v_gemv_pg_batch_fp8 check their pointers, call pg::plan and launch what it picked;
// g2v_gemv_pg_route reports the same plan without touching a device.  No device code here.
#pragma once
#include <type_traits>
#include <utility>

#include "common.h"

namespace pg {

// Ascending list of the values a template parameter is instantiated with.
struct List {
  int n, v[7];
  constexpr int cap() const { return v[n - 1]; }
  constexpr int fit(int x) const {                           // the first entry that holds x (the last if none does)
    for (int i = 0; i < n; ++i)
      if (x <= v[i]) return v[i];
    return cap();
  }
};

// RB (units per batch; the last entry is the register cap) of gemv_pg_kernel / gemv_pg8_kernel (nb == 0) and of
// gemv_pgb_kernel / gemv_pgb8_kernel (nb = 2, 4, 8 scenes per weight pass).
// Batch 1: ROWS x KCH x 4 registers per batch; a long-K row is 18 loads per lane in bf16 (two rows spill), 9 in e4m3.
// Batched: NB x RB <= 32 values are reduced together; an e4m3 unit is a row pair (12 registers, 16 NB of activation).
constexpr List rbs(bool fp8, int nb, bool act, bool longk) {
  if (nb == 0) {
    if (longk) return fp8 ? List{2, {1, 2}} : List{1, {1}};
    if (act) return fp8 ? List{5, {1, 2, 3, 4, 6}} : List{5, {1, 2, 3, 4, 5}};
    return fp8 ? List{7, {1, 2, 3, 4, 6, 8, 12}} : List{7, {1, 2, 3, 4, 5, 6, 8}};
  }
  if (fp8) return nb == 8 ? List{2, {1, 2}} : List{3, {1, 2, 4}};
  return nb == 8 ? List{2, {1, 2}} : (nb == 4 ? List{3, {1, 2, 3}} : List{4, {1, 2, 3, 5}});
}

// f(std::integral_constant<int, RB>) for the entry of rbs(FP8, NB, ACT, LONGK) that equals rb: the planned batch depth
// becomes a template argument, and exactly the listed depths are instantiated
template <bool FP8, int NB, bool ACT, bool LONGK, class F, int... I>
void with_rb_(int rb, F&& f, std::integer_sequence<int, I...>) {
  constexpr List l = rbs(FP8, NB, ACT, LONGK);
  (..., (rb == l.v[I] ? f(std::integral_constant<int, l.v[I]>{}) : void()));
}
template <bool FP8, int NB, bool ACT, bool LONGK, class F>
void with_rb(int rb, F&& f) {
  with_rb_<FP8, NB, ACT, LONGK>(rb, f, std::make_integer_sequence<int, rbs(FP8, NB, ACT, LONGK).n>{});
}

// the same for the scenes per weight pass: B = 1..8 rows run as NB = 2, 4 or 8
constexpr List NBS = {3, {2, 4, 8}};
template <class F>
int with_nb(int nb, F&& f) {
  if (nb == 2) return f(std::integral_constant<int, 2>{});
  if (nb == 4) return f(std::integral_constant<int, 4>{});
  return f(std::integral_constant<int, 8>{});
}

// several equal batches rather than a full one and a remainder
inline int equal_batches(int per_wave, int cap) {
  if (per_wave <= cap) return per_wave;
  const int nbat = (per_wave + cap - 1) / cap;
  return (per_wave + nbat - 1) / nbat;
}

// Waves per block of the batch-1 kernels: the count (3..8) that splits the U units most evenly over 256 blocks; a wave then
// takes ceil(U / waves) units.  Ties go to MORE waves for a streaming kernel (loads in flight per CU) and to FEWER, fatter
// waves for a small one (< 48 KB per CU: all of it is in flight either way, and 1536 waves take ~1.4 us to dispatch - half
// of a 3 us kernel, profiles/r02f_decode_stamps.txt: wave life 2.1 us, kernel span 3.5 us)
inline int pick_waves(int U, double bytes_per_cu, int rb_cap) {
  const bool small = bytes_per_cu < 48.0 * 1024.0;
  int best = 4;
  double best_imb = 1e30;
  for (int t = 0; t < 6; ++t) {
    const int nwb = small ? 3 + t : 8 - t;
    const long nw = 256L * nwb;
    const double per = (double)U / nw;
    const double imb = per >= 1.0 ? (double)((U + nw - 1) / nw) / per : 1.0 / per;
    if (small && (U + nw - 1) / nw > rb_cap && best_imb < 1e29) continue;    // a small kernel is ONE batch per wave
    if (imb < best_imb - 1e-9) { best_imb = imb; best = nwb; }
  }
  return best;
}

// form 1: gemv_pg_kernel / gemv_pg8_kernel <.., KCH = kch, RB = rb>, 256 blocks of `threads`, wave gw takes uq (+1 if gw < ur) units
// form 2: gemv_pgb_kernel / gemv_pgb8_kernel <.., NB = nb, RB = rb>, 256 blocks of 8 waves, units split the same way
// form 3: gemv_pgk_kernel / gemv_pgk8_kernel <NB = nb>: a block owns `per` rows and streams them rb (the kernel's R) at a
//         time; kch is the K chunks per wave (CW, bf16: 8 waves) or the waves per block (S, e4m3: one per 1024 elements)
struct Plan { int form, threads, rb, kch, nb, uq, ur, per; };

constexpr int NORM_K = 1536;   // the fused norm keeps (batch 1) or stages (batched) whole fp32 rows: hidden-size K

// B == 0: the batch-1 entry points (K <= 9216); B = 1..8: the batched ones (K <= 12288).  K % 8 == 0 in bf16, % 16 in e4m3.
// act: the MLP's first half, gate/up interleaved per 16 rows with the norm fused.  G2V_ERR_ARG exactly where a launch is refused.
inline int plan(int B, int N, int K, bool act, bool norm, bool fp8, Plan& p) {
  if (B < 0 || B > 8 || N <= 0 || K <= 0 || K % (fp8 ? 16 : 8) || K > (B ? 12288 : 9216)) return G2V_ERR_ARG;
  if ((act && ((N & 31) || !norm)) || (norm && K > NORM_K)) return G2V_ERR_ARG;
  if (B == 0) {
    const bool longk = K > (fp8 ? 2048 : NORM_K);
    const List l = rbs(fp8, 0, act, longk);
    const int U = act ? N / 2 : N;
    const int nwb = pick_waves(U, (double)N * K * (fp8 ? 1.0 : 2.0) / 256.0, l.cap()), waves = 256 * nwb;
    p = Plan{1, 64 * nwb, l.fit(equal_batches((U + waves - 1) / waves, l.cap())), fp8 ? (longk ? 9 : 2) : (longk ? 18 : 3), 0,
             U / waves, U % waves, 0};
    return G2V_OK;
  }
  const int nb = NBS.fit(B);
  if (K > NORM_K) {                                          // long K (down): the K axis is cut over the waves of a block
    const int S = (K / 16 + 63) / 64, CW = (K / 8 + 7) / 8;
    p = fp8 ? Plan{3, 64 * S, nb == 8 ? 4 : 8, S, nb, 0, 0, (N + 255) / 256} : Plan{3, 512, 6, CW, nb, 0, 0, (N + 255) / 256};
    return G2V_OK;
  }
  const List l = rbs(fp8, nb, act, false);
  const int U = fp8 ? (N + 1) / 2 : (act ? N / 2 : N), waves = 256 * 8;   // e4m3 units: pairs of rows (act: gate and up row)
  const int uq = U / waves, ur = U % waves;
  p = Plan{2, 512, l.fit(equal_batches(uq + (ur ? 1 : 0), l.cap())), fp8 ? 2 : 3, nb, uq, ur, 0};
  return G2V_OK;
}

}  // namespace pg
