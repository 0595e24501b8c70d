// Private: everything the two forms of the persistent 256x256x64 bf16 GEMM share - gemm_8p.hip (eight waves, three main
// loops) and gemm_4w.hip (four waves, accumulators in a0 .. a255).  The forms differ in their main loops, DMA geometry and
// fragment code only; the kernel arguments, the LDS geometry, the tile walk, the epilogue and the launcher are here, once.
#pragma once
#include <type_traits>
#include <utility>
#include "common.h"
#include "g2vlm_hip.h"

// kernel arguments of both forms: the large group first, tile_start = first tile id of the group, sm x sn = supertile,
// total = tiles of the launch (the first 16 dwords arrive preloaded in SGPRs: keep the field order)
struct T256Group {
  const __bf16* A; const __bf16* W; const __bf16* bias; void* C; const void* res; const float* gamma;
  int M, tile_start;
};
struct T256Args {
  T256Group g[2];
  int ngroups, N, K, lda, ldc, ldres, tiles_n, flags, sm, sn, total;
};

// compute units a persistent launch may fill, asked once per process: a multiple of 8, so that a workgroup keeps its XCD
// group across tiles (0: the query failed)
inline int g2v_persistent_cus() {
  static int n_cu = 0;
  if (n_cu == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
    n_cu = prop.multiProcessorCount & ~7;
    if (n_cu <= 0) n_cu = 256;
  }
  return n_cu;
}

namespace {

constexpr int BN = 256, BK = 64;
constexpr int BM_MAX = 288;
constexpr int OP_BYTES = BM_MAX * 128;                   // A tile: up to 288 rows x 128 B = 36 KiB; the 256-row B tile follows it
constexpr int KBUF_BYTES = OP_BYTES + 256 * 128;         // A + B = 68 KiB per K-tile slot, two slots
constexpr int OUT_PITCH = 256 * 2 + 16;                  // epilogue staging: bf16 [bm][256] rows padded by 16 B (conflict-free b64 writes)
constexpr int LDS_BYTES = KBUF_BYTES + 160 * OUT_PITCH;  // epilogue image (<= 160 rows per pass) sits above ring slot 0: 150.5 KiB of 160

// compile-time loop: f(std::integral_constant<int, 0>{}) ... f(std::integral_constant<int, N - 1>{})
template <class F, int... I>
__device__ __forceinline__ void sfor_impl(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void sfor(F&& f) { sfor_impl(f, std::make_integer_sequence<int, N>{}); }

// tile id -> group and origin of a BM-row tile: XCD-aware bijective remap, then a supertile walk, column first
template <int BM>
__device__ __forceinline__ void tile_origin(const T256Args& a, int vt, int& gi, int& m0, int& n0) {
  const int nwg = a.total;
  int bid = vt;
  {
    int xcd = bid & 7, qn = nwg >> 3, rn = nwg & 7;
    bid = (xcd < rn ? xcd * (qn + 1) : rn * (qn + 1) + (xcd - rn) * qn) + (bid >> 3);
  }
  gi = (a.ngroups > 1 && bid >= a.g[1].tile_start) ? 1 : 0;
  const int t_id = bid - a.g[gi].tile_start;
  const int tiles_m = (a.g[gi].M + BM - 1) / BM;
  const int row_sz = a.sm * a.tiles_n;
  int sup_m = t_id / row_sz, r = t_id - sup_m * row_sz;
  int h = min(a.sm, tiles_m - sup_m * a.sm);
  int full_w = a.sn * h;
  int sup_n = r / full_w, p = r - sup_n * full_w;
  m0 = (sup_m * a.sm + p % h) * BM;                        // walk down the column first: consecutive tiles share the W slab
  n0 = (sup_n * a.sn + p / h) * BN;
}

// Epilogue of one tile of group g at (m0, n0), for a block of NT threads = 2 wave rows x NT/128 wave columns, each wave holding
// MT m-fragments x NJ n-fragments of C^T: acc(i, j, r), called with std::integral_constants, is C[m = i*16 + fr][n = j*16 +
// fq*4 + r] of lane (fr, fq) - four consecutive columns of one row.  Two passes over the m-fragments (i < I0, then the rest), each:
// (1) every lane rounds its accumulators to the bf16 Linear output (bias, activation) and writes them, 4 consecutive
//     columns = 8 bytes at a time, into a row-major bf16 image in LDS: image row wr*16*I0 + (i - h*I0)*16 + fr;
// (2) the block walks that image in 16-byte chunks, 32 (16 for SwiGLU) consecutive lanes per output row, so every
//     global access - output store, and for the residual forms the fp32/bf16 residual load - is a full 16-byte
//     lane access on 512 (256) contiguous bytes per row instead of 2- and 4-byte scattered ones.
// Every wave must be past its last read of the LDS above ring slot 0; ends with a barrier.
template <int EPI, int MT, int NT, int NJ, class Acc>
__device__ __forceinline__ void tile_epilogue(const T256Args& a, const T256Group& g, char* smem, int tid, int wr, int wc, int m0, int n0, Acc&& acc) {
  constexpr bool SWI = EPI == G2V_EPI_SWIGLU;
  constexpr int HB = 16 * MT;                              // rows per wave row
  constexpr int PITCH = OUT_PITCH;
  constexpr int I0 = (MT + 1) / 2;                         // m-fragments per pass
  constexpr int CPR = SWI ? 16 : 32;                       // 16-byte chunks per output row
  constexpr int RPI = NT / CPR;                            // rows per sweep
  const int M = g.M;
  char* const img = smem + KBUF_BYTES;
  // the lane constants are recomputed per tile from an opaque copy of the thread id: hoisted out of the persistent loop
  // they would sit in (or spill from) the registers the main loop needs
  int etid = tid;
  asm volatile("" : "+v"(etid));
  const int efr = etid & 15, efq = (etid >> 4) & 3;
  const int ch = etid % CPR, r0 = etid / CPR;
  const int gn = (SWI ? (n0 >> 1) : n0) + ch * 8;          // first of this lane's 8 output columns
  const bool round_gamma = a.flags & G2V_GEMM_GAMMA_ROUND_BF16;
  // this lane's 16 bytes of image row r0, and its 8 columns of row 0 of C and of the residual: the sweep adds whole rows, so
  // an image row is an immediate offset of the LDS read and a global address one 64-bit multiply-add
  using OutT = std::conditional_t<EPI == G2V_EPI_RES_F32, float, __bf16>;
  const char* const rd = img + r0 * PITCH + ch * 16;
  OutT* const cl = reinterpret_cast<OutT*>(g.C) + gn;
  const OutT* const rl = reinterpret_cast<const OutT*>(g.res) + gn;
  sfor<2>([&](auto h_) {
    constexpr int h = h_;
    const int irow0 = wr * 16 * I0 + efr;
    if constexpr (SWI) {
      sfor<I0>([&](auto ii_) {
        constexpr int ii = ii_, i = h * I0 + ii;
        if constexpr (i < MT) {
          sfor<NJ / 2>([&](auto jp_) {
            constexpr int jp = jp_;
            float o[4];
            sfor<4>([&](auto r_) {
              constexpr int r = r_;
              float gt = bfround(acc(std::integral_constant<int, i>{}, std::integral_constant<int, 2 * jp>{}, r_));
              float up = bfround(acc(std::integral_constant<int, i>{}, std::integral_constant<int, 2 * jp + 1>{}, r_));
              float sl = bfround(siluf_fast_(gt));
              o[r] = sl * up;
            });
            *reinterpret_cast<u32x2*>(img + (irow0 + ii * 16) * PITCH + (wc * NJ * 8 + jp * 16 + efq * 4) * 2) =
                u32x2{pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3])};
          });
        }
      });
    } else {
      sfor<NJ>([&](auto j_) {
        constexpr int j = j_;
        const int cl = wc * NJ * 16 + j * 16 + efq * 4;
        float bv[4] = {0.f, 0.f, 0.f, 0.f};
        if (g.bias) {
          u32x2 bb = *reinterpret_cast<const u32x2*>(g.bias + n0 + cl);
          bv[0] = bits2f_lo(bb[0]); bv[1] = bits2f_hi(bb[0]); bv[2] = bits2f_lo(bb[1]); bv[3] = bits2f_hi(bb[1]);
        }
        sfor<I0>([&](auto ii_) {
          constexpr int ii = ii_, i = h * I0 + ii;
          if constexpr (i < MT) {
            float o[4];
            sfor<4>([&](auto r_) {
              constexpr int r = r_;
              float v = bfround(acc(std::integral_constant<int, i>{}, j_, r_) + bv[r]);
              if constexpr (EPI == G2V_EPI_GELU) v = gelu_fast(v);
              if constexpr (EPI == G2V_EPI_QUICKGELU) {
                float u = bfround(1.702f * v);
                float sg = bfround(sigmoidf_(u));
                v = v * sg;
              }
              o[r] = v;
            });
            *reinterpret_cast<u32x2*>(img + (irow0 + ii * 16) * PITCH + cl * 2) = u32x2{pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3])};
          }
        });
      });
    }
    float gam[8];
    bool has_gam = false;
    if constexpr (EPI == G2V_EPI_RES_F32) {
      has_gam = g.gamma != nullptr;
      if (has_gam) {
        f32x4 g0 = *reinterpret_cast<const f32x4*>(g.gamma + gn), g1 = *reinterpret_cast<const f32x4*>(g.gamma + gn + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { gam[e] = g0[e]; gam[4 + e] = g1[e]; }
      }
    }
    __syncthreads();
    // sweep in batches: residual loads and LDS reads of a batch are all issued before the first store waits on them
    constexpr int NIT = 2 * 16 * I0 / RPI;
    constexpr int SB = NIT % 5 == 0 ? 5 : (NIT % 4 == 0 ? 4 : (NIT % 3 == 0 ? 3 : 2));
    static_assert(NIT % SB == 0, "sweep batches");
#pragma unroll
    for (int it0 = 0; it0 < NIT; it0 += SB) {
      u32x4 pk[SB];
      int gmv[SB];
      bool ok[SB];
      [[maybe_unused]] f32x4 ra[SB], rb[SB];
      [[maybe_unused]] u32x4 rr[SB];
#pragma unroll
      for (int c = 0; c < SB; ++c) {
        const int irow = (it0 + c) * RPI + r0;
        const int iwr = irow / (16 * I0), rem = irow - iwr * (16 * I0);
        const int trow = h * 16 * I0 + rem;                // row inside the wave row
        gmv[c] = m0 + iwr * HB + trow;
        ok[c] = trow < HB && gmv[c] < M;
        if constexpr (EPI == G2V_EPI_RES_F32) {
          ra[c] = rb[c] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (ok[c] && g.res) {
            const float* rp = rl + (size_t)gmv[c] * a.ldres;
            ra[c] = *reinterpret_cast<const f32x4*>(rp); rb[c] = *reinterpret_cast<const f32x4*>(rp + 4);
          }
        } else if constexpr (EPI == G2V_EPI_RES_BF16) {
          rr[c] = u32x4{0u, 0u, 0u, 0u};
          if (ok[c]) rr[c] = *reinterpret_cast<const u32x4*>(rl + (size_t)gmv[c] * a.ldres);
        }
      }
#pragma unroll
      for (int c = 0; c < SB; ++c) pk[c] = *reinterpret_cast<const u32x4*>(rd + (it0 + c) * RPI * PITCH);
#pragma unroll
      for (int c = 0; c < SB; ++c) {
        if (!ok[c]) continue;
        const int gm = gmv[c];
        if constexpr (EPI == G2V_EPI_RES_F32) {
          float v[8];
#pragma unroll
          for (int e = 0; e < 4; ++e) { v[2 * e] = bits2f_lo(pk[c][e]); v[2 * e + 1] = bits2f_hi(pk[c][e]); }
          if (has_gam) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              v[e] = __fmul_rn(v[e], gam[e]);
              if (round_gamma) v[e] = bfround(v[e]);
            }
          }
          float* cp = cl + (size_t)gm * a.ldc;
          *reinterpret_cast<f32x4*>(cp) = f32x4{__fadd_rn(ra[c][0], v[0]), __fadd_rn(ra[c][1], v[1]), __fadd_rn(ra[c][2], v[2]), __fadd_rn(ra[c][3], v[3])};
          *reinterpret_cast<f32x4*>(cp + 4) = f32x4{__fadd_rn(rb[c][0], v[4]), __fadd_rn(rb[c][1], v[5]), __fadd_rn(rb[c][2], v[6]), __fadd_rn(rb[c][3], v[7])};
        } else if constexpr (EPI == G2V_EPI_RES_BF16) {
          u32x4 ov;
#pragma unroll
          for (int e = 0; e < 4; ++e)
            ov[e] = pack_bf16x2(bits2f_lo(rr[c][e]) + bits2f_lo(pk[c][e]), bits2f_hi(rr[c][e]) + bits2f_hi(pk[c][e]));
          *reinterpret_cast<u32x4*>(cl + (size_t)gm * a.ldc) = ov;
        } else {
          *reinterpret_cast<u32x4*>(cl + (size_t)gm * a.ldc) = pk[c];
        }
      }
    }
    __syncthreads();                                      // the image is dead: the second pass / the next tile's DMA may overwrite it
  });
}

// one workgroup of NT threads per CU (or per tile when there are fewer) walks the a.total tiles
template <auto KERNEL, int NT>
int launch_persistent(const T256Args& a, hipStream_t s) {
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES) != hipSuccess)
      return G2V_ERR_LAUNCH;
    attr_set = true;
  }
  const int n_cu = g2v_persistent_cus();
  if (n_cu == 0) return G2V_ERR_LAUNCH;
  hipLaunchKernelGGL(KERNEL, dim3(a.total < n_cu ? a.total : n_cu), dim3(NT), LDS_BYTES, s, a);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

}  // namespace
