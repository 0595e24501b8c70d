// 256x256x64 bf16 GEMM, FOUR waves (2 M x 2 N), one wave per SIMD, 128-column x (128 ... 144)-row wave tiles.
//
// Why a second form of gemm_8p.hip's kernel: a SIMD issues the instructions of its waves one after the other, so with two
// waves per SIMD the LDS-DMA issue (60-185 cycles a piece), the fragment reads and the barriers of one wave are not hidden
// behind the other wave's MFMAs - they queue in front of them (gemm_8p.hip, staggered: load segment ~1.7 x the MFMA segment,
// 59 % MFMA busy, 1.35 PFLOP/s at 8192^3).  Here every wave owns a whole SIMD and 512 registers: a 128-column wave tile
// needs 0.25 fragment reads per MFMA instead of 0.375, there is ONE barrier per 64-72 MFMAs, and every load instruction is
// hand-placed between two MFMAs of the SAME wave (the matrix pipe runs on while the next instruction issues).  This is the
// shape the vendor library's own 256x256x64 kernels have on this chip (4 waves, 8 x 8 fragments of 16x16 per wave).
//
// Ring, half-tiles, LDS image, hazards: as gemm_8p.hip's software-pipelined form.  Half-tile j = 4 t + c of K-tile t:
// c = 0 A-q0 (rows wr*HB + [0, 16 MA0)), 1 B-q0 (cols wc*128 + [0, 64)), 2 B-q1 (cols wc*128 + [64, 128)), 3 A-q1.  Phase
// p = 4 t + i:  lgkmcnt(0) -> [i == 2: counted vmcnt retiring K-tile t+1] -> [i even: barrier] -> { MFMAs of quadrant i,
// between them: fragment reads for phase p + 1, LDS-DMA of half-tile p + 8 }.
//   quadrant / operands   i=0 (A0, B0)   i=1 (A0, B1)   i=2 (A1, B1)   i=3 (A1, B0)
//   reads issued          B1 of t        A1 of t        A0 of t+1      B0 of t+1 (second B0 register set: B0 of t is in use)
//   DMA issued            A-q0 of t+2    B-q0 of t+2    B-q1 of t+2    A-q1 of t+2
//   RAW  half-tile j is first read in phase j - 2; K-tile t+1's four half-tiles are retired (vmcnt + barrier) at the start of
//        phase 4 t + 2, whose reads are the first of that K-tile.
//   WAR  the slot of half-tile j is overwritten by half-tile j + 8, issued in phase j; its reads were issued in phase j - 2 and
//        retired by every wave's lgkmcnt(0) at the start of phase j - 1.  The barrier in front of phase j (j even) or j - 1 (j
//        odd) therefore lies between every wave's last read of the slot and every wave's DMA into it: TWO barriers per K-tile.
// The LDS-DMA is an asm statement (lds_dma.h): the landing of the pieces is tracked by the counted vmcnt above, not by hipcc.
//
// Same math, epilogues, grouping (und / geo experts) and bf16 rounding points as gemm.hip / gemm_8p.hip (reference: every
// nn.Linear under autocast, e.g. modeling/qwen2vl/modeling_qwen2_vl.py:508-521, modeling/g2vlm/qwen2vl.py:579-606).
//
// This file: the four-wave main loop, its DMA geometry, fragment code and accumulator registers.  Kernel arguments, LDS
// geometry, tile walk, epilogue (it reads the accumulators through acc_get) and the persistent launcher are shared with
// gemm_8p.hip: gemm_tile256.h; gemm_8p.hip packs the arguments and picks the form.
#include "gemm_tile256.h"
#include "lds_dma.h"
#include "gemm_internal.h"

namespace {

constexpr int NT = 256;                                 // four waves

// the K-tile bases are formed by SALU adds from per-tile bases (no VALU-written SGPR): only the M0 write needs its wait state
#ifdef EXP_4W_NO_READS
#define RD(x)
#else
#define RD(x) x
#endif
#ifdef EXP_4W_DMA_NOP4
#define DMA16 dma16_saddr
#else
#define DMA16 dma16_saddr_settled
#endif

// The accumulators live in a0 .. a255, OWNED by this file: hipcc cannot be made to keep 256 accumulator registers in AGPRs
// beside 200 VGPRs of fragments (builtin MFMAs: 2.8 v_accvgpr moves per MFMA and scratch spills in the main loop), so the
// MFMAs are asm statements naming their accumulator registers literally, as in attn.hip's flash_fwd64_kernel; the compiler
// keeps every C++ value in the 256 VGPRs (tests/test_build_cpu.py audits: no compiler-made AGPR use, no scratch).
#define G2V_A8(k) "a" #k "0", "a" #k "1", "a" #k "2", "a" #k "3", "a" #k "4", "a" #k "5", "a" #k "6", "a" #k "7", "a" #k "8", "a" #k "9"
__device__ __forceinline__ void acc_declare() {
  asm volatile("" ::: "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", G2V_A8(1), G2V_A8(2), G2V_A8(3), G2V_A8(4), G2V_A8(5), G2V_A8(6),
               G2V_A8(7), G2V_A8(8), G2V_A8(9), G2V_A8(10), G2V_A8(11), G2V_A8(12), G2V_A8(13), G2V_A8(14), G2V_A8(15), G2V_A8(16), G2V_A8(17),
               G2V_A8(18), G2V_A8(19), G2V_A8(20), G2V_A8(21), G2V_A8(22), G2V_A8(23), G2V_A8(24), "a250", "a251", "a252", "a253", "a254", "a255");
}
template <int R> __device__ __forceinline__ void acc_zero() { asm volatile("v_accvgpr_write_b32 a%c0, 0" :: "i"(R)); }
template <int R> __device__ __forceinline__ float acc_read() { float v; asm volatile("v_accvgpr_read_b32 %0, a%c1" : "=v"(v) : "i"(R)); return v; }
__device__ __forceinline__ void wait32() { asm volatile("s_nop 15\n\ts_nop 15"); }
// a[R .. R+3] += B fragment . A fragment (16x16x32; the operands are swapped so that the accumulator holds C^T fragments)
template <int R> __device__ __forceinline__ void mfma_acc(const bf16x8& b, const bf16x8& a) {
  asm volatile("v_mfma_f32_16x16x32_bf16 a[%c2:%c3], %0, %1, a[%c2:%c3]" :: "v"(b), "v"(a), "i"(R), "i"(R + 3));
}
// the same into a VGPR accumulator (the ninth m-fragment of the 288-row tile: a0 .. a255 hold the first eight)
__device__ __forceinline__ void mfma_vacc(f32x4& c, const bf16x8& b, const bf16x8& a) {
  asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(b), "v"(a));
}

template <int EPI, int MA0, int MA1>
__global__ __launch_bounds__(NT, 1) void gemm4w_kernel(T256Args a) {
  static_assert(MA0 + MA1 <= 9, "256 accumulator AGPRs + 32 VGPRs");
  acc_declare();
  constexpr int MT = MA0 + MA1;                            // 16-row m-fragments per wave
  constexpr int HB = 16 * MT;                              // rows per wave row
  constexpr int BMv = 2 * HB;                              // tile height
  constexpr int MAX_MA = MA0 > MA1 ? MA0 : MA1;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = w >> 1, wc = w & 1;
  const int N = a.N, K = a.K;
  const uint32_t lds0 = __builtin_amdgcn_readfirstlane(lds_addr(smem));
  // ---- DMA geometry.  One wave-instruction fills 8 rows x 128 B (1 KiB, lane-linear): lane -> row srow, 16-B chunk scp;
  // the chunk it FETCHES is scp ^ srow (all staged rows have row & 7 == srow).
  const int srow = lane >> 3, scp = lane & 7;
  const int kcol = (scp ^ srow) << 3;
  // A quadrant q, piece i2 < MAq: linear row L = (4 i2 + w) * 8 of the quadrant's 32 MAq rows; wave row L / (16 MAq)
  // B half q, piece i2 < 4: group gq = w + 4 i2 -> cols (gq >> 3) * 128 + q * 64 + (gq & 7) * 8 + srow
  int a_row[2][MAX_MA], b_col[2][4];
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int i2 = 0; i2 < MAX_MA; ++i2) {
      const int MA = q ? MA1 : MA0;
      const int Lr = min((4 * i2 + w) * 8, 32 * MA - 8);
      a_row[q][i2] = (Lr / (16 * MA)) * HB + (q ? 16 * MA0 : 0) + Lr % (16 * MA);
    }
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int i2 = 0; i2 < 4; ++i2) {
      const int gq = w + 4 * i2;
      b_col[q][i2] = (gq >> 3) * 128 + q * 64 + (gq & 7) * 8;
    }

  struct TileCtx {
    int gi, m0, n0;
    uint32_t a_src[2][MAX_MA], b_src[2][4];                // per-lane byte offsets from the tile's first A row / W row
  };
  // tile id -> context (gemm_tile256.h: XCD remap, supertile walk)
  auto setup_tile = [&](int vt, TileCtx& c) {
    tile_origin<BMv>(a, vt, c.gi, c.m0, c.n0);
    const int gM = a.g[c.gi].M;
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int i2 = 0; i2 < MAX_MA; ++i2)
        c.a_src[q][i2] = ((uint32_t)(min(c.m0 + a_row[q][i2] + srow, gM - 1) - c.m0) * (uint32_t)a.lda + kcol) * 2u;
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int i2 = 0; i2 < 4; ++i2)
        c.b_src[q][i2] = ((uint32_t)(min(c.n0 + b_col[q][i2] + srow, N - 1) - c.n0) * (uint32_t)K + kcol) * 2u;
  };
  // piece i2 of half-tile (t, c) of the tile (Ab, Wb: wave-uniform byte pointers to the tile's first A row / W row)
  auto dma_piece = [&](int t, auto c_, auto i2_, const char* Ab, const char* Wb, const uint32_t (&as)[2][MAX_MA], const uint32_t (&bs)[2][4]) {
    constexpr int c = c_, i2 = i2_;
    const uint32_t slot = lds0 + (uint32_t)((t & 1) * KBUF_BYTES);
    if constexpr (c == 0) DMA16(Ab + (size_t)t * (BK * 2), as[0][i2], slot + (uint32_t)a_row[0][i2] * 128u);
    else if constexpr (c == 3) DMA16(Ab + (size_t)t * (BK * 2), as[1][i2], slot + (uint32_t)a_row[1][i2] * 128u);
    else DMA16(Wb + (size_t)t * (BK * 2), bs[c == 2][i2], slot + (uint32_t)(OP_BYTES + b_col[c == 2][i2] * 128));
  };
  // every piece of half-tile c of K-tile t (MA0, 4, 4, MA1 pieces per wave for c = 0 .. 3)
  auto stage_half = [&](int t, auto c_, const char* Ab, const char* Wb, const uint32_t (&as)[2][MAX_MA], const uint32_t (&bs)[2][4]) {
    constexpr int c = c_;
    constexpr int NP = c == 0 ? MA0 : (c == 3 ? MA1 : 4);
    sfor<NP>([&](auto i2) { dma_piece(t, c_, i2, Ab, Wb, as, bs); });
  };
  // s_waitcnt vmcnt(n): the instruction takes an immediate (vmcnt = bits 3:0 and 15:14; expcnt / lgkmcnt left at their maximum)
  auto wait_vm = [&](auto n_) {
    constexpr int n = n_;
    __builtin_amdgcn_s_waitcnt(0x0F70 | (n & 15) | ((n >> 4) << 14));
  };

  TileCtx cur;
  setup_tile(blockIdx.x, cur);
  bool prefetched = false;                                 // K-tile 0 of `cur` is already in flight / landed in slot 0
  for (int vt = blockIdx.x; vt < a.total; vt += gridDim.x) {
  const T256Group g = a.g[cur.gi];
  const int m0 = cur.m0, n0 = cur.n0;
  const char* Ab = uniform_ptr(reinterpret_cast<const char*>(g.A + (size_t)m0 * a.lda));
  const char* Wb = uniform_ptr(reinterpret_cast<const char*>(g.W + (size_t)n0 * K));
  const int nk = K / BK;

  // accumulator (i, j) = a[4 (8 i + j) .. + 3] holds a C^T fragment (operands swapped in the MFMA): register r of lane
  // (fr, fq) is C[m = i*16 + fr][n = j*16 + fq*4 + r]; j = 4 qb + jj.  Zeroed below, under the prologue's DMA latency.
  // m-fragment 8 (288-row tile only) lives in VGPRs.
  f32x4 acc8[8];
  if constexpr (MT > 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) acc8[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  auto acc_get = [&](auto i_, auto j_, auto r_) -> float {
    constexpr int i = i_, j = j_, r = r_;
    if constexpr (i < 8) return acc_read<4 * (8 * i + j) + r>();
    else return acc8[j][r];
  };

  // ---- fragment read offsets (k-step kk toggles byte bit 6)
  const int fr = lane & 15, fq = lane >> 4;
  const int sw = (fq ^ (fr & 7)) << 4;
  const int aoff = (wr * HB + fr) * 128 + sw;                        // + (qa*16*MA0 + i*16) * 128
  const int boff = OP_BYTES + (wc * 128 + fr) * 128 + sw;            // + (qb*64 + jj*16) * 128

  bf16x8 fa0[MA0][2], fa1[MA1][2], fb0[2][4][2], fb1[4][2];
  // fragment read number r of an operand (r = 2 * fragment + kk)
  auto rd_a0 = [&](const char* base, auto r_) { constexpr int r = r_; fa0[r >> 1][r & 1] = *reinterpret_cast<const bf16x8*>(base + ((aoff + (r >> 1) * 2048) ^ ((r & 1) << 6))); };
  auto rd_a1 = [&](const char* base, auto r_) { constexpr int r = r_; fa1[r >> 1][r & 1] = *reinterpret_cast<const bf16x8*>(base + ((aoff + (16 * MA0 + (r >> 1) * 16) * 128) ^ ((r & 1) << 6))); };
  auto rd_b0 = [&](const char* base, auto set_, auto r_) { constexpr int r = r_, S = set_; fb0[S][r >> 1][r & 1] = *reinterpret_cast<const bf16x8*>(base + ((boff + (r >> 1) * 2048) ^ ((r & 1) << 6))); };
  auto rd_b1 = [&](const char* base, auto r_) { constexpr int r = r_; fb1[r >> 1][r & 1] = *reinterpret_cast<const bf16x8*>(base + ((boff + (64 + (r >> 1) * 16) * 128) ^ ((r & 1) << 6))); };

  // MFMA number m of quadrant (QA, QB): kk-major, then m-fragment, then n-fragment; S = the B0 register set in use
  auto mfma_one = [&](auto qa_, auto qb_, auto set_, auto m_) {
    constexpr int QA = qa_, QB = qb_, S = set_, m = m_;
    constexpr int MAq = QA ? MA1 : MA0;
    constexpr int kk = m / (4 * MAq), i = (m % (4 * MAq)) / 4, jj = m % 4;
    constexpr int I = QA * MA0 + i, J = QB * 4 + jj, R = 4 * (8 * I + J);
    const bf16x8& av = [&]() -> const bf16x8& { if constexpr (QA == 0) return fa0[i][kk]; else return fa1[i][kk]; }();
    const bf16x8& bv = [&]() -> const bf16x8& { if constexpr (QB == 0) return fb0[S][jj][kk]; else return fb1[jj][kk]; }();
    if constexpr (I < 8) mfma_acc<R>(bv, av);
    else mfma_vacc(acc8[J], bv, av);
  };
  // one phase: NM MFMAs with NF fillers spread evenly between them (filler f follows MFMA floor-spaced), order pinned
  auto phase = [&](auto qa_, auto qb_, auto set_, auto nf_, auto&& filler) {
    constexpr int QA = qa_, NF = nf_;
    constexpr int NM = 8 * (QA ? MA1 : MA0);
    sfor<NM>([&](auto m_) {
      constexpr int m = m_;
      mfma_one(qa_, qb_, set_, m_);
      constexpr int f_lo = (m * NF + NM - 1) / NM, f_hi = ((m + 1) * NF + NM - 1) / NM;   // ceil(m NF / NM) .. ceil((m+1) NF / NM)
      if constexpr (f_hi > f_lo) {
        __builtin_amdgcn_sched_barrier(0);
        sfor<f_hi - f_lo>([&](auto d_) { filler(std::integral_constant<int, f_lo + decltype(d_)::value>{}); });
        __builtin_amdgcn_sched_barrier(0);
      }
    });
  };
  auto begin_phase = [&](auto barrier_) {
    __builtin_amdgcn_s_waitcnt(0xC07F);                    /* lgkmcnt(0) */
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (decltype(barrier_)::value) {
#ifndef EXP_4W_NO_BARRIER
      __builtin_amdgcn_s_barrier();
#endif
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  // K-tile t.  SET: the B0 register set holding B0 of t (the other one receives B0 of t+1).  STEADY: K-tile t + 2 exists:
  // no per-piece conditions inside the MFMA stream.
  auto ktile = [&](int t, auto set_, auto steady_) {
    constexpr int S = set_;
    constexpr bool STEADY = steady_;
    const char* base = smem + (t & 1) * KBUF_BYTES;
    const char* nbase = smem + ((t + 1) & 1) * KBUF_BYTES;
    // EXP_4W_* (tools/gemm4w_ablate.sh): timing ablations only, wrong results; the shipped library defines none of them
    auto dma = [&](int tt, auto c_, auto i2) {             // piece i2 of half-tile c of K-tile tt
#ifndef EXP_4W_NO_DMA
      if (STEADY || tt < nk) dma_piece(tt, c_, i2, Ab, Wb, cur.a_src, cur.b_src);
#endif
    };
    using C0 = std::integral_constant<int, 0>; using C1 = std::integral_constant<int, 1>;
    using C2 = std::integral_constant<int, 2>; using C3 = std::integral_constant<int, 3>;
    // phase 0: barrier | (A0, B0) | reads B1 of t | DMA A-q0 of t+2
    begin_phase(std::true_type{});
    phase(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, set_, std::integral_constant<int, 8 + MA0>{}, [&](auto f_) {
      constexpr int f = f_;
      if constexpr (f < 8) { RD(rd_b1(base, f_)); }
      else dma(t + 2, C0{}, std::integral_constant<int, f - 8>{});
    });
    // phase 1: (A0, B1) | reads A1 of t | DMA B-q0 of t+2
    begin_phase(std::false_type{});
    phase(std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{}, set_, std::integral_constant<int, 2 * MA1 + 4>{}, [&](auto f_) {
      constexpr int f = f_;
      if constexpr (f < 2 * MA1) { RD(rd_a1(base, f_)); }
      else dma(t + 2, C1{}, std::integral_constant<int, f - 2 * MA1>{});
    });
    // phase 2: retire K-tile t+1 (the two youngest half-tiles - A-q0, B-q0 of t+2 - stay in flight) | barrier | (A1, B1) |
    // reads A0 of t+1 | DMA B-q1 of t+2
    __builtin_amdgcn_s_waitcnt(0xC07F);                    /* lgkmcnt(0) */
    if (STEADY || t + 2 < nk) wait_vm(std::integral_constant<int, MA0 + 4>{});
    else __builtin_amdgcn_s_waitcnt(0x0F70);               /* vmcnt(0) */
    __builtin_amdgcn_sched_barrier(0);
#ifndef EXP_4W_NO_BARRIER
    __builtin_amdgcn_s_barrier();
#endif
    __builtin_amdgcn_sched_barrier(0);
    phase(std::integral_constant<int, 1>{}, std::integral_constant<int, 1>{}, set_, std::integral_constant<int, 2 * MA0 + 4>{}, [&](auto f_) {
      constexpr int f = f_;
      if constexpr (f < 2 * MA0) { RD(rd_a0(nbase, f_)); }
      else dma(t + 2, C2{}, std::integral_constant<int, f - 2 * MA0>{});
    });
    // phase 3: (A1, B0) | reads B0 of t+1 into the other register set | DMA A-q1 of t+2
    begin_phase(std::false_type{});
    phase(std::integral_constant<int, 1>{}, std::integral_constant<int, 0>{}, set_, std::integral_constant<int, 8 + MA1>{}, [&](auto f_) {
      constexpr int f = f_;
      if constexpr (f < 8) { RD(rd_b0(nbase, std::integral_constant<int, S ^ 1>{}, f_)); }
      else dma(t + 2, C3{}, std::integral_constant<int, f - 8>{});
    });
  };

  // ---- prologue: K-tiles 0 and 1 in flight, K-tile 0 retired, its A0 / B0 fragments read
  if (!prefetched) sfor<4>([&](auto c) { stage_half(0, c, Ab, Wb, cur.a_src, cur.b_src); });
  sfor<4>([&](auto c) { stage_half(1, c, Ab, Wb, cur.a_src, cur.b_src); });   // nk >= 2 (g2v_gemm_8p_supported)
  sfor<32 * (MT < 8 ? MT : 8)>([&](auto r) { acc_zero<decltype(r)::value>(); });
  wait_vm(std::integral_constant<int, MT + 8>{});          // K-tile 1's four half-tiles stay in flight
  __builtin_amdgcn_s_barrier();
  sfor<2 * MA0>([&](auto r) { rd_a0(smem, r); });
  sfor<8>([&](auto r) { rd_b0(smem, std::integral_constant<int, 0>{}, r); });
  __builtin_amdgcn_s_waitcnt(0xC07F);                      /* lgkmcnt(0) */

  {
    int t = 0;
    for (; t + 3 < nk; t += 2) {                           // t + 1 + 2 < nk: both K-tiles are steady
      ktile(t, std::integral_constant<int, 0>{}, std::true_type{});
      ktile(t + 1, std::integral_constant<int, 1>{}, std::true_type{});
    }
    for (; t < nk; t += 2) {
      ktile(t, std::integral_constant<int, 0>{}, std::false_type{});
      if (t + 1 < nk) ktile(t + 1, std::integral_constant<int, 1>{}, std::false_type{});
    }
  }
  __builtin_amdgcn_s_waitcnt(0xC07F);                      /* lgkmcnt(0) */
  __builtin_amdgcn_s_barrier();                            // the epilogue reuses the LDS the last reads came from
  wait32();                                                // the last MFMAs' results are in their registers before v_accvgpr_read

  // ---- the next tile of this workgroup: its first K-tile goes into ring slot 0 now (every wave is past its last LDS
  // read), and lands while the epilogue below runs out of the LDS above slot 0
  const int vn = vt + gridDim.x;
  const bool has_next = vn < a.total;
  if (has_next) {
    setup_tile(vn, cur);                                   // m0 / n0 / g of the tile being finished are in locals
    const T256Group& gn_ = a.g[cur.gi];
    const char* An = uniform_ptr(reinterpret_cast<const char*>(gn_.A + (size_t)cur.m0 * a.lda));
    const char* Wn = uniform_ptr(reinterpret_cast<const char*>(gn_.W + (size_t)cur.n0 * K));
    sfor<4>([&](auto c) { stage_half(0, c, An, Wn, cur.a_src, cur.b_src); });
  }

#ifdef EXP_4W_NO_EPI
  __builtin_amdgcn_s_barrier();
  prefetched = has_next;
  continue;
#endif
  tile_epilogue<EPI, MT, NT, 8>(a, g, smem, tid, wr, wc, m0, n0, acc_get);
  prefetched = has_next;
  }
}

template <int EPI, int MA0, int MA1>
int launch_h(const T256Args& a, hipStream_t s) { return launch_persistent<gemm4w_kernel<EPI, MA0, MA1>, NT>(a, s); }

template <int EPI>
int launch(const T256Args& a, int bm, hipStream_t s) {
  if (bm == 288) return launch_h<EPI, 5, 4>(a, s);
#ifndef G2V_4W_FEW                                           // G2V_4W_FEW: tests/test_build_cpu.py audits a subset of the instantiations
  if (bm == 256) return launch_h<EPI, 4, 4>(a, s);
  if (bm == 224) return launch_h<EPI, 4, 3>(a, s);
  if (bm == 192) return launch_h<EPI, 4, 2>(a, s);
#endif
  if (bm == 160) return launch_h<EPI, 3, 2>(a, s);
  return launch_h<EPI, 2, 2>(a, s);
}

}  // namespace

// Same eligibility as gemm_8p.hip (g2v_gemm_8p_supported); the arguments are packed and the tile height is chosen there.
int g2v_gemm_4w_launch(const T256Args& a, int epilogue, int bm, hipStream_t s) {
  return g2v_gemm_with_epilogue(epilogue, [&](auto epi) {
    constexpr int EPI = decltype(epi)::value;
#ifdef G2V_4W_FEW
    if constexpr (EPI != G2V_EPI_SWIGLU && EPI != G2V_EPI_RES_F32) return G2V_ERR_ARG; else
#endif
    return launch<EPI>(a, bm, s);
  });
}

