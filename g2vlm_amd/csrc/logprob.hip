// Log-probability of one target id per row of bf16 logits: log_softmax(x.float(), -1)[target], the row's logsumexp and the
// target's rank, in ONE pass over the row (Engine.score_rows: teacher-forced scoring of candidate answers).
//
// Work split.  Elements are grouped BY INDEX, never by address: vector v of a row holds elements [8 v, 8 v + 8), chunk c the
// vectors [1024 c, 1024 c + 1024) = LP_CHUNK elements; thread t of the workgroup that takes chunk c owns vectors 1024 c + 256 u + t,
// u < 4.  A chunk is reduced to one partial (max, sum exp(x - max), rank count) by a fixed tree: lane -> wave (DPP) -> the
// four waves in order; the row's partials are merged in ascending chunk order.  Which workgroup computes a chunk changes
// nothing in that, so the result has the same bits whether a row's chunks are taken by one workgroup (many rows) or dealt
// out to several (few rows: the vocabulary of one row alone is 300 KB, far too little for one CU to be worth waiting for
// 255 others), and whatever the row's base address is: a row whose base is 16-byte aligned is read with 16-byte loads, a
// row that is not (odd ld) with 4- or 2-byte loads of the same elements into the same slots.  The last vector of a row is
// read element by element, so columns [n, ld) are never touched.
#include "decode_util.h"
#include "g2vlm_hip.h"

namespace {

constexpr int LP_THREADS = 256, LP_U = 4, LP_CHUNK = LP_THREADS * LP_U * 8;
constexpr float LP_L2E = 1.4426950408889634f;
constexpr int LP_SPLIT_ROWS = 512;                         // two workgroups per CU: from here on the rows fill the chip by themselves

template <int CTRL>
__device__ __forceinline__ int dpp_i(int x) {
  return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xF, 0xF, true);
}
// 64-lane max / integer sum: DPP inside the 16-lane rows (row_ror 8, 4, 2, 1: every lane of a row ends with the row's
// result), the four rows through scalar registers - decode_util.h's wave_sum_dpp for the other two operators
__device__ __forceinline__ float wave_max_dpp(float x) {
  x = fmaxf(x, dpp_f<0x128>(x));
  x = fmaxf(x, dpp_f<0x124>(x));
  x = fmaxf(x, dpp_f<0x122>(x));
  x = fmaxf(x, dpp_f<0x121>(x));
  return fmaxf(fmaxf(readlane_f(x, 0), readlane_f(x, 16)), fmaxf(readlane_f(x, 32), readlane_f(x, 48)));
}
__device__ __forceinline__ int wave_sum_dpp_i(int x) {
  x += dpp_i<0x128>(x);
  x += dpp_i<0x124>(x);
  x += dpp_i<0x122>(x);
  x += dpp_i<0x121>(x);
  return (__builtin_amdgcn_readlane(x, 0) + __builtin_amdgcn_readlane(x, 16)) +
         (__builtin_amdgcn_readlane(x, 32) + __builtin_amdgcn_readlane(x, 48));
}

// exp(a - b) for a <= b; 1 when they are equal, which covers a == b == -inf (nothing finite seen yet, the sum is 0)
__device__ __forceinline__ float lp_scale(float a, float b) {
  return a == b ? 1.0f : __builtin_amdgcn_exp2f((a - b) * LP_L2E);
}
// (M, S) <- (M, S) merged with (m, s): the one place partial sums meet, always in the same order (waves 0..3, chunks 0..)
__device__ __forceinline__ void lp_merge(float& M, float& S, float m, float s) {
  const float nm = fmaxf(M, m);
  S = fmaf(S, lp_scale(M, nm), s * lp_scale(m, nm));
  M = nm;
}

// the 8 elements [e0, e0 + 8) of a row; elements >= n read as -inf
__device__ __forceinline__ void lp_load8(const __bf16* row, long e0, int n, int align, float (&v)[8]) {
  if (e0 + 8 <= (long)n && align == 0) {
    const u32x4 w = *reinterpret_cast<const u32x4*>(row + e0);
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[2 * k] = bits2f_lo(w[k]); v[2 * k + 1] = bits2f_hi(w[k]); }
  } else if (e0 + 8 <= (long)n && align == 1) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(row + e0);
#pragma unroll
    for (int k = 0; k < 4; ++k) { const uint32_t w = p[k]; v[2 * k] = bits2f_lo(w); v[2 * k + 1] = bits2f_hi(w); }
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (e0 + k < (long)n) ? bf2f(row[e0 + k]) : -INFINITY;
  }
}

// grid: rows * S workgroups; workgroup b takes the chunks b % S, b % S + S, ... of row b / S.
// scratch (S > 1 only, which implies rows < LP_SPLIT_ROWS): int32 [LP_SPLIT_ROWS] arrival tickets, one per row (zeroed once by
// the caller, reset here; their place does not depend on the launch, so launches of any shape can share one scratch), then
// per row nc_max partials of 3 words {max, sum, count}.
__global__ __launch_bounds__(LP_THREADS) void logprob_rows_bf16_kernel(const __bf16* x, int n, long ld, const int* targets, float* out_lp,
                                                                       float* out_lse, int* out_rank, int S, int nc_max, int* scratch) {
  __shared__ float sm[LP_THREADS], ss[LP_THREADS];
  __shared__ int sc[LP_THREADS];
  __shared__ int last;
  const int row = blockIdx.x / S, slice = blockIdx.x % S;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const __bf16* xr = x + (size_t)row * ld;
  const uintptr_t addr = reinterpret_cast<uintptr_t>(xr);
  const int align = (addr & 15) == 0 ? 0 : ((addr & 3) == 0 ? 1 : 2);
  const int t = targets[row];
  const bool valid = t >= 0 && t < n;
  const float xt = valid ? bf2f(xr[t]) : __builtin_nanf("");   // NaN compares false with everything: the count stays 0
  const int nc = (int)(((long)n + LP_CHUNK - 1) / LP_CHUNK);
  float M = -INFINITY, S_ = 0.0f;                            // thread 0 of a workgroup that owns the whole row: the running merge
  int R = 0;
  float* part = S > 1 ? reinterpret_cast<float*>(scratch + LP_SPLIT_ROWS) + (size_t)row * nc_max * 3 : nullptr;

  for (int c = slice; c < nc; c += S) {
    float v[LP_U][8];
#pragma unroll
    for (int u = 0; u < LP_U; ++u) lp_load8(xr, (long)c * LP_CHUNK + ((long)u * LP_THREADS + tid) * 8, n, align, v[u]);
    float m = -INFINITY;
    int cnt = 0;
#pragma unroll
    for (int u = 0; u < LP_U; ++u) {
      const long e0 = (long)c * LP_CHUNK + ((long)u * LP_THREADS + tid) * 8;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        m = fmaxf(m, v[u][k]);
        cnt += (v[u][k] > xt || (v[u][k] == xt && e0 + k < (long)t)) ? 1 : 0;
      }
    }
    const float m0 = m == -INFINITY ? 0.0f : m;              // an all -inf lane: exp2(-inf - 0) = 0, not exp2(-inf + inf)
    float s = 0.0f;
#pragma unroll
    for (int u = 0; u < LP_U; ++u) {
#pragma unroll
      for (int k = 0; k < 8; ++k) s += __builtin_amdgcn_exp2f((v[u][k] - m0) * LP_L2E);
    }
    const float mw = wave_max_dpp(m);
    s = wave_sum_dpp(s * lp_scale(m, mw));
    cnt = wave_sum_dpp_i(cnt);
    if (lane == 0) { sm[wv] = mw; ss[wv] = s; sc[wv] = cnt; }
    __syncthreads();
    if (tid == 0) {
      float pm = sm[0], ps = ss[0];
      int pc = sc[0];
      for (int k = 1; k < LP_THREADS / 64; ++k) { lp_merge(pm, ps, sm[k], ss[k]); pc += sc[k]; }
      if (S > 1) {
        __hip_atomic_store(part + 3 * c, pm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(part + 3 * c + 1, ps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(reinterpret_cast<int*>(part) + 3 * c + 2, pc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else {
        lp_merge(M, S_, pm, ps);
        R += pc;
      }
    }
    __syncthreads();
  }

  if (S > 1) {                                               // the workgroup that arrives last merges the row's partials
    if (tid == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const int k = __hip_atomic_fetch_add(scratch + row, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      last = (k == S - 1);
    }
    __syncthreads();
    if (!last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    for (int c0 = 0; c0 < nc; c0 += LP_THREADS) {            // loads side by side, the merge itself in chunk order
      if (c0 + tid < nc) {
        sm[tid] = __hip_atomic_load(part + 3 * (c0 + tid), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ss[tid] = __hip_atomic_load(part + 3 * (c0 + tid) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sc[tid] = __hip_atomic_load(reinterpret_cast<int*>(part) + 3 * (c0 + tid) + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      __syncthreads();
      if (tid == 0) {
        for (int k = 0; k < min(LP_THREADS, nc - c0); ++k) { lp_merge(M, S_, sm[k], ss[k]); R += sc[k]; }
      }
      __syncthreads();
    }
    if (tid == 0) __hip_atomic_store(scratch + row, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (tid == 0) {
    const bool none = M == -INFINITY;                       // every entry -inf: logsumexp -inf, and a -inf target gives -inf here too
    const float lg = logf(S_);
    out_lp[row] = valid ? (none ? -INFINITY : (xt - M) - lg) : __builtin_nanf("");
    if (out_lse) out_lse[row] = none ? -INFINITY : M + lg;
    if (out_rank) out_rank[row] = valid ? R : -1;
  }
}

// workgroups per row: 1 once the rows alone give every CU two workgroups, else enough slices to get there
inline int lp_slices(int rows, int n) {
  const long nc = ((long)n + LP_CHUNK - 1) / LP_CHUNK;
  const long want = rows >= LP_SPLIT_ROWS ? 1 : (LP_SPLIT_ROWS + rows - 1) / rows;
  return (int)(want < nc ? want : nc);
}

}  // namespace

extern "C" int64_t g2v_logprob_rows_workspace(int rows, int n) {
  if (rows <= 0 || n <= 0 || lp_slices(rows, n) <= 1) return 0;
  const int64_t nc = ((int64_t)n + LP_CHUNK - 1) / LP_CHUNK;
  return 4 * ((int64_t)LP_SPLIT_ROWS + (int64_t)rows * nc * 3);
}

extern "C" int g2v_logprob_rows_bf16(const void* x, int rows, int n, int64_t ld, const void* targets, void* out_lp, void* out_lse,
                                     void* out_rank, void* scratch, int64_t scratch_bytes, void* stream) {
  if (!x || !targets || !out_lp || rows <= 0 || n <= 0 || ld < n) return G2V_ERR_ARG;
  int S = lp_slices(rows, n);
  if (S > 1 && (!scratch || scratch_bytes < g2v_logprob_rows_workspace(rows, n))) S = 1;   // no scratch: one workgroup per row
  if ((int64_t)rows * S > 0x7fffffffLL) return G2V_ERR_ARG;
  const int nc = (int)(((int64_t)n + LP_CHUNK - 1) / LP_CHUNK);
  hipLaunchKernelGGL(logprob_rows_bf16_kernel, dim3((unsigned)(rows * S)), dim3(LP_THREADS), 0, (hipStream_t)stream, (const __bf16*)x, n,
                     (long)ld, (const int*)targets, (float*)out_lp, (float*)out_lse, (int*)out_rank, S, nc, (int*)scratch);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}
