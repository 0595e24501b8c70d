// The k largest entries of every row of bf16 logits, in order (Engine.score_rows / score_questions with top_k > 0: what the
// model preferred at a scored position).  The order is g2v_argmax_rows_bf16's total order (misc.hip: argmax_key /
// argmax_merge, restated below): larger value first, -0 == +0, every NaN above +inf, equal keys by ascending index.  No two
// elements of a row are equal in it, so the answer is unique: entry j is the element with exactly j elements before it.
//
// Work split: logprob.hip's.  Elements are grouped BY INDEX: chunk c is the TK_CHUNK elements [8192 c, 8192 c + 8192), thread
// t of the workgroup that takes it owns the four 8-element vectors 1024 c + 256 u + t, u < 4 - 32 keys in registers, ascending
// in index.  A wave selects its k best by k rounds of "wave maximum of the lanes' best (DPP), the lane that held it rescans
// its 32 keys for its best element BEHIND the winner"; the four waves' sorted lists and the workgroup's running list (held by
// wave 0, entry j in lane j) are merged by the same rounds over three candidates per lane.  From its second chunk on a
// workgroup carries its running k-th element as a threshold: a wave stops its rounds at the first winner that does not beat it.
// While the rows alone do not fill the chip a row is dealt out to S workgroups (chunks slice, slice + S, ..), which leave
// their sorted k-lists in `scratch`; the last to arrive (one ticket per row) merges them.  Nobody waits for anybody.
// The selected values are read again from x at the end (the key forgets the sign of a zero and a NaN's payload).
#include "common.h"
#include "g2vlm_hip.h"

namespace {

constexpr int TK_THREADS = 256, TK_U = 4, TK_E = TK_U * 8, TK_CHUNK = TK_THREADS * TK_E;
constexpr int TK_SPLIT_ROWS = 512;                         // two workgroups per CU: from here on the rows fill the chip by themselves
constexpr int TK_MERGE_E = 3;                              // (4 wave lists + the running list) * 32 entries over 64 lanes
constexpr int TK_KEY_NAN = 0x7fffffff;
constexpr int TK_KEY_NONE = (int)0x80000000;               // below -inf's key: "no element"; always paired with TK_IDX_NONE
constexpr int TK_IDX_NONE = 0x7fffffff;

// misc.hip's argmax_key on the bf16 bit pattern: monotone in the value, -0 == +0, every NaN on top
__device__ __forceinline__ int tk_key(uint32_t bf16_bits) {
  const int b = (int)(bf16_bits << 16);
  const int m = b & 0x7fffffff;
  return m > 0x7f800000 ? TK_KEY_NAN : (m == 0 ? 0 : (b >= 0 ? b : (b ^ 0x7fffffff)));
}
// misc.hip's argmax_merge: (ok, oi) replaces (best, bi) when it comes before it in the order
__device__ __forceinline__ bool tk_before(int ak, int ai, int bk, int bi) { return ak > bk || (ak == bk && ai < bi); }
__device__ __forceinline__ void tk_merge(int& best, int& bi, int ok, int oi) {
  if (tk_before(ok, oi, best, bi)) { best = ok; bi = oi; }
}

template <int CTRL>
__device__ __forceinline__ int tk_dpp(int x) {
  return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xF, 0xF, true);
}
// the first (key, index) of the 64 lanes' pairs, in every lane (and in scalar registers): DPP inside the 16-lane rows
// (row_ror 8, 4, 2, 1: every lane of a row ends with the row's first), the four rows through readlane - logprob.hip's
// wave_max_dpp for pairs
__device__ __forceinline__ void tk_wave_first(int& k, int& i) {
  tk_merge(k, i, tk_dpp<0x128>(k), tk_dpp<0x128>(i));
  tk_merge(k, i, tk_dpp<0x124>(k), tk_dpp<0x124>(i));
  tk_merge(k, i, tk_dpp<0x122>(k), tk_dpp<0x122>(i));
  tk_merge(k, i, tk_dpp<0x121>(k), tk_dpp<0x121>(i));
  int rk = __builtin_amdgcn_readlane(k, 0), ri = __builtin_amdgcn_readlane(i, 0);
  tk_merge(rk, ri, __builtin_amdgcn_readlane(k, 16), __builtin_amdgcn_readlane(i, 16));
  tk_merge(rk, ri, __builtin_amdgcn_readlane(k, 32), __builtin_amdgcn_readlane(i, 32));
  tk_merge(rk, ri, __builtin_amdgcn_readlane(k, 48), __builtin_amdgcn_readlane(i, 48));
  k = rk; i = ri;
}

// the keys of the 8 elements [e0, e0 + 8) of a row; elements >= n are "no element".  Loads as logprob.hip's lp_load8.
__device__ __forceinline__ void tk_load8(const __bf16* row, long e0, int n, int align, int* key) {
  const uint16_t* r16 = reinterpret_cast<const uint16_t*>(row);
  if (e0 + 8 <= (long)n && align == 0) {
    const u32x4 w = *reinterpret_cast<const u32x4*>(row + e0);
#pragma unroll
    for (int k = 0; k < 4; ++k) { key[2 * k] = tk_key(w[k] & 0xffffu); key[2 * k + 1] = tk_key(w[k] >> 16); }
  } else if (e0 + 8 <= (long)n && align == 1) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(row + e0);
#pragma unroll
    for (int k = 0; k < 4; ++k) { const uint32_t w = p[k]; key[2 * k] = tk_key(w & 0xffffu); key[2 * k + 1] = tk_key(w >> 16); }
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) key[k] = (e0 + k < (long)n) ? tk_key(r16[e0 + k]) : TK_KEY_NONE;
  }
}

// a lane's first element strictly behind (lk, li) among its 32 chunk keys; element e has index i0 + 2048 (e / 8) + e % 8,
// ascending in e, so among equal keys the first one met stays
__device__ __forceinline__ void tk_rescan_chunk(const int (&key)[TK_E], int i0, int lk, int li, int& bk, int& bi) {
  bk = TK_KEY_NONE; bi = TK_IDX_NONE;
#pragma unroll
  for (int e = 0; e < TK_E; ++e) {
    const int i = i0 + (e >> 3) * (TK_THREADS * 8) + (e & 7);
    if (key[e] > bk && tk_before(lk, li, key[e], i)) { bk = key[e]; bi = i; }
  }
}
// the same among E (key, index) candidates in any order
template <int E>
__device__ __forceinline__ void tk_rescan(const int (&ck)[E], const int (&ci)[E], int lk, int li, int& bk, int& bi) {
  bk = TK_KEY_NONE; bi = TK_IDX_NONE;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    if (tk_before(ck[e], ci[e], bk, bi) && tk_before(lk, li, ck[e], ci[e])) { bk = ck[e]; bi = ci[e]; }
  }
}
// k rounds over one wave's candidates, E per lane: the sorted list's entry j ends in lane j's (rk, ri); entries the
// candidates do not fill are "no element"
template <int E>
__device__ __forceinline__ void tk_merge_rounds(const int (&ck)[E], const int (&ci)[E], int k, int lane, int& rk, int& ri) {
  int bk, bi;
  tk_rescan<E>(ck, ci, TK_KEY_NAN, -1, bk, bi);            // (NaN key, index -1) comes before every element
  rk = TK_KEY_NONE; ri = TK_IDX_NONE;
  for (int j = 0; j < k; ++j) {
    int wk = bk, wi = bi;
    tk_wave_first(wk, wi);
    if (wk == TK_KEY_NONE) break;
    if (lane == j) { rk = wk; ri = wi; }
    if (bk == wk && bi == wi) tk_rescan<E>(ck, ci, wk, wi, bk, bi);
  }
}

// grid: rows * S workgroups; workgroup b takes the chunks b % S, b % S + S, ... of row b / S.
// scratch (S > 1 only, which implies rows < TK_SPLIT_ROWS): int32 [TK_SPLIT_ROWS] arrival tickets, one per row (zeroed once by
// the caller, reset here; their place does not depend on the launch), then per (row, slice) k pairs {key, index}.
__global__ __launch_bounds__(TK_THREADS) void topk_rows_bf16_kernel(const __bf16* x, int n, long ld, int k, int* out_idx, float* out_val,
                                                                    int S, int* scratch) {
  __shared__ int wl_key[TK_THREADS / 64][G2V_TOPK_MAX], wl_idx[TK_THREADS / 64][G2V_TOPK_MAX];
  __shared__ int thr_key, thr_idx, last;
  const int row = blockIdx.x / S, slice = blockIdx.x % S;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const __bf16* xr = x + (size_t)row * ld;
  const uintptr_t addr = reinterpret_cast<uintptr_t>(xr);
  const int align = (addr & 15) == 0 ? 0 : ((addr & 3) == 0 ? 1 : 2);
  const int nc = (int)(((long)n + TK_CHUNK - 1) / TK_CHUNK);
  int rk = TK_KEY_NONE, ri = TK_IDX_NONE;                    // wave 0: entry `lane` of the workgroup's running list
  int tk = TK_KEY_NONE, ti = TK_IDX_NONE;                    // its k-th entry: what a new element has to beat

  for (int c = slice; c < nc; c += S) {
    int key[TK_E];
#pragma unroll
    for (int u = 0; u < TK_U; ++u) tk_load8(xr, (long)c * TK_CHUNK + ((long)u * TK_THREADS + tid) * 8, n, align, key + 8 * u);
    const int i0 = (int)((unsigned)c * TK_CHUNK + (unsigned)tid * 8);
    int bk, bi;
    tk_rescan_chunk(key, i0, TK_KEY_NAN, -1, bk, bi);
    int cnt = 0;
    for (; cnt < k; ++cnt) {
      int wk = bk, wi = bi;
      tk_wave_first(wk, wi);
      if (!tk_before(wk, wi, tk, ti)) break;                 // behind the running k-th (or no element left): so is all that follows
      if (lane == 0) { wl_key[wv][cnt] = wk; wl_idx[wv][cnt] = wi; }
      if (bk == wk && bi == wi) tk_rescan_chunk(key, i0, wk, wi, bk, bi);
    }
    if (lane >= cnt && lane < G2V_TOPK_MAX) { wl_key[wv][lane] = TK_KEY_NONE; wl_idx[wv][lane] = TK_IDX_NONE; }
    __syncthreads();
    if (wv == 0) {
      int ck[TK_MERGE_E], ci[TK_MERGE_E];
      ck[0] = rk; ci[0] = ri;
#pragma unroll
      for (int e = 1; e < TK_MERGE_E; ++e) {
        const int w = (e - 1) * 2 + (lane >> 5), j = lane & 31;
        ck[e] = wl_key[w][j]; ci[e] = wl_idx[w][j];
      }
      tk_merge_rounds<TK_MERGE_E>(ck, ci, k, lane, rk, ri);
      if (lane == k - 1) { thr_key = rk; thr_idx = ri; }
    }
    __syncthreads();
    tk = __builtin_amdgcn_readfirstlane(thr_key); ti = __builtin_amdgcn_readfirstlane(thr_idx);   // uniform: the rounds' exit is a scalar branch
  }

  if (S > 1) {                                               // the workgroup that arrives last merges the row's lists
    int* part = scratch + TK_SPLIT_ROWS + (size_t)row * S * 2 * k;
    if (wv == 0) {                                           // one wave stores, fences and takes the ticket: its fence covers its lanes' stores
      if (lane < k) {
        __hip_atomic_store(part + ((size_t)slice * k + lane) * 2, rk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(part + ((size_t)slice * k + lane) * 2 + 1, ri, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (lane == 0) {
        const int t = __hip_atomic_fetch_add(scratch + row, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = (t == S - 1);
      }
    }
    __syncthreads();
    if (!last || wv != 0) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    // S k <= 64 * 32 entries: rounds of 4 lists' worth (<= 128 entries, two per lane) merged into the running list in turn
    rk = TK_KEY_NONE; ri = TK_IDX_NONE;
    const int total = S * k;
    for (int e0 = 0; e0 < total; e0 += 128) {
      int ck[TK_MERGE_E], ci[TK_MERGE_E];
      ck[0] = rk; ci[0] = ri;
#pragma unroll
      for (int e = 1; e < TK_MERGE_E; ++e) {
        const int j = e0 + (e - 1) * 64 + lane;
        ck[e] = TK_KEY_NONE; ci[e] = TK_IDX_NONE;
        if (j < total) {
          ck[e] = __hip_atomic_load(part + (size_t)j * 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          ci[e] = __hip_atomic_load(part + (size_t)j * 2 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      tk_merge_rounds<TK_MERGE_E>(ck, ci, k, lane, rk, ri);
    }
    if (lane == 0) __hip_atomic_store(scratch + row, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (wv == 0 && lane < k) {
    const bool some = rk != TK_KEY_NONE && ri >= 0 && ri < n;   // an index written is ALWAYS one of the row, or -1
    out_idx[(size_t)row * k + lane] = some ? ri : -1;
    if (out_val) {
      const uint32_t bits = some ? ((uint32_t) reinterpret_cast<const uint16_t*>(xr)[ri]) << 16 : 0x7fc00000u;
      out_val[(size_t)row * k + lane] = __uint_as_float(bits);
    }
  }
}

// workgroups per row: 1 once the rows alone give every CU two workgroups, else enough slices to get there
inline int tk_slices(int rows, int n) {
  const long nc = ((long)n + TK_CHUNK - 1) / TK_CHUNK;
  const long want = rows >= TK_SPLIT_ROWS ? 1 : (TK_SPLIT_ROWS + rows - 1) / rows;
  return (int)(want < nc ? want : nc);
}

}  // namespace

extern "C" int64_t g2v_topk_rows_workspace(int rows, int n, int k) {
  if (rows <= 0 || n <= 0 || k < 1 || k > G2V_TOPK_MAX || tk_slices(rows, n) <= 1) return 0;
  return 4 * ((int64_t)TK_SPLIT_ROWS + (int64_t)rows * tk_slices(rows, n) * 2 * k);
}

extern "C" int g2v_topk_rows_bf16(const void* x, int rows, int n, int64_t ld, int k, void* out_idx, void* out_val, void* scratch,
                                  int64_t scratch_bytes, void* stream) {
  if (!x || !out_idx || rows <= 0 || n <= 0 || ld < n || k < 1 || k > G2V_TOPK_MAX) return G2V_ERR_ARG;
  int S = tk_slices(rows, n);
  if (S > 1 && (!scratch || scratch_bytes < g2v_topk_rows_workspace(rows, n, k))) S = 1;   // no scratch: one workgroup per row
  if ((int64_t)rows * S > 0x7fffffffLL) return G2V_ERR_ARG;
  hipLaunchKernelGGL(topk_rows_bf16_kernel, dim3((unsigned)(rows * S)), dim3(TK_THREADS), 0, (hipStream_t)stream, (const __bf16*)x, n,
                     (long)ld, k, (int*)out_idx, (float*)out_val, S, (int*)scratch);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}
