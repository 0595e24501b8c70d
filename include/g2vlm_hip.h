/* libg2vlm_hip.so — C ABI of the MI355X (gfx950) kernels behind the G2VLM inference hot path.
 *
 * The reference (ushariRanasinghe/G2VLM) has NO in-repo native/FFI interface: its native work is
 * done by third-party wheels reached from Python.  Each entry point below names
 * the reference call site(s) it replaces; INTEGRATION.md shows the ctypes binding a maintainer
 * of the reference would add.  Conventions (last row):
 *   - plain pointers and ints only; every pointer is DEVICE memory owned by the caller unless
 *     marked "host"; kernels allocate nothing and keep no global state;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous
 *     and re-entrant across streams;
 *   - return 0 on success, negative errno-style code otherwise (-22 bad argument, -5 launch
 *     failure); nothing throws.
 *   - bf16 = raw uint16 storage, row-major; "ld*" are row strides in ELEMENTS.
 */
#ifndef G2VLM_HIP_H
#define G2VLM_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int g2v_version(void);              /* ABI version, currently 1 */
const char* g2v_arch(void);         /* "gfx950" */

/* ---- GEMM: every nn.Linear / patch conv under autocast(bf16) (SURVEY K-k, K-l, K-m) ---------- */
enum {
  G2V_EPI_BF16 = 0,      /* C(bf16) = bf16(acc + bias)                                              */
  G2V_EPI_GELU = 1,      /* C(bf16) = bf16(gelu_erf(bf16(acc + bias)))     dinov2_model.py:174-177   */
  G2V_EPI_QUICKGELU = 2, /* x*sigmoid(1.702x) with the reference's 3 bf16 roundings (ViT MLP)       */
  G2V_EPI_SWIGLU = 3,    /* W = gate/up interleaved per 16 columns; C(bf16)[M,N/2] = silu(g)*u
                            modeling_qwen2_vl.py:519-521                                            */
  G2V_EPI_RES_F32 = 4,   /* C(f32) = res(f32 or NULL) + [bf16]( bf16(acc+bias) * gamma(f32 or NULL) )
                            dinov2_model.py:233-245, qwen2vl.py:883-909                             */
  G2V_EPI_RES_BF16 = 5   /* C(bf16) = bf16(res(bf16) + bf16(acc+bias))   modeling_qwen2_vl.py:476-482 */
};
#define G2V_GEMM_GAMMA_ROUND_BF16 1 /* flags: round (linear*gamma) to bf16 (MoT ls1/ls2 `.to(bf16)`) */
#define G2V_GEMM_SUPERTILE 4        /* flags: big-tile kernel walks 4x8 supertiles (L2 reuse experiment)         */
#define G2V_GEMM_FORCE_BIG_TILE 8   /* flags: always use the 256-wide DMA-staged kernel when K%64==0 && N%256==0  */
#define G2V_GEMM_FORCE_8P 16        /* flags: always use the 256x256 8-phase kernel (gemm_8p.hip) when K%64==0 && N%256==0  */
/* A/B testing of the 8-phase kernel's variants (tools/bench_kernels.py, tests): a forced tile height, or the two-barrier main loop */
#define G2V_GEMM_8P_H192 128
#define G2V_GEMM_8P_H128 256
#define G2V_GEMM_8P_H256 512
#define G2V_GEMM_8P_TWO_BARRIER 1024
#define G2V_GEMM_8P_H288 4096
#define G2V_GEMM_8P_H224 8192
#define G2V_GEMM_8P_H160 16384
#define G2V_GEMM_8P_PIPELINED 32768 /* A/B: round 1's main loop (one barrier per phase, reads of phase p+1 before the MFMAs of p) */
/* 256x256x64 tile, two bit-identical forms; without either flag the launcher picks by shape class (gemm_8p.hip, G2V_GEMM_4W_MASK) */
#define G2V_GEMM_8P_FOUR_WAVES 65536   /* force gemm_4w.hip: four waves, one per SIMD, 128-column wave tiles, accumulators in AGPRs */
#define G2V_GEMM_8P_NO_ROW_SKIP 262144 /* A/B: wave rows without a valid row run their MFMAs anyway (gemm_8p.hip) */
#define G2V_GEMM_8P_EIGHT_WAVES 131072 /* force gemm_8p.hip: eight waves, the two wave rows staggered by one barrier (round 2) */
#define G2V_GEMM_FORCE_SMALL_TILE 2 /* flags: always use the 128x128 register-staged kernel (A/B testing)  */

typedef struct {
  const void* A;     /* bf16 [M, lda]                         */
  const void* W;     /* bf16 [N, K]  (nn.Linear.weight)       */
  const void* bias;  /* bf16 [N] or NULL                      */
  void* C;           /* output, row stride ldc                */
  const void* res;   /* residual (epilogue 4: f32, 5: bf16), row stride ldres, may alias C */
  const void* gamma; /* f32 [N] layer-scale or NULL           */
  int32_t M;
  int32_t _pad;
} g2v_gemm_group;

typedef struct {
  g2v_gemm_group g[2]; /* two row-partitioned problems sharing N,K,epilogue = und / geo experts */
  int32_t ngroups, N, K, lda, ldc, ldres, epilogue, flags;
  /* optional device scratch for the skinny (M <= 64) path's cross-workgroup K split: `workspace_bytes` bytes, ZEROED ONCE
   * by the caller (arrival tickets live at its head and reset themselves), not shared by launches that may overlap on
   * different streams.  NULL: the split stays inside a workgroup (slower for small N).  A few MiB cover every shape.   */
  void* workspace;
  int64_t workspace_bytes;
} g2v_gemm_desc;       /* host struct */

int g2v_gemm_bf16(const g2v_gemm_desc* desc, void* stream);
/* What g2v_gemm_bf16 launches for `desc` (host only, no launch; tests and tools): out = {form, tile height, S, KS}.
 * form 1 = 128x128 (gemm.hip), 2 = big tile (gemm_big.hip), 3 = eight-wave 256x256 (gemm_8p.hip), 4 = four-wave
 * 256x256 (gemm_4w.hip), 5 = skinny (gemm_skinny.hip, height = its m-tile rows 16 / 32 / 64); S / KS = the skinny
 * kernel's K split inside / across workgroups (1 elsewhere).  Returns what g2v_gemm_bf16 would for a bad descriptor. */
int g2v_gemm_route(const g2v_gemm_desc* desc, int32_t out[4]);

/* fp32 islands (autocast disabled): Pi3LinearPts3d.proj, Pi3CameraHead linears
 * (transformer_head.py:75, camera_head.py:26-29).  C = [relu](A x W^T + bias) [+ res]            */
int g2v_gemm_f32(const void* A, const void* W, const void* bias, void* C, const void* res,
                 int M, int N, int K, int lda, int ldc, int ldres, int relu, void* stream);

/* ---- norms ------------------------------------------------------------------------------------ */
#define G2V_F32 0
#define G2V_BF16 1
/* nn.LayerNorm in fp32 (autocast fp32 op), dinov2_model.py:225,240,351; block.py:316-320.
 * x [M,C] (f32 or bf16) -> out [M,C] (f32 or bf16)                                               */
int g2v_layernorm(const void* x, int x_dtype, int ldx, const void* w, const void* b, float eps,
                  void* out, int out_dtype, int ldo, int M, int C, void* stream);
/* Qwen2RMSNorm (modeling_qwen2_vl.py:496-501) with expert routing by row range: rows < split use
 * w_lo, rows >= split use w_hi (qwen2vl.py:861-865, 897-898, 1325-1329).  x f32 [M,C].            */
int g2v_rmsnorm(const void* x, int ldx, const void* w_lo, const void* w_hi, int split, float eps,
                void* out, int out_dtype, int ldo, int M, int C, void* stream);

/* ---- LLM rotary + qk-norm + KV-cache write ---------------------------------------------------- */
/* Qwen2VLRotaryEmbedding.forward + mrope section select (modeling_qwen2_vl.py:142-166, 223-225).
 * pos int32 [3,L] -> cos,sin f32 [L,128]                                                         */
int g2v_mrope_table(const void* pos, int L, const void* inv_freq /* f32[64] */, void* cos, void* sin, void* stream);
/* qwen2vl.py:572-576 / 596-619 / 626-634 fused: per-head RMSNorm(128) of q,k with routed weights,
 * mRoPE in fp32, cast to bf16; q -> q_out [L,Hq,128]; k,v -> cache rows kv_rows[i] of
 * k_cache/v_cache [*,Hkv,128].  qkv bf16 [L, (Hq+2Hkv)*128].  und_rounding=1 replicates the
 * bf16 round of the normalised value in und mode (bf16 input to Qwen2RMSNorm).                   */
int g2v_qknorm_mrope_cache(const void* qkv, int L, int Hq, int Hkv,
                           const void* qw_lo, const void* qw_hi, const void* kw_lo, const void* kw_hi,
                           int split, float eps, int und_rounding, const void* cos, const void* sin,
                           void* q_out, void* k_cache, void* v_cache, const void* kv_rows, void* stream);

/* ---- attention: flash_attn_varlen_func / SDPA-flash call sites (SURVEY K-a,b,c,d) ------------- */
typedef struct {
  int32_t q0, q_rows;     /* query rows [q0, q0+q_rows) (<= tile_rows) of one window               */
  int32_t k0, k_len;      /* keys [k0, k0+k_len) of that window                                    */
  int32_t causal_shift;   /* key j allowed iff j - k0 <= (q - q_win0) + shift; INT32_MAX/2 = none.
                           * Every query row of a descriptor must be allowed at least one key (shift >= 0 for a
                           * window's first row): the output of a row without a key is UNDEFINED here (NaN from
                           * 0 x 1/0, or never written); make_attn_plan refuses causal windows with k_len < q_len. */
  int32_t q_win0;         /* first query row of the window                                         */
  int32_t _pad[2];
} g2v_attn_tile;          /* device array, one entry per (window, 128-row query tile)              */

/* Persistent schedule, built by the host (g2vlm_amd/hip.py::make_attn_plan).  An ITEM is (tile descriptor, head); its KV
 * window is walked in 64-key tiles.  Workgroup b runs segments segs[seg_ptr[b] .. seg_ptr[b+1]):                          */
typedef struct {
  int32_t desc;           /* index into `tiles`                                                            */
  int32_t head;           /* query head                                                                    */
  int32_t kt0, kt1;       /* 64-key KV tiles [kt0, kt1) of the descriptor's window                           */
  int32_t slot;           /* < 0: the segment covers the item's whole KV work and writes the normalised bf16 output;
                             >= 0: it leaves unnormalised fp32 partials (m, l, O) in workspace slot `slot`            */
  int32_t _pad[3];
} g2v_attn_seg;
/* `comb` (device int32 [n_comb][4]) = (descriptor, head, first slot, number of slots): the output rows of that descriptor
 * and head are merged from those consecutive slots by a second launch (n_comb = 0: none).  Slots of one output tile may
 * come from different descriptors with the same query rows (disjoint KV windows: local block / remote blocks of the
 * view-sharded prefill) and from EARLIER calls on the same workspace: a call with n_blocks = 0 only merges.
 * tile_rows = query rows per descriptor at most: 128 (4-wave workgroups) or 256 (8-wave workgroups).
 * `workspace`: g2v_flash_attn_workspace(n_slots) bytes of fp32 scratch.                                                  */
int64_t g2v_flash_attn_workspace(int n_slots);
/* A/B switch for tools and tests (process-wide, not for production use): which kernel serves head dim 128 with 256-row items.
 * 1 (default) = 4 waves x 64 query rows, one wave per SIMD (flash_fwd64_kernel); 0 = the 8 waves x 32 rows form.  Both implement
 * the same contract; they differ in fp32 summation order and in the softmax reference (exact row maximum vs a power of two).     */
int g2v_debug_attn_form(int form);
int g2v_flash_attn(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv,
                   void* o, int ldo, const g2v_attn_tile* tiles, int n_tiles,
                   int Hq, int Hkv, int D, float scale,
                   const g2v_attn_seg* segs, const int32_t* seg_ptr, int n_blocks, const int32_t* comb, int n_comb,
                   int tile_rows, void* workspace, void* stream);

/* ---- decoders' RoPE2D (pos_embed.py:112-159), in place on the q and k thirds of a fused qkv ---- */
/* x bf16 rows [M, ld]; for each of n_heads heads at column col0 + h*D: 2-D rope with the bf16 tables
 * cos/sin [max_pos, D/2] (built on the host exactly as the reference does, hazard H3);
 * pos int32 [P,2] (y,x), row r uses pos[r % P].                                                  */
int g2v_rope2d(void* x, int ld, int M, int col0, int n_heads, int D, const void* cos, const void* sin,
               const void* pos, int P, void* stream);

/* Qwen2-VL ViT rope (apply_rotary_pos_emb_vision, modeling_qwen2_vl.py:235-246): fp32 rotate-half
 * rope on n_heads heads of width D starting at x (bf16 rows [M, ld]); cos/sin f32 [M, D]            */
int g2v_rope_vision(void* x, int ld, int M, int n_heads, int D, const void* cos, const void* sin, void* stream);

/* ---- DINO front end (modeling_dinov2_with_registers.py:62-71, 147-171) ------------------------ */
/* ToTensor + Normalize + the original_images copy of prepare_dino_images_pi3 (g2vlm.py:947-953) on the device:
 * in = the loader's uint8 frames [N,H,W,3] (in_is_u8) or an f32 [N,3,H,W] image in [0,1]; norm f32 [N,3,H,W] =
 * (x - mean) / std, orig f32 [N,3,H,W] = x (may be NULL); mean3 / std3 host floats.  Bit-identical to the host ops.  */
int g2v_dino_preprocess(const void* in, int in_is_u8, int N, int H, int W, const float* mean3, const float* std3, void* norm,
                        void* orig, void* stream);

/* PIL's Image.resize(size, LANCZOS) on uint8 RGB frames (what the reference's loader calls per image,
 * data/transforms_vggt.py:437), bit-exact: src u8 [N, Hin, Win, 3] -> dst u8 [N, Hout, Wout, 3].  bounds_* int32 [out, 2]
 * (first tap, taps) and kk_* int32 [out, ksize] are Pillow's 22-bit fixed-point tap tables for the x and the y axis, built on
 * the host (g2vlm_amd/host.py::lanczos_tables); an axis whose size does not change takes no pass (tables may be NULL);
 * tmp: u8 [N, Hin, Wout, 3] scratch when both axes change.                                                              */
int g2v_lanczos_resize_u8(const void* src, int N, int Hin, int Win, void* dst, int Hout, int Wout, void* tmp,
                          const void* bounds_h, const void* kk_h, int ksize_h,
                          const void* bounds_v, const void* kk_v, int ksize_v, void* stream);
/* im2col of 14x14/14 patches: img f32 [N,3,H,W] -> bf16 [N*P, Kpad] (K=588 zero-padded)           */
int g2v_im2col14(const void* img, int N, int H, int W, void* out, int Kpad, void* stream);
/* x f32 [N, 5+P, C] = {cls+pos[0], reg0..3, patch[p] + pos[1+p]}; patch bf16 [N*P, C]             */
int g2v_dino_assemble(const void* patch, const void* cls, const void* regs, const void* pos,
                      void* x, int N, int P, int C, void* stream);

/* DINOv3 front end (modeling/dinov3/dinov3_model.py:47-69): Conv2d patch/patch under autocast = im2col (K = 3*patch^2,
 * zero-padded to Kpad) + g2v_gemm_bf16; then [cls | R register tokens | patch rows] per view, fp32, no position table
 * (positions enter as RoPE on q/k: g2v_rope_vision with an identity row for the prefix tokens).                         */
int g2v_im2col_patch(const void* img, int N, int H, int W, int patch, void* out, int Kpad, void* stream);
int g2v_vit_assemble(const void* patch, const void* cls, const void* regs, void* x, int N, int P, int R, int C,
                     void* stream);

/* Qwen2VLImageProcessor._preprocess after the PIL resize (image_processing_qwen2_vl.py:218-273) on the device: uint8
 * frames [F,H,W,3] (H, W multiples of 28) -> rescale, normalise (host floats mean3 / std3), temporal pairing, patch
 * reorder -> bf16 [ceil(F/2) * H/14 * W/14, Kpad] (columns >= 1176 zero): the A operand of the patch-embed GEMM.
 * Bit-identical to the bf16 cast of the host transform's fp32 matrix.                                            */
int g2v_qwen_patchify_u8(const void* img_u8, int F, int H, int W, const float* mean3, const float* std3, void* out,
                         int Kpad, void* stream);

/* ---- small data movers ------------------------------------------------------------------------ */
int g2v_gather_rows_f32(const void* src, int ld_src, const void* idx, void* dst, int ld_dst,
                        int rows, int C, void* stream);      /* dst[i] = src[idx[i]]  (nn.Embedding) */
int g2v_scatter_rows_f32(const void* src, int ld_src, const void* idx, void* dst, int ld_dst,
                         int rows, int C, void* stream);     /* dst[idx[i]] = src[i]                 */
int g2v_cast_f32_bf16(const void* src, void* dst, int64_t n, void* stream);
int g2v_cast_bf16_f32(const void* src, void* dst, int64_t n, void* stream);

/* ---- pointmap / camera heads (g2vlm.py:1200-1226, transformer_head.py:69-81, camera_head.py) -- */
/* feat f32 [N*P, 3*patch^2] -> out f32 [N,H,W,3] via pixel_shuffle(patch); patch = the geometry encoder's patch size,
 * 14 (DINOv2, g2vlm.py:172) or 16 (use_dinov3, g2vlm.py:170); H, W multiples of it.  mode 0: raw (global points);
 * mode 1: local points (xy*exp(z), exp(z)) into `out` AND world points = pose[:3,:4] . (local,1)
 * into `out2` (pose f32 [N,4,4]).                                                                */
int g2v_pts_epilogue_ps(const void* feat, int N, int H, int W, int patch, int mode, const void* pose,
                        void* out, void* out2, void* stream);
/* the patch-14 form (kept for callers bound before the DINOv3 variant existed) */
int g2v_pts_epilogue(const void* feat, int N, int H, int W, int mode, const void* pose,
                     void* out, void* out2, void* stream);
/* F.pixel_shuffle(., patch) of a Pi3LinearPts3d output with C channels (transformer_head.py:69-81; the confidence head of
 * train_conf_pi3 checkpoints has C = 1, g2vlm.py:1208-1219): feat f32 [N*P, C*patch^2] -> out f32 [N, H, W, C]        */
int g2v_pixel_shuffle(const void* feat, int N, int H, int W, int C, int patch, void* out, void* stream);
int g2v_pixel_shuffle14(const void* feat, int N, int H, int W, int C, void* out, void* stream);   /* patch = 14 */

/* mean over P tokens of f32 [N,P,512] -> 2x(Linear+ReLU) -> fc_t, fc_rot -> SVD-orthogonalise ->
 * pose f32 [N,4,4].  Weights f32 in nn.Linear layout.                                            */
int g2v_camera_tail(const void* feat, int N, int P, const void* w0, const void* b0, const void* w1,
                    const void* b1, const void* wt, const void* bt, const void* wr, const void* br,
                    void* pose, void* stream);

/* torch.argmax over bf16 logits (g2vlm.py:1125), first maximal index -> int32 out[0].
 * scratch: int32[129] device words, zeroed ONCE by the caller (the kernel resets its arrival ticket).   */
int g2v_argmax_bf16(const void* x, int n, void* out, void* scratch, void* stream);


/* ---- batch-1 decode (g2vlm.py:1086-1135) ------------------------------------------------------- */
/* nn.Linear at M=1: y = bf16(W[N,K] . x[K] + bias); res != NULL: res[n] (f32) += y, else out[n] = y   */
int g2v_gemv_bf16(const void* x, const void* W, const void* bias, void* out, void* res, int N, int K, void* stream);
/* the same Linear with its producer fused in: (a) x = bf16(Qwen2RMSNorm(x_f32[K]; norm_w, eps)) -> out bf16[N];
 * (b) x = SwiGLU of the interleaved gate/up vector gu bf16[2K] -> res f32[N] += y (the MLP's down_proj + residual)  */
int g2v_gemv_rmsnorm_bf16(const void* x_f32, const void* norm_w, float eps, const void* W, const void* bias, void* out,
                          int N, int K, void* stream);
int g2v_gemv_swiglu_bf16(const void* gu, const void* W, void* res, int N, int K, void* stream);
/* (c) Qwen2MLP's first half in one launch (modeling_qwen2_vl.py:519-521 at q_len 1): x = bf16(Qwen2RMSNorm(x_f32[K])),
 * W_gu = gate/up interleaved per 16 rows [N2 = 2F, K] -> act_out bf16[F] = bf16(bf16(silu(g)) * u); the down projection
 * is then g2v_gemv_bf16(act_out, W_down, NULL, NULL, res)                                               */
int g2v_gemv_rmsnorm_swiglu_bf16(const void* x_f32, const void* norm_w, float eps, const void* W_gu, void* act_out,
                                 int N2, int K, void* stream);
/* Qwen2MLP activation on the fused gate/up GEMV output (interleaved per 16, as G2V_EPI_SWIGLU's W):
 * gu bf16[2n] -> out bf16[n] = bf16(bf16(silu(g)) * u)                                                */
int g2v_swiglu_bf16(const void* gu, void* out, int n, void* stream);
/* flash_attn_varlen_func with q_len 1 (qwen2vl.py:643-652): q bf16 [Hq,128]; caches bf16 [*,Hkv,128];
 * out bf16 [Hq,128]; workspace f32 of g2v_decode_attn_workspace(Lk,Hq) bytes                          */
int64_t g2v_decode_attn_workspace(int Lk, int Hq);
int g2v_decode_attn(const void* q, const void* k_cache, const void* v_cache, void* out, int Lk, int Hq,
                    int Hkv, float scale, void* workspace, void* stream);
/* hipGraph-replayable forms of the decode step: the KV length lives in device memory (int32 Lk_dev[1]) and the grid
 * is sized for max_len keys; g2v_decode_advance bumps {rope pos[3], cache row, kv length} by one on the device.   */
int g2v_decode_attn_dyn(const void* q, const void* k_cache, const void* v_cache, void* out, const void* Lk_dev,
                        int max_len, int Hq, int Hkv, float scale, void* workspace, void* stream);
int g2v_decode_advance(void* pos3, void* row, void* len, void* stream);

/* ---- batched decode (lifts the reference's batch = 1 limit, g2vlm.py:1006, 1137) -------------------
 * `batch` scenes share the weights; each has its own KV cache and length.  The Linears run as M = batch GEMMs through
 * g2v_gemm_bf16 (skinny kernel), norms / RoPE / cache write through the row-batched prefill entry points with cache rows
 * scene * scene_rows + len; only attention, argmax and the state bump need batch-aware forms:
 *   q / out bf16 [batch, Hq*128]; caches bf16 [batch, scene_rows, Hkv, 128]; Lk_dev int32[batch] (device);
 *   workspace >= batch * g2v_decode_attn_workspace(max_len, Hq) bytes; the grid covers max_len keys per scene.          */
int g2v_decode_attn_batch(const void* q, const void* k_cache, const void* v_cache, void* out, const void* Lk_dev,
                          int batch, int64_t scene_rows, int max_len, int Hq, int Hkv, float scale, void* workspace,
                          void* stream);
/* The decode step's attention with the q/k-norm, mRoPE and KV-cache append folded in (replaces g2v_qknorm_mrope_cache +
 * g2v_decode_attn_* for the one new token per scene; reference qwen2vl.py:596-652 at q_len 1):
 *   qkv bf16 [batch, (Hq + 2 Hkv) * 128] = the step's RAW fused projections; q_norm_w / k_norm_w f32 [128];
 *   cos / sin f32 [batch, 128] (g2v_mrope_table); Lk_dev[b] = cache length INCLUDING the new token - its K (normalised,
 *   rotated) and V are written to row Lk_dev[b] - 1 of scene b's block by this call; the rest as g2v_decode_attn_batch. */
int g2v_decode_attn_fused(const void* qkv, const void* q_norm_w, const void* k_norm_w, float eps, int und_rounding,
                          const void* cos, const void* sin, void* k_cache, void* v_cache, void* out, const void* Lk_dev,
                          int batch, int64_t scene_rows, int max_len, int Hq, int Hkv, float scale, void* workspace,
                          void* stream);
/* pos3 int32 [3, batch], row / len int32 [batch]: all += 1                                                             */
int g2v_decode_advance_batch(void* pos3, void* row, void* len, int batch, void* stream);
/* torch.argmax(logits, dim=-1) for bf16 [rows, ld >= n], first maximal index per row -> int32 out[rows];
 * scratch int32[rows * 129], zeroed once by the caller                                                                */
int g2v_argmax_rows_bf16(const void* x, int rows, int n, int64_t ld, void* out, void* scratch, void* stream);
/* torch.multinomial(softmax(logits / temperature, -1), 1) of generate_text's do_sample branch (g2vlm.py:1119-1122), per
 * row of bf16 [rows, ld >= n] -> int32 out[rows].  Drawn as argmax_i(logit_i / T - log(-log u_i)) (Gumbel-max: the same
 * distribution in one pass), u_i = Philox4x32-10(counter = {i, row, step, 0}, key = seed) top 24 bits.
 * rng: int32[4] on the device = {seed lo, seed hi, step, float bits of 1 / T}; this call advances `step` by one, so a
 * hipGraph-captured decode step draws fresh numbers at each replay.  torch's own CUDA Philox offsets are not
 * reproduced: parity with the reference is distributional.  scratch as g2v_argmax_rows_bf16.                          */
int g2v_sample_rows_bf16(const void* x, int rows, int n, int64_t ld, void* out, void* scratch, void* rng, void* stream);


/* ---- batch-1 decode, persistent-grid kernels (csrc/decode_layer.hip): every launch is 256 workgroups with an equal share
 * of the bytes each, which is what streams HBM at the full rate (one CU pulls ~1/256 of it) -------------------------- */
/* nn.Linear at M = 1 (g2vlm.py:1086-1125).  norm_w != NULL: x is the fp32 residual row and Qwen2RMSNorm(norm_w, eps) is
 * applied on the fly (K <= 1536), else x bf16[K] (K <= 9216).  act: W = gate/up interleaved per 16 rows [N = 2F, K], out
 * bf16[F] = bf16(bf16(silu(g)) * u) (norm_w required).  res != NULL: res[n] f32 += bf16(y[n] + bias[n]), else out[n] = it. */
int g2v_gemv_pg(const void* x, const void* norm_w, float eps, const void* W, const void* bias, void* out, void* res, int N,
                int K, int act, void* stream);
/* The same Linear for B = 1..8 decode rows at once (batched decode; the reference asserts B == 1,
 * g2vlm.py:1006 / 1137): Y[B, N] = X[B, K] . W[N, K]^T with the weights streamed ONCE.  Argument meaning as g2v_gemv_pg;
 * x / out / res are row-major [B, K] / [B, N (N/2 for act)] / [B, N].  K % 8 == 0, K <= 12288 (<= 1536 with norm_w).     */
int g2v_gemv_pg_batch(const void* x, const void* norm_w, float eps, const void* W, const void* bias,
                      void* out, void* res, int B, int N, int K, int act, void* stream);

/* ---- FP8 weight-only decode (csrc/decode_fp8.hip): the two entry points above with the weight matrix stored as OCP e4m3fn
 * codes and one power-of-two scale per output row, W[n][k] = e4m3(Wq[n][k]) * wscale[n] (g2vlm_amd/quant.py).  Wq uint8
 * [N, K], wscale f32 [N]; every other argument, fused form, rounding point and argument error as g2v_gemv_pg /
 * g2v_gemv_pg_batch.  The scale is applied exactly, so the result is that of the bf16 entry point on the dequantised
 * matrix up to the order of the fp32 partial sums.  K % 16 == 0; K <= 9216 / 12288 (<= 1536 with norm_w).               */
int g2v_gemv_pg_fp8(const void* x, const void* norm_w, float eps, const void* Wq, const void* wscale, const void* bias,
                    void* out, void* res, int N, int K, int act, void* stream);
int g2v_gemv_pg_batch_fp8(const void* x, const void* norm_w, float eps, const void* Wq, const void* wscale, const void* bias,
                          void* out, void* res, int B, int N, int K, int act, void* stream);

/* What the four entry points above launch for a shape, decided by the code they launch with (csrc/decode_dispatch.h);
 * touches no device.  B == 0: g2v_gemv_pg / g2v_gemv_pg_fp8, B = 1..8: the batched ones; norm: norm_w != NULL.
 * out = {form: 1 gemv_pg*, 2 gemv_pgb*, 3 gemv_pgk* kernels; threads per block; instantiated RB (form 3: R); KCH (form 3:
 * CW in bf16, S in e4m3)}.  G2V_ERR_ARG for every shape the entry point refuses.                                        */
int g2v_gemv_pg_route(int B, int N, int K, int act, int norm, int fp8, int32_t out[4]);

/* g2v_decode_attn_fused on a persistent grid (same arguments): 256 / Hkv blocks per kv head and scene, each an equal share
 * of the max_len cache rows (the share is fixed by the capacity so that no address depends on the device-side length), one
 * partial per (head, block).  Rows in [Lk_dev[b], max_len) may hold anything.  Hkv <= 128.
 * workspace >= g2v_decode_attn_pg_workspace(Hq, Hkv, batch) bytes.                                                       */
int64_t g2v_decode_attn_pg_workspace(int Hq, int Hkv, int batch);
int g2v_decode_attn_pg(const void* qkv, const void* q_norm_w, const void* k_norm_w, float eps, int und_rounding,
                       const void* cos, const void* sin, void* k_cache, void* v_cache, void* out, const void* Lk_dev,
                       int batch, int64_t scene_rows, int max_len, int Hq, int Hkv, float scale, void* workspace, void* stream);

/* ---- shared-prefix decode (csrc/decode_shared.hip): B questions about one scene ----------------------------------------
 * One step of g2v_decode_attn_pg for `batch` query slots whose caches share their first rows: slot z attends to the prefix
 * rows [0, prefix_len) of k_prefix / v_prefix [>= prefix_len, Hkv, 128] (read only, fetched once per column group of
 * floor(32 / G) slots rather than once per slot) followed by its own suffix rows [0, suffix_len_dev[z]) of
 * k_suffix / v_suffix [batch, suffix_rows, Hkv, 128].  suffix_len_dev (int32 [batch], on the device) INCLUDES the new token:
 * its normalised, rotated K row and its V row go to suffix row suffix_len_dev[z] - 1 of slot z, bit-identical to what
 * g2v_decode_attn_pg appends.  qkv [batch, (Hq + 2 Hkv) * 128] raw fused rows, cos / sin [batch, 128], out [batch, Hq * 128]:
 * as g2v_decode_attn_pg, whose result on the concatenated cache this is up to fp32 summation order.  Rows past prefix_len
 * or past a suffix length may hold anything.  batch 1..64, prefix_len >= 1, suffix_rows >= suffix_max_len >= every suffix
 * length; hipGraph-capturable.  workspace >= g2v_decode_attn_shared_workspace(...) bytes (0: invalid shape).            */
int64_t g2v_decode_attn_shared_workspace(int Hq, int Hkv, int batch, int prefix_len, int suffix_max_len);
int g2v_decode_attn_shared(const void* qkv, const void* q_norm_w, const void* k_norm_w, float eps, int und_rounding,
                           const void* cos, const void* sin, const void* k_prefix, const void* v_prefix, int prefix_len,
                           void* k_suffix, void* v_suffix, const void* suffix_len_dev, int batch, int64_t suffix_rows,
                           int suffix_max_len, int Hq, int Hkv, float scale, void* out, void* workspace, void* stream);

/* ---- FP8 KV cache of the decode step (csrc/decode_kv8.hip) ---------------------------------------------------------------
 * A cache row of one kv head is 128 OCP e4m3fn codes and one fp32 power-of-two scale, 2^ceil(log2(amax / 448)) (a zero row: 1),
 * K and V separately: the encoding of g2vlm_amd/quant.py applied to the rows viewed as [rows * Hkv, 128].  code * scale is
 * exactly a bf16 value.
 * g2v_kv_quant_e4m3:   src bf16 [rows, Hkv, 128] -> codes uint8 [rows, Hkv, 128], scales f32 [rows, Hkv].
 * g2v_kv_dequant_e4m3: the inverse, exact: out bf16 [rows, Hkv, 128] = codes * scales.
 * g2v_decode_attn_pg_kv8: g2v_decode_attn_pg with k_cache / v_cache as codes [batch, scene_rows, Hkv, 128] and k_scale /
 * v_scale f32 [batch, scene_rows, Hkv].  The new token's K row (normalised, rotated, rounded to bf16 as g2v_decode_attn_pg
 * rounds it) and V row are quantised, written to row Lk_dev[b] - 1 as codes + scale, and attended to as their dequantised
 * values; the result is g2v_decode_attn_pg's on the dequantised cache up to fp32 summation order.  Rows in
 * [Lk_dev[b], max_len) may hold any codes and any scales, NaN included.  Same workspace, same argument errors.            */
int g2v_kv_quant_e4m3(const void* src, int64_t rows, int Hkv, void* codes, void* scales, void* stream);
int g2v_kv_dequant_e4m3(const void* codes, const void* scales, int64_t rows, int Hkv, void* out, void* stream);
int g2v_decode_attn_pg_kv8(const void* qkv, const void* q_norm_w, const void* k_norm_w, float eps, int und_rounding,
                           const void* cos, const void* sin, void* k_cache, void* v_cache, void* k_scale, void* v_scale,
                           void* out, const void* Lk_dev, int batch, int64_t scene_rows, int max_len, int Hq, int Hkv,
                           float scale, void* workspace, void* stream);

/* ---- scoring (csrc/logprob.hip): log-probability of a given token per row of logits ------------------------------------------
 * log_softmax(x.float(), -1)[target] per row of bf16 x[rows, ld >= n]; targets int32 [rows] on the device.
 * out_lp   fp32 [rows]  : x[t] - max - log(sum exp(x - max)), fp32 arithmetic
 * out_lse  fp32 [rows]  or NULL : max + log(sum exp(x - max))
 * out_rank int32 [rows] or NULL : #{i : x[i] > x[t]} + #{i < t : x[i] == x[t]} (0: what g2v_argmax_rows_bf16 picks on a NaN-free row)
 * A target outside [0, n) gives out_lp = NaN and out_rank = -1; nothing is read out of range, and columns [n, ld) are never read.
 * -inf entries contribute 0, a -inf target gives -inf - also in a row whose n entries are all -inf, whose logsumexp is -inf
 * (torch gives NaN there); a difference x[t] - max beyond the fp32 range gives -inf.
 * One pass over the row, 16-byte loads where the row's base allows them.  A row's three results depend on its n elements and
 * its target only - not on rows, on its position, on the alignment of its base or on `scratch` - bit for bit.
 * scratch: NULL, or int32 words zeroed ONCE by the caller (the kernel resets its tickets), >= g2v_logprob_rows_workspace(rows, n)
 * bytes: with it, the rows of a launch too small to fill the chip are each dealt out to several workgroups; without it (or
 * with too little) every row is one workgroup's.  The workspace size is 0 where no split would be made.  hipGraph-capturable.
 * (The entry point was proposed as (x, rows, n, ld, targets, out_lp, out_lse, out_rank, stream); scratch, scratch_bytes and
 * g2v_logprob_rows_workspace are added to it because the library owns no device memory: the caller does, per scratch owner.) */
int64_t g2v_logprob_rows_workspace(int rows, int n);
int g2v_logprob_rows_bf16(const void* x, int rows, int n, int64_t ld, const void* targets, void* out_lp, void* out_lse,
                          void* out_rank, void* scratch, int64_t scratch_bytes, void* stream);

/* ---- top-k per row of logits (csrc/topk.hip): what the model preferred at a scored position ---------------------------------
 * The first k elements of every row of bf16 x[rows, ld >= n] in g2v_argmax_rows_bf16's total order: larger value first,
 * -0 == +0, every NaN above +inf, equal values by ascending index.  1 <= k <= G2V_TOPK_MAX.
 * out_idx int32 [rows, k]         : entry j is the index of the element with exactly j elements before it in that order, so
 *                                   out_idx[r][0] is what g2v_argmax_rows_bf16 gives for row r (NaN rows included) and, on a
 *                                   NaN-free row, out_idx[r][j] is the one target for which g2v_logprob_rows_bf16 reports rank j
 * out_val fp32 [rows, k] or NULL  : the selected elements' own values, converted exactly (a NaN's bits and a zero's sign kept)
 * Entries j >= n (k > n) are index -1 and value NaN.  Every index written is in [0, n) or -1; columns [n, ld) are never read.
 * One pass over the row, 16-byte loads where the row's base allows them.  The answer is exact and unique: a row's results
 * depend on its n elements and k only - not on rows, on its position, on the alignment of its base or on `scratch`.
 * scratch: as g2v_logprob_rows_bf16's - NULL, or int32 words zeroed ONCE by the caller (the kernel resets its tickets),
 * >= g2v_topk_rows_workspace(rows, n, k) bytes: with it, the rows of a launch too small to fill the chip are each dealt out to
 * several workgroups, which leave sorted k-lists there for the last of them to merge (no workgroup waits for another); without
 * it every row is one workgroup's.  The workspace size is 0 where no split would be made.  hipGraph-capturable.
 * -22 before any launch: rows <= 0, n <= 0, ld < n, k < 1, k > G2V_TOPK_MAX, x or out_idx NULL.                             */
#define G2V_TOPK_MAX 32
int64_t g2v_topk_rows_workspace(int rows, int n, int k);
int g2v_topk_rows_bf16(const void* x, int rows, int n, int64_t ld, int k, void* out_idx, void* out_val, void* scratch,
                       int64_t scratch_bytes, void* stream);

/* ---- point-cloud export (csrc/cloud.hip): what follows `recon` ------------------------------------------------------------
 * Inputs are recon's outputs for one batch entry: points / local fp32 [N,H,W,3], conf fp32 [N,H,W] (logits), colors fp32
 * [N,3,H,W] (the `images` layout).  Every entry point returns -22 before any launch on a NULL pointer its flags require, on
 * N, H or W <= 0, on N*H*W > 2^31 - 1 (and N or ceil(H/16) > 65535), on a pointer that is not 4-byte aligned, and on a workspace
 * that is missing or smaller than its query says.  Workspaces need no initialisation.  hipGraph-capturable.
 *
 * g2v_cloud_mask: mask u8 [N,H,W] = 1 where every test enabled in `flags` passes.
 *   G2V_CLOUD_FINITE     the three coordinates of `points` are finite
 *   G2V_CLOUD_CONF       conf > conf_logit_min, an fp32 compare (the caller turns a probability p into log(p / (1 - p)) in
 *                        fp64, rounded to fp32 once; no sigmoid is evaluated here); a NaN logit fails
 *   G2V_CLOUD_EDGE_ATOL, G2V_CLOUD_EDGE_RTOL   the pixel is dropped if it is an edge of d = local[..., 2] under the
 *                        reference's depth_edge (modeling/pi3/utils/geometry.py:339; 3x3 window, no mask): over the in-bounds
 *                        pixels of the window (never across a row, column or view boundary), a NaN among them means "not an edge";
 *                        else diff = max(window) + max(-window) in fp32; an edge if diff > atol (ATOL) or if q > rtol (RTOL)
 *                        for q = diff / d_centre, correctly rounded, NaN -> 0, +-inf -> +-FLT_MAX
 *   `points` may be NULL without FINITE, `conf` without CONF, `local` without either EDGE bit.
 *
 * g2v_cloud_compact: the kept pixels (mask != 0) as packed 15-byte PLY records (<f4 x, y, z; u1 r, g, b) in view-major,
 *   row-major order - numpy boolean indexing's - into records u8 [max_records, 15]; counts int32 [N] receives the kept pixels
 *   of every view (always their true number).  Records past max_records are not written (max_records = N*H*W always
 *   suffices; 0 with records NULL only counts).  The colour byte is (uint8)(min(max((double)c, 0), 1) * 255), truncated;
 *   colours are assumed finite.  Positions are integer prefix sums: the bytes are the same on every run.
 *
 * g2v_intrinsics_lsq: per view the least-squares pinhole fit u = fx X/Z + cx, v = fy Y/Z + cy over pixel centres
 *   u = x + 0.5, v = y + 0.5 and the pixels of `local` that mask keeps (NULL: all) with finite X, Y, Z and Z > 0.  Ratios and
 *   sums in fp64, reduced in a fixed order (no atomics): the same bits on every run.  K fp32 [N,3,3] = {fx 0 cx; 0 fy cy; 0 0 1},
 *   used int32 [N] = pixels fitted.  Fewer than 2 such pixels, or no variance of X/Z (Y/Z), gives NaN for fx, cx (fy, cy).  */
#define G2V_CLOUD_FINITE 1
#define G2V_CLOUD_CONF 2
#define G2V_CLOUD_EDGE_ATOL 4
#define G2V_CLOUD_EDGE_RTOL 8
int g2v_cloud_mask(const void* points, const void* local, const void* conf, int N, int H, int W, int flags, float conf_logit_min,
                   float edge_atol, float edge_rtol, void* mask, void* stream);
int64_t g2v_cloud_compact_workspace(int N, int H, int W);
int g2v_cloud_compact(const void* points, const void* colors, const void* mask, int N, int H, int W, void* records,
                      int64_t max_records, void* counts, void* workspace, int64_t workspace_bytes, void* stream);
int64_t g2v_intrinsics_lsq_workspace(int N, int H, int W);
int g2v_intrinsics_lsq(const void* local, const void* mask, int N, int H, int W, void* K, void* used, void* workspace,
                       int64_t workspace_bytes, void* stream);

/* ---- multi-view consistency of the cloud (csrc/consistency.hip): does any other view see this point? ------------------------
 * points / local fp32 [N,H,W,3] as above (of local only the depth local[..., 2] is read), mask u8 [N,H,W] or NULL (all pixels),
 * poses fp32 [N,4,4] camera-to-world (R = poses[j,:3,:3], t = poses[j,:3,3]), K fp32 [N,3,3] (fx = K[j,0,0], fy = K[j,1,1],
 * cx = K[j,0,2], cy = K[j,1,2]; g2v_intrinsics_lsq's), depth_rtol >= 0.
 *
 * The rule is exact: fp32 throughout, every operation rounded once, no fused multiply-add, every comparison an IEEE compare
 * (false on NaN).  For a source pixel (i, p) with world point P and every target view j != i:
 *   d = P - t;  q_k = (R[0][k] d0 + R[1][k] d1) + R[2][k] d2  (k = 0, 1, 2: R^T d, parenthesised as written);
 *   u = fx (q0 / q2) + cx,  v = fy (q1 / q2) + cy, the divisions correctly rounded;
 *   inside iff q2 > 0 && u >= 0 && u < W && v >= 0 && v < H; only then x = (int)u, y = (int)v (pixel centres are at + 0.5, so
 *   the pixel that contains u is floor(u): a nearest-neighbour lookup) and zt = local[j,y,x,2];
 *   valid iff inside, mask[j,y,x] != 0, zt finite and zt > 0;  tol = depth_rtol zt, diff = q2 - zt;
 *   AGREE iff valid and |diff| <= tol;  IN FRONT iff valid and diff < -tol (P floats between camera j and the surface j sees).
 *   A point behind the surface is merely occluded: neither.
 * A source pixel is eligible iff mask[i,p] != 0 and P is finite; a pixel that is not has both counts 0.
 *
 * Outputs, each optional (NULL) but not all four at once: agree / in_front u8 [N,H,W] = the number of target views in each
 * class; pairs int32 [N,N,2], pairs[i,j,0] / [i,j,1] = the pixels of view i that agree / lie in front in view j (diagonal 0;
 * integer atomics: the same on every run); mask_out u8 [N,H,W] = eligible && agree >= min_agree && (max_in_front < 0 ||
 * in_front <= max_in_front).  The workspace (4 N H W bytes, no initialisation needed) receives a depth plane: local z where
 * valid, NaN elsewhere.  -22 before any launch for the section's reasons above, for N > 256 (the counts are bytes), for
 * H > 524280 (8 rows per tile, 65535 tile rows per launch), for a depth_rtol that is negative or NaN, and when there is nothing
 * to write.  The query returns 0 for every shape that the entry point refuses.
 * hipGraph-capturable, no host synchronisation.  */
int64_t g2v_cloud_consistency_workspace(int N, int H, int W);
int g2v_cloud_consistency(const void* points, const void* local, const void* mask, const void* poses, const void* K,
                          int N, int H, int W, float depth_rtol, int min_agree, int max_in_front,
                          void* agree, void* in_front, void* pairs, void* mask_out,
                          void* workspace, int64_t workspace_bytes, void* stream);

/* ---- rendering the cloud from any camera with a z-buffer (csrc/render.hip) ----------------------------------------------------
 * points fp32 [N,H,W,3] (world), colors fp32 [N,3,H,W] (may be NULL only when color_out is NULL), mask u8 [N,H,W] or NULL (all
 * pixels): the SOURCE, as above.  poses fp32 [M,4,4] camera-to-world and K fp32 [M,3,3] of the M TARGET cameras (R, t, fx, fy,
 * cx, cy as in the consistency section), target images of OH x OW pixels.  skip int32 [M] or NULL: source view skip[m] takes no
 * part in target m; -1 or any value outside [0, N) leaves nobody out.  radius 0..8: the half-width of the square a point is
 * drawn as.  background: 0xRRGGBB.
 *
 * The rule is exact: fp32 throughout, every operation rounded once, no fused multiply-add, every comparison an IEEE compare
 * (false on NaN).  For target m and the source pixel with flat index p = (i H + y) W + x and world point P:
 *   eligible iff mask[p] != 0, the three coordinates of P are finite and i != skip[m];
 *   d = P - t;  q_k = (R[0][k] d0 + R[1][k] d1) + R[2][k] d2  (k = 0, 1, 2: R^T d, parenthesised as written);
 *   u = fx (q0 / q2) + cx,  v = fy (q1 / q2) + cy, the divisions correctly rounded;
 *   the point lands iff q2 > 0, q2 is finite, u >= 0 && u < OW and v >= 0 && v < OH; only then x0 = (int)u, y0 = (int)v (the
 *   centre must be inside the image), and the point covers the pixels [x0 - radius, x0 + radius] x [y0 - radius, y0 + radius]
 *   clipped to the image;
 *   its key is ((uint64)bits(q2) << 32) | (uint32)p.  A target pixel keeps the MINIMUM key over the points that cover it: for
 *   positive finite floats bit order is value order, so the nearest point wins and the lower source index among equal depths.
 *   Keys are distinct and the minimum is associative: the result does not depend on the order in which anything ran.
 * Resolve: a pixel that no point covers gets background, depth 0.0f and index -1; otherwise depth = the float in the key's high
 * word, index = its low word, and colour = the three bytes the PLY export writes for source pixel index:
 * (uint8)(clip((double)c, 0, 1) * 255) of colors[i, 0..2, y, x].
 *
 * Outputs, each optional (NULL) but not all three at once: color_out u8 [M,OH,OW,3], depth_out fp32 [M,OH,OW], index_out int32
 * [M,OH,OW].  The workspace (8 M OH OW bytes, 8-byte aligned, no initialisation needed) holds the keys; the entry point fills
 * it itself.  -22 before any launch for a dimension <= 0, N H W or M OH OW above 2^31 - 1, M > 65535, a radius outside [0, 8], a
 * background outside [0, 0xFFFFFF], a required pointer that is NULL, an fp32 / int32 pointer that is not 4-byte aligned, a
 * workspace that is too small or not 8-byte aligned, colors NULL with color_out given, and when there is nothing to write.
 * The query returns 0 for every target shape that the entry point refuses.
 * Three launches (fill, splat, resolve) on the stream; hipGraph-capturable, no host synchronisation.  */
int64_t g2v_cloud_render_workspace(int M, int OH, int OW);
int g2v_cloud_render(const void* points, const void* colors, const void* mask, int N, int H, int W,
                     const void* poses, const void* K, const void* skip, int M, int OH, int OW,
                     int radius, int background,
                     void* color_out, void* depth_out, void* index_out,
                     void* workspace, int64_t workspace_bytes, void* stream);

/* ---- voxel-grid downsampling of the cloud (csrc/voxel.hip) ------------------------------------------------------------------
 * One vertex per occupied cell of the grid origin + k * voxel_size: the mean of the cell's points and of their colour bytes.
 * points fp32 [N,H,W,3], colors fp32 [N,3,H,W], mask u8 [N,H,W].  A pixel takes part if mask != 0 and its three coordinates are
 * finite.  Per axis, in fp64 without contraction: t = ((double)p - o) / v, g = floor(t); the pixel is out of range (dropped and
 * counted) unless -2^20 <= g < 2^20; q = (int64)floor((t - g) * 2^24 + 0.5).  Per cell: n points, S = sum q, C = sum of the
 * colour bytes of g2v_cloud_compact; the vertex is (float)(o + ((double)g + (double)S / ((double)n * 2^24)) * v) and the colour
 * byte (2 C + n) / (2 n), which rounds half up.  Cells are numbered in the order of the flat pixel index (view-major, row-major)
 * of their first participating pixel.  Every sum is an integer sum: the same inputs give the same bytes on every run.
 * Every entry point returns -22 before any launch on a NULL required pointer, on N, H or W <= 0, on N*H*W >= 2^31, on a voxel
 * size that is not > 0 or not finite, on a non-finite origin, on M < 0 and on a workspace smaller than its query says (8-byte
 * aligned, no initialisation needed).  The queries return 0 for what the entry points refuse.  hipGraph-capturable.
 *
 * g2v_voxel_bounds: bounds[0..2] / [3..5] = the fp32 minimum / maximum per axis of the participating points, bounds[6] (int32)
 *   their number (0: the six floats are 0).
 * g2v_voxel_assign: voxel_of int32 [N,H,W] = the dense id of the pixel's cell, -1 for a pixel that is dropped; stats int32 [4] =
 *   {cells M, participating pixels, out-of-range pixels, status (non-zero: a probe ran out of slots; never with the table this
 *   sizes, which holds at least 2 N H W slots)}.
 * g2v_voxel_reduce: records u8 [M,15] (the PLY record of g2v_cloud_compact), counts int32 [M] = points per cell and, where the
 *   pointers are not NULL, out_points fp32 [M,3] and out_colors u8 [M,3]; voxel_of, voxel_size and origin as given to / made by
 *   g2v_voxel_assign, M = its stats[0] (ids >= M are ignored).  M == 0 is a valid no-op.  G2V_VOXEL_NO_RUNS (A/B only): every
 *   pixel issues its own atomics; without it the lanes of a wave that share a cell are summed first.  The result is the same.  */
#define G2V_VOXEL_NO_RUNS 1
int g2v_voxel_bounds(const void* points, const void* mask, int N, int H, int W, void* bounds, void* stream);
int64_t g2v_voxel_assign_workspace(int N, int H, int W);
int g2v_voxel_assign(const void* points, const void* mask, int N, int H, int W, double voxel_size, double origin_x,
                     double origin_y, double origin_z, void* voxel_of, void* stats, void* workspace, int64_t workspace_bytes,
                     void* stream);
int64_t g2v_voxel_reduce_workspace(int64_t M);
int g2v_voxel_reduce(const void* points, const void* colors, const void* voxel_of, int N, int H, int W, double voxel_size,
                     double origin_x, double origin_y, double origin_z, int64_t M, void* records, void* counts, void* out_points,
                     void* out_colors, void* workspace, int64_t workspace_bytes, int flags, void* stream);

/* ---- triangle-mesh export (csrc/mesh.hip): the pixel grid of every view triangulated -----------------------------------------
 * points fp32 [N,H,W,3], mask u8 [N,H,W] or NULL (all pixels), max_edge fp32, read only with G2V_MESH_MAX_EDGE in flags.
 *
 * The rule is exact: fp32 throughout, every operation rounded once, no fused multiply-add, every comparison an IEEE compare
 * (false on NaN).  The squared length of the edge between points A and B is d = A - B; e2 = (d0 d0 + d1 d1) + d2 d2.
 * In view i the quad (y, x), 0 <= y < H-1, 0 <= x < W-1, has the corners p00 = (y, x), p01 = (y, x+1), p10 = (y+1, x),
 * p11 = (y+1, x+1); with H < 2 or W < 2 there are no quads and the result is valid and empty.  Its candidate triangles, by how
 * many corners the mask keeps:
 *   4, and e2(p01, p10) < e2(p00, p11) (the anti diagonal is shorter):   (p00, p10, p01) then (p01, p10, p11);
 *   4 otherwise (ties and NaN included: the main diagonal):              (p00, p10, p11) then (p00, p11, p01);
 *   3: the one triangle of the kept corners - (p00, p10, p01), (p01, p10, p11), (p00, p10, p11) or (p00, p11, p01) when p11, p00,
 *      p01 or p10 is the missing one;  fewer: none.
 * All four orders face the camera: for an OpenCV camera (x right, y down, z forward) (B - A) x (C - A) points towards the camera
 * centre.  With G2V_MESH_MAX_EDGE a candidate survives iff e2 <= max_edge max_edge holds for each of its three edges, the product
 * formed once in fp32 (an edge with a NaN fails); without it every candidate survives, non-finite vertices included, as
 * non-finite points survive g2v_cloud_compact.
 * Faces are the surviving candidates in view-major, quad row-major order, within a quad in the order above.  Vertices are the
 * pixels that the mask keeps and that at least one face references (`used`), in flat pixel order (i H + y) W + x; a vertex's id is
 * its rank among the used pixels of all views, and faces hold vertex ids.  A vertex record is g2v_cloud_compact's 15-byte record:
 * call it with `used` as the mask.  A face record is 13 bytes: u1 3; <i4 a, b, c.
 *
 * Outputs, each optional (NULL) except counts: used u8 [N,H,W]; vertex_of int32 [N,H,W] = the id or -1; faces int32
 * [max_faces,3]; face_records u8 [max_faces,13]; counts int32 [N,2] = the vertices and faces of every view, always their true
 * numbers.  Faces past max_faces are not written (2 N (H-1) (W-1) always suffices; 0 only counts).  Positions are integer
 * prefix sums: the bytes are the same on every run.  The workspace needs no initialisation.
 * -22 before any launch for a dimension <= 0, N > 65535, N H W or 2 N (H-1) (W-1) above 2^31 - 1 (ids and face counts are int32),
 * points, counts or workspace NULL, an unknown flag, a max_edge that is negative or NaN with the flag set, max_faces < 0, an fp32 /
 * int32 pointer that is not 4-byte aligned and a workspace smaller than the query says; the query returns 0 for every shape that
 * the entry point refuses.  Up to five launches on the stream; hipGraph-capturable, no host synchronisation.  */
#define G2V_MESH_MAX_EDGE 1
int64_t g2v_cloud_mesh_workspace(int N, int H, int W);
int g2v_cloud_mesh(const void* points, const void* mask, int N, int H, int W, int flags, float max_edge, void* used,
                   void* vertex_of, void* faces, void* face_records, int64_t max_faces, void* counts, void* workspace,
                   int64_t workspace_bytes, void* stream);

/* ---- exact nearest neighbour between two clouds (csrc/nn.hip) ------------------------------------------------------------------
 * query fp32 [Nq,3], target fp32 [Nt,3], query_mask u8 [Nq] / target_mask u8 [Nt] or NULL (all points), max_distance fp32.
 *
 * The rule is exact: a point takes part if its mask byte is non-zero and its three coordinates are finite.  For a participating
 * pair, in fp32 with every operation rounded once and no fused multiply-add: d = q - t, d2 = (d0 d0 + d1 d1) + d2 d2 (never NaN;
 * +inf by overflow is possible).  m2 = max_distance max_distance, one fp32 product; a target counts unless d2 > m2 (equality
 * counts; max_distance = +inf, or any value whose square overflows, is no limit).  The answer of a query is the minimum over the
 * counting targets of the 64-bit key bits(d2) << 32 | target index: the nearest target, ties to the lowest index, and the lowest
 * participating index where every d2 is +inf.  index int32 [Nq] and sq_distance fp32 [Nq] hold the key's two halves; a query that
 * takes no part or has no counting target gets -1 and +inf.  stats int32 [4] = {participating queries, participating targets,
 * participating queries without a neighbour, participating queries with one}.  Nq == 0 and Nt == 0 are valid calls.
 * The minimum of integer keys does not depend on the order in which the targets are visited: the bytes of the three outputs are
 * the same on every run and on both paths.  G2V_NN_BRUTE / G2V_NN_GRID (A/B and tests only) force a path: every query against
 * every target through LDS tiles, or a uniform grid of cubic cells over the targets' bounding box (at most G^3 cells, G = the
 * largest G with G^3 <= 2 Nt, at most 256) walked ring by ring until no unvisited cell can hold a smaller key (DESIGN.md 6p has the argument).
 * Without a flag the brute path runs for every Nt: it was the faster one at every size measured.
 *
 * The workspace (16-byte aligned, no initialisation needed) is 256 + 24 Nt + 8 Nq + 4 (G^3 + 1) + 4 ceil(G^3 / 1024) bytes.
 * -22 before any launch for Nq or Nt < 0 or above 2^31 - 1, a max_distance that is negative or NaN, an unknown flag or both path
 * flags, stats or workspace NULL, query, index or sq_distance NULL with Nq > 0, target NULL with Nt > 0, an fp32 / int32 pointer
 * that is not 4-byte aligned, a workspace that is not 16-byte aligned or smaller than the query says; the query returns 0 for
 * counts that the entry point refuses.  Eleven launches on the grid path; on the brute path five plus one per 2^36 pairs (the
 * targets are cut so that no single kernel holds a device for long).  One stream; hipGraph-capturable, no host synchronisation.  */
#define G2V_NN_BRUTE 1
#define G2V_NN_GRID 2
int64_t g2v_cloud_nn_workspace(int64_t Nq, int64_t Nt);
int g2v_cloud_nn(const void* query, const void* query_mask, int64_t Nq, const void* target, const void* target_mask, int64_t Nt,
                 float max_distance, int flags, void* index, void* sq_distance, void* stats, void* workspace,
                 int64_t workspace_bytes, void* stream);

/* ---- per-pixel surface normals (csrc/normals.hip): image-space normals of every view's pixel grid ---------------------------
 * points fp32 [N,H,W,3], mask u8 [N,H,W] or NULL (all pixels), poses fp32 [N,4,4] camera-to-world or NULL (the camera of every
 * view is at the origin: camera-frame normals of local points), step 1..G2V_NORMALS_STEP_MAX = the distance to the neighbours,
 * max_edge fp32, read only with G2V_NORMALS_MAX_EDGE in flags.
 *
 * The rule is exact: fp32 throughout, every - * + rounded once, no fused multiply-add, sqrt and / correctly rounded, every
 * comparison an IEEE compare (false on NaN).  Pixel P = (y, x) of view i takes part iff mask != 0 (or mask is NULL) and its
 * three coordinates are finite.  Its neighbours are R = (y, x+step), D = (y+step, x), L = (y, x-step), U = (y-step, x).  A
 * neighbour Q is available iff it lies inside the same view, takes part and, with G2V_NORMALS_MAX_EDGE, its edge e = Q - P has
 * (e0 e0 + e1 e1) + e2 e2 <= max_edge max_edge (the product formed once in fp32; equality is kept, an edge with a NaN fails).
 * For the pairs (a, b) = (R,D), (D,L), (L,U), (U,R), in this order, of which both edges are available:
 *   c0 = a1 b2 - a2 b1,  c1 = a2 b0 - a0 b2,  c2 = a0 b1 - a1 b0   (each product rounded, then the difference);
 * m = the sum of the present c in that order, starting from the first present one (not from +0);
 * s2 = (m0 m0 + m1 m1) + m2 m2.  The pixel is VALID iff it takes part, at least one pair is present, s2 is finite and s2 > 0.
 * If valid:  n = m / sqrt(s2) (three divisions);  d = P - C with C = (pose[3], pose[7], pose[11]) of view i, or 0 without poses;
 *   t = (n0 d0 + n1 d1) + n2 d2;  if t > 0 the sign bit of all three components of n is flipped (the normal looks at the camera;
 *   -0.0 can occur);  dd = (d0 d0 + d1 d1) + d2 d2;  q = |t| / sqrt(dd), a NaN q replaced by 0;  cos_view = min(q, 1);
 *   colour k = n_k * 0.5f + 0.5f (two roundings).
 * If not valid every output is +0.0 / 0.
 *
 * Outputs, each optional (NULL) but not all four at once: normals fp32 [N,H,W,3], valid u8 [N,H,W], cos_view fp32 [N,H,W],
 * colors_out fp32 [N,3,H,W] (the layout of `colors` / images).  The result depends on nothing but the inputs: no atomics, the
 * same bytes on every run.  G2V_NORMALS_PLAIN / G2V_NORMALS_HALO (A/B and tests only) force a form of the kernel: the neighbours
 * by plain global loads, or - step 1 only - from a tile with a one-pixel halo staged in LDS.  The bytes are the same; without a
 * flag the plain form runs.
 * -22 before any launch for a dimension <= 0, N H W above 2^31 - 1, N > 65535, a step outside [1, G2V_NORMALS_STEP_MAX], an unknown
 * flag, both form flags, G2V_NORMALS_HALO with step != 1, a max_edge that is negative or NaN with the flag set, points NULL, all
 * four outputs NULL and an fp32 pointer that is not 4-byte aligned.  One launch, no workspace; hipGraph-capturable.
 *
 * g2v_cloud_compact_normals is g2v_cloud_compact for 27-byte records <f4 x, y, z; <f4 nx, ny, nz; u1 r, g, b (the property order
 * that Open3D and MeshLab write): the pixels with mask != 0 in view-major, row-major order, the normal copied bit for bit from
 * normals fp32 [N,H,W,3], the colour bytes those of g2v_cloud_compact; counts int32 [N] = the kept pixels of every view, always
 * their true numbers; records past max_records are not written (0, with records NULL, only counts).  The workspace
 * (8 N ceil(H W / 1024) bytes, no initialisation needed) and the -22 cases are g2v_cloud_compact's, plus normals NULL; the query
 * returns 0 for every shape that the entry point refuses.  Three launches; hipGraph-capturable.  */
#define G2V_NORMALS_MAX_EDGE 1
#define G2V_NORMALS_PLAIN 2
#define G2V_NORMALS_HALO 4
#define G2V_NORMALS_STEP_MAX 8
int g2v_cloud_normals(const void* points, const void* mask, const void* poses, int N, int H, int W, int step, int flags,
                      float max_edge, void* normals, void* valid, void* cos_view, void* colors_out, void* stream);
int64_t g2v_cloud_compact_normals_workspace(int N, int H, int W);
int g2v_cloud_compact_normals(const void* points, const void* normals, const void* colors, const void* mask, int N, int H, int W,
                              void* records, int64_t max_records, void* counts, void* workspace, int64_t workspace_bytes,
                              void* stream);
#ifdef __cplusplus
}
#endif
#endif
