/* painter_hip.h -- C ABI of libpainter_hip.so: the MI355X (gfx950) kernels behind the Painter / SegGPT
 * ViT forward/backward hot path.
 *
 * The reference (baaivision/Painter) has no FFI of its own: its hot path is a chain of ATen ops issued from
 * Python.  Each entry point below is the fused replacement for one group of those ops;
 * the comment on each cites the reference lines it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - plain pointers + sizes, no torch types; every pointer is a DEVICE pointer unless noted.
 *   - `dtype` selects the operand/activation storage type T: PA_F32 (exact fp32 MFMA, parity build) or
 *     PA_BF16 (bf16 operands, fp32 accumulate).  Parameters, the residual stream, statistics, losses and all
 *     parameter gradients are fp32 in both builds.  "T*" in a comment means float* or bf16* per `dtype`.
 *   - every function only ENQUEUES work on `stream` (no allocation, no synchronisation) and returns a
 *     hipError_t as int (0 = success).  Buffers are borrowed for the duration of the enqueued work.
 *   - `ld*` arguments are row strides in ELEMENTS.  16-byte alignment of all base pointers is required.
 *   - *_workspace_bytes() are host-only helpers giving the scratch size the matching call needs.
 */
#ifndef PAINTER_HIP_H
#define PAINTER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

enum { PA_F32 = 0, PA_BF16 = 1 };
enum {
    PA_EPI_BIAS = 0,       /* out(T)   = x.W^T + b                                   */
    PA_EPI_BIAS_F32 = 1,   /* out(f32) = x.W^T + b                                   */
    PA_EPI_BIAS_GELU = 2,  /* out2(T) = x.W^T + b (pre-activation, may be NULL); out(T) = gelu_erf(out2) */
    PA_EPI_BIAS_RESID = 3  /* out(f32) = resid + rowscale[row / rows_per_sample] * (x.W^T + b) */
};

/* Bumped whenever an entry point's argument list changes (2: `tables` in pa_attn_fwd / pa_attn_bwd; 3: `head_dim` in the attention and
 * rel-pos entry points; 4: `dxT_colsum` in pa_layernorm_bwd, `relpos_part` in pa_attn_bwd, `dx_colsum` in pa_linear_dgrad; 5: the bf16 GELU side output is gelu'(pre), pa_debug_set(9) is a test knob of the conv3x3 weight gradient, pa_attn4_trace is gone, pa_attn_bwd takes `out` / `ldo`, pa_debug_get / pa_attn_launch_counts are new; 6: the bf16 GELU side output is an 8-bit code (uint8, row pitch ldo bytes), pa_debug_set knobs 10 .. 15; 7: the *_skip entry points (DropPath skipping) and pa_debug_set knob 16 -- every earlier entry point keeps its argument list; 8: the pa_painter_* / pa_palette_argmin entry points of Painter task inference -- every earlier entry point keeps its argument list; 9: `steps` of pa_adamw_step is one count per table record (float[ntensors]) instead of one per group, its `beta1` / `beta2` are doubles, and PaOptGroups loses `active`; still 9 with the pa_pq_* and pa_ap_* entry points: they are purely additive, every earlier entry point keeps its argument list and its meaning).  painter_amd/_lib.py refuses a library whose pa_abi_version() differs from the header it parsed. */
#define PA_ABI_VERSION 9
int pa_abi_version(void);
/* diagnostics only (tools/): which = 0 start-up stagger of alternate workgroup rows of the 256x256 GEMM in shader cycles,
 * 1 drop that kernel's epilogue stores (never set by the product path); 2 = tile order of that kernel: 0 blocked 4 x 8 patches per XCD and, for
 * split-K launches, one contiguous (split, tile) run per XCD (default), 1 plain row-major, 2 blocked with split = blockIdx.y (before round 5); 3 = TUNING, set by the engine: target number of workgroups
 * of the weight-gradient GEMM (0 = 256, the whole chip; 64 when the weight gradients run on a side stream); 4 = row-tile height of the un-split bf16
 * GEMMs: 0 by rule (224 rows where that fills the last round of workgroups better), 1 always 256, 2 224 wherever possible; 5 = (G256_ILV_AB experiment
 * builds only) 1 + the DMA-placement schedule of that kernel; 6 = K splits of the
 * rel-pos table-gradient GEMM; 7 = rel-pos table gradient inside the generation-3 dQ kernel: 0 default (on), 1 off, 2 on (tests);
 * 8 = generation-3 attention: workgroups with idle waves dispatched last: 0 default (off since round 5), 1 off, 2 on;
 * 9 = tests: cap on the workgroups of the conv3x3 weight-gradient kernel (0 = 512), so that small images make a workgroup walk many tiles;
 * 10 = LayerNorm backward: 0 rows split over the workgroup's waves wherever D >= 1024 (default), 1 one wave per row everywhere (the kernel of
 * rounds 1 - 4) -- index 5 until round 5, where it collided with the ILV override; 11 .. 15 = round-6 experiment knobs (csrc/common.h);
 * 16 = DropPath skipping in the *_skip entry points: 0 default (on unless the environment has PAINTER_AMD_DROP_SKIP=0), 1 off (the factor vector
 * is ignored: exactly the launches of the entry points without _skip), 2 on. */
int pa_debug_set(int which, int value);
int pa_debug_get(int which);      /* the value last set (-1: no such knob) -- callers that change a knob temporarily restore what they found */

/* ---- nn.Linear: y = x W^T + b.  models_painter.py:76 (qkv), :87 (proj), timm Mlp fc1/fc2 (:201,:230) ----
 * PA_EPI_BIAS_GELU: out = gelu(pre), pre = x W^T + b rounded to T; out2 (optional) receives what the backward needs of pre, to be handed
 * to pa_linear_dgrad as `gelu_aux`:
 *   PA_F32 : pre itself, f32 [M,N] ld = ldo (erf-GELU' is evaluated on it there, to fp32 accuracy);
 *   PA_BF16: the DERIVATIVE gelu'(pre) = Phi(pre) + pre phi(pre) (ABI 5: the forward epilogue has both factors in registers, and the fc2 data
 *            gradient's epilogue becomes one load and one multiply) -- since ABI 6 as an 8-BIT CODE, uint8 [M,N] with a row pitch of ldo BYTES:
 *            q = round((g' + 0.13) * 255 / 1.26), g' = q * 1.26 / 255 - 0.13 (g' lies in [-0.129, 1.129]; absolute error <= 2.5e-3).  Half the
 *            bytes of the bf16 form on the fc1 write and on the fc2 data-gradient read; parity measured unchanged. */
int pa_linear_fwd(int dtype, int epilogue, const void* x /*T [M,K]*/, int64_t ldx, const void* w /*T [N,K]*/,
                  const float* bias /*[N]*/, void* out, void* out2, int64_t ldo, const float* resid /*f32 [M,N] ld=ldo*/,
                  const float* rowscale /*[M/rows_per_sample] or NULL*/, int rows_per_sample, int M, int N, int K,
                  hipStream_t stream);
/* DropPath skipping (ABI 7).  The *_skip entry points take the DropPath factor vector of the residual branch the call belongs to: rowskip f32
 * [samples], one factor per `skip_rows_per_sample` contiguous rows (attention: one per sample of the batch).  A sample whose factor is exactly 0
 * contributes nothing to anything that leaves the step (forward: its branch output is multiplied by 0; backward: its incoming gradient IS 0),
 * so its work is not done, and everything it would have written is written with defined values instead:
 *   pa_linear_fwd_skip / pa_linear_dgrad_skip (bf16 256 x 256 kernel only): a row tile whose rows all belong to dropped samples runs its epilogue on
 *       a zero accumulator -- bias; gelu(bias) and its GELU' code; resid; zero rows and a zero column-sum partial.  A tile that touches a kept
 *       sample runs in full, so rows of a dropped sample near its borders may hold the ordinary result.
 *   pa_attn_fwd_skip / pa_attn_bwd_skip (28-token-wide bf16 kernels only): zeros in the sample's out rows, lse entries and table tiles; zero
 *       dq / dk / dv rows, a zero rel-pos partial (or dG rows) and Delta field.
 * Kernels that do not implement it (exact-fp32 build, other grids) ignore the vector: each call's skip is valid on its own.  rowskip = NULL, or
 * knob 16 = off: the same launches as the entry point without _skip.  Results agree with the unskipped computation as numbers wherever the
 * skipped branch is finite (the sign of an exact zero may differ; a dropped branch that overflowed no longer poisons its sample through 0 * inf). */
int pa_linear_fwd_skip(int dtype, int epilogue, const void* x, int64_t ldx, const void* w, const float* bias, void* out, void* out2,
                       int64_t ldo, const float* resid, const float* rowscale, int rows_per_sample, int M, int N, int K,
                       const float* rowskip, int skip_rows_per_sample, hipStream_t stream);
/* decoder_embed + pixel shuffle 'nhwpqc->nchpwq' (models_painter.py:423-428); output is NHWC [B, Hp*P, Wp*P, C] T */
int pa_linear_pixshuf(int dtype, const void* x, int64_t ldx, const void* w /*T [P*P*C, K]*/, const float* bias,
                      void* out_nhwc, int batch, int Hp, int Wp, int P, int C, int K, hipStream_t stream);
/* autograd of the above: dX = dY.W (optionally * gelu'(pre), from the `out2` of pa_linear_fwd(PA_EPI_BIAS_GELU) of the same dtype), dW = dY^T.X (fp32), db = colsum(dY).
 * dx_colsum (optional, f32 [K], with workspace = pa_linear_dgrad_workspace_bytes(M, K)): the column sums of dX (fp32, in front of its rounding to T on the bf16 fast path) -- dX is the dY
 * of the layer in front (fc1 behind the GELU), so this is that layer's bias gradient, taken in the GEMM's epilogue instead of a second
 * pass over dX. */
int64_t pa_linear_dgrad_workspace_bytes(int M, int K);
int pa_linear_dgrad(int dtype, const void* dy /*T [M,N]*/, int64_t lddy, const void* w /*T [N,K]*/,
                    const void* gelu_aux /*NULL, or what pa_linear_fwd(PA_EPI_BIAS_GELU) put into out2: f32 [M,K] ld=lddx | uint8 [M,K] pitch lddx bytes*/, void* dx /*T [M,K]*/, int64_t lddx, float* dx_colsum,
                    void* workspace, int M, int N, int K, hipStream_t stream);
int pa_linear_dgrad_skip(int dtype, const void* dy, int64_t lddy, const void* w, const void* gelu_aux, void* dx, int64_t lddx, float* dx_colsum,
                         void* workspace, int M, int N, int K, const float* rowskip /* of the rows of dy / dx */, int skip_rows_per_sample,
                         hipStream_t stream);
/* pa_linear_wgrad_workspace_bytes: enough for every route pa_linear_wgrad can take at this shape (the maximum over the 256 x 256 kernel's and
 * the generic engine's split-K slabs: the route also depends on the leading dimensions).  lddy and ldx are multiples of 4 elements. */
int64_t pa_linear_wgrad_workspace_bytes(int dtype, int M, int N, int K);
int pa_linear_wgrad(int dtype, const void* dy /*T [M,N]*/, int64_t lddy, const void* x /*T [M,K]*/, int64_t ldx,
                    float* dw /*f32 [N,K]*/, void* workspace, int M, int N, int K, hipStream_t stream);
int64_t pa_colsum_workspace_bytes(int M, int N);
int pa_colsum(int dtype, const void* x /*T [M,N]*/, int64_t ld, int M, int N, float* out /*[N]*/, void* workspace,
              hipStream_t stream);
int pa_slab_reduce(const float* in, float* out, int64_t n, int nz, int64_t stride, int accumulate, hipStream_t stream);

/* ---- nn.LayerNorm(eps=1e-6) over channels: models_painter.py:218,230 (norm1/2), :416-417 (shared tap norm) ---- */
int pa_layernorm_fwd(int dtype, const float* x, int64_t ldx, const float* gamma, const float* beta, float eps,
                     void* y /*T, may be a column slice of the tap concat buffer*/, int64_t ldy, float* mean, float* rstd,
                     int R, int D, hipStream_t stream);
int64_t pa_layernorm_bwd_workspace_bytes(int R, int D);
/* dx = (dres ? dres : 0) + LN'(dy); dres may alias dx.  dxT (optional, T) = rowscale[row/rows_per_sample] * dx.
 * dgamma_dbeta: f32 [2, D], overwritten.  dxT_colsum (optional, f32 [D], needs dxT): the column sums of rowscale * dx (the fp32 values
 * dxT is rounded from) -- dxT is the dY of the nn.Linear in front of this norm's residual branch, so this is that layer's bias gradient, fused here. */
int pa_layernorm_bwd(int dtype, const void* dy, int64_t lddy, const float* x, int64_t ldx, const float* mean,
                     const float* rstd, const float* gamma, const float* dres, float* dx, int64_t lddx, void* dxT,
                     int64_t lddxT, const float* rowscale, int rows_per_sample, float* dgamma_dbeta, float* dxT_colsum,
                     void* workspace, int R, int D, hipStream_t stream);
/* Deferred form: pa_layernorm_bwd with dgamma_dbeta = NULL leaves the per-workgroup partial rows in `workspace` (dxT_colsum non-NULL there
 * = "with column sums"; nothing is written through it); pa_layernorm_bwd_reduce finishes them -- nothing downstream in the backward reads
 * these parameter gradients, so the engine runs the reduction on its side stream. */
int pa_layernorm_bwd_reduce(const void* workspace, float* dgamma_dbeta, float* dxT_colsum, int with_colsum, int R, int D,
                            hipStream_t stream);

/* ---- Attention with decomposed rel-pos bias: models_painter.py:76-86 + util/vitdet_utils.py:63-125 ---- */
int pa_relpos_rows_padded(int Hp, int Wp);
/* head_dim (hd) = embed_dim / heads: 64 (every reference factory; all kernel generations) or 80 (ViT-H/14, BASELINE configs[4]: the
 * generic kernels of csrc/attn_fwd.hip / attn_bwd.hip, both dtypes); anything else is rejected.
 * rcat: T [pa_relpos_rows_padded, hd] = [rel_pos_h ; rel_pos_w ; 0] */
int pa_relpos_pack(int dtype, const float* rel_pos_h, const float* rel_pos_w, void* rcat, int Hp, int Wp, int head_dim,
                   hipStream_t stream);
/* Every block's Rcat and Rcat^T (pa_relpos_pack_t below) in ONE launch: tabs = device array of 2 * nblocks `const float*` -- rel_pos_h of
 * every block, then rel_pos_w of every block (util/vitdet_utils.py:63-125 reads these per block); rcat: T [nblocks, NRP, hd]; rcatT: T
 * [nblocks, hd, NRP].  Values identical to the per-block entry points; what a training step calls after the optimizer has written the tables. */
int pa_relpos_pack_batch(int dtype, const void* tabs, void* rcat, void* rcatT, int nblocks, int Hp, int Wp, int head_dim, hipStream_t stream);
/* qkv: T [batch*L, 3*heads*hd] as produced by the qkv Linear; out: T [batch*L, heads*hd]; lse: f32 [batch*heads, L].
 * tables: NULL (inference), or pa_attn_tables_bytes() of device memory that receives the per-query bias tables the
 * backward reuses (only the 28-token-wide bf16 kernels write it; the size is 0 for every other case). */
int64_t pa_attn_tables_bytes(int dtype, int batch, int L, int heads, int Hp, int Wp, int head_dim);
/* 0 = default kernels for the grid (generation 3 where it applies), 3 = the same explicitly, 2 = never use the 28-token-wide
 * generation-3 kernels (diagnostics, A/B, cross-generation tests) */
int pa_attn_set_generation(int generation);
/* diagnostics / tests: host-side launch counts since process start, out6 = {pa_attn_fwd on the generic kernels (csrc/attn_fwd.hip),
 * on generation 2 (attn2.hip: every head_dim-80 grid with key rows of 12..32 tokens), on generation 3 (attn3.hip), pa_attn_bwd likewise} */
int pa_attn_launch_counts(long long* out6);
/* diagnostics: enable != 0 runs the generation-3 dQ kernel with s_memtime stamps (two workgroups, waves 0 / 1, 64 tiles, 8 slots);
 * host_out (may be NULL) receives the 2 x 2 x 64 x 8 stamps of the last traced launch */
int pa_attn_trace(int enable, unsigned long long* host_out);
int pa_attn_fwd(int dtype, const void* qkv, int64_t ldq, const void* rcat, void* out, int64_t ldo, float* lse,
                void* tables, int batch, int L, int heads, int Hp, int Wp, int head_dim, float scale, hipStream_t stream);
int pa_attn_fwd_skip(int dtype, const void* qkv, int64_t ldq, const void* rcat, void* out, int64_t ldo, float* lse,
                     void* tables, int batch, int L, int heads, int Hp, int Wp, int head_dim, float scale, const float* rowskip /*[batch] or NULL*/,
                     hipStream_t stream);

/* autograd of pa_attn_fwd (no reference source: torch autograd of the lines above).
 *   delta  : f32 [batch*heads, L] = rowsum(dO o O)                      (pa_attn_bwd_delta)
 *   dqkv   : T, same layout as qkv (dq | dk | dv) -- the same leading dimension ldq too: a buffer of batch*L rows at that pitch
 *   dG     : T [batch*L, heads*NRP] r-space bias gradient, consumed by pa_attn_bwd_relpos (NULL when relpos_part is given)
 *   relpos_part : NULL, or pa_attn_bwd_relpos_partials_bytes() (> 0 only where the 28-token-wide bf16 kernels run and `tables` is
 *            given) of device scratch: the dQ kernel then contracts d rel_pos itself -- one fp32 [NRP, hd] partial per workgroup --
 *            dG is not written, and pa_attn_bwd_relpos_reduce() sums the partials into drcat in a fixed order (deterministic)
 *   aux    : scratch of pa_attn_bwd_aux_bytes()
 *   tables : what pa_attn_fwd wrote (NULL: the backward recomputes the bias tables itself, generation-2 kernels); since ABI 5 the forward
 *            also writes the log-sum-exp fields of the tiles, the backward adds the Delta field.
 *            CONTRACT: the tiles must come from pa_attn_fwd of THIS library version (ABI >= 5) on the SAME qkv / rcat / scale -- the dKV kernel
 *            contracts the bf16 bias entries and the -lse / scale hi + lo fields it finds there and nothing checks their origin; tiles
 *            built or copied another way (the ABI-4 contract: a prep launch filled every field) give silently wrong dK / dV.  Callers
 *            that cannot guarantee it pass tables = NULL (generation 2 recomputes everything) or run pa_attn_bwd_prep, which rewrites the
 *            lse and Delta fields from `lse` / `out` / `dout` (the bias entries still have to be the forward's).
 *   out / ldo : the forward's output O (T [batch*L, heads*hd]) or NULL.  Given with delta = NULL where pa_attn_bwd_prep_ok(): the dQ kernel
 *            computes Delta = rowsum(dO o O) itself -- no pa_attn_bwd_delta / pa_attn_bwd_prep launch at all (ABI 5; the engine's route)
 *   rcatT  : T [hd, NRP] from pa_relpos_pack_t
 *   drcat  : f32 [NRP, hd] = [d rel_pos_h ; d rel_pos_w ; 0], overwritten */
int pa_relpos_pack_t(int dtype, const float* rel_pos_h, const float* rel_pos_w, void* rcatT, int Hp, int Wp, int head_dim,
                     hipStream_t stream);
int pa_attn_bwd_delta(int dtype, const void* out, int64_t ldo, const void* dout, int64_t lddo, float* delta, int batch,
                      int L, int heads, int head_dim, hipStream_t stream);
/* pa_attn_bwd_prep_ok() == 1 (28-token-wide bf16 kernels, `tables` given): Delta can live in the table tiles.  Either pa_attn_bwd is given
 * `out` and delta = NULL (the dQ kernel computes Delta: no extra launch), or -- the round-4 route, kept for A/B and tests -- pa_attn_bwd_prep
 * computes Delta and writes it with the log-sum-exp fields into the tiles in one pass and pa_attn_bwd is called with delta = out = NULL. */
int pa_attn_bwd_prep_ok(int dtype, int L, int Hp, int Wp, int head_dim);
int pa_attn_bwd_prep(int dtype, const void* out, int64_t ldo, const void* dout, int64_t lddo, const float* lse, void* tables,
                     int batch, int L, int heads, int Hp, int Wp, int head_dim, float scale, hipStream_t stream);
int64_t pa_attn_bwd_aux_bytes(int batch, int L, int heads, int Hp, int Wp);
int64_t pa_attn_bwd_relpos_partials_bytes(int dtype, int batch, int L, int heads, int Hp, int Wp, int head_dim);
int pa_attn_bwd(int dtype, const void* qkv, int64_t ldq, const void* rcat, const void* rcatT, const void* dout,
                int64_t lddo, const float* lse, const float* delta, void* dqkv, void* dG, void* relpos_part, void* aux,
                void* tables, const void* out, int64_t ldo, int batch, int L, int heads, int Hp, int Wp, int head_dim, float scale,
                hipStream_t stream);
int pa_attn_bwd_skip(int dtype, const void* qkv, int64_t ldq, const void* rcat, const void* rcatT, const void* dout,
                     int64_t lddo, const float* lse, const float* delta, void* dqkv, void* dG, void* relpos_part, void* aux,
                     void* tables, const void* out, int64_t ldo, int batch, int L, int heads, int Hp, int Wp, int head_dim, float scale,
                     const float* rowskip /*[batch] or NULL*/, hipStream_t stream);
int64_t pa_attn_bwd_relpos_workspace_bytes(int dtype, int batch, int L, int heads, int Hp, int Wp, int head_dim);
int pa_attn_bwd_relpos_reduce(const void* relpos_part, float* drcat, void* workspace, int batch, int L, int heads, int Hp, int Wp,
                              int head_dim, hipStream_t stream);
int pa_attn_bwd_relpos(int dtype, const void* dG, const void* qkv, int64_t ldq, float* drcat, void* workspace,
                       int batch, int L, int heads, int Hp, int Wp, int head_dim, hipStream_t stream);

/* ---- PatchEmbed (Conv2d k=P s=P as an im2col GEMM) + token assembly: util/vitdet_utils.py:182-186,
 *      models_painter.py:387-409 (mask token, segment tokens, abs pos), models_seggpt.py:415-420 (type tokens) ----
 * imgs/tgts: f32 NCHW [B,3,Hp*P,Wp*P]; w: T [D, ldw], ldw >= Kp = 3*P*P rounded up to 8, columns >= 3*P*P zero (pa_patch_weight_pack
 * makes it from the conv weight; for P % 8 == 0 it is the plain T copy with ldw = 3*P*P); any P >= 1 (P = 14: ViT-H/14);
 * pos: f32 [L, D] from pa_pos_fwd; mask: bool bytes [B or 1, L];
 * type_cls/type_ins/seg_type: SegGPT only (NULL otherwise), seg_type f32 [B];
 * tokens: f32 [2*B*L, D] = cat(x stream, y stream) on the batch axis (models_painter.py:409). */
int pa_patch_weight_pack(int dtype, const float* w /*f32 [D, 3*P*P]*/, void* out /*T [D, Kp]*/, int D, int P, hipStream_t stream);
int pa_patch_embed_fwd(int dtype, const float* imgs, const float* tgts, const void* w, int64_t ldw, const float* bias,
                       const float* mask_token, const float* seg_x, const float* seg_y, const float* pos,
                       const unsigned char* mask, int mask_batch_stride, const float* type_cls, const float* type_ins,
                       const float* seg_type, float* tokens, int batch, int Hp, int Wp, int P, int D, hipStream_t stream);
/* bf16 fast path (P % 8 == 0 and 3*P*P % 128 == 0, i.e. every reference factory): materialise the im2col operand once
 * (cols: bf16 [2*B*L, 3*P*P], also the X operand of the weight gradient: pa_linear_wgrad(dpe, cols)) and run the contraction on the
 * 256x256 LDS-DMA kernel.  pa_patch_cols_ok() says whether the shape qualifies; pa_patch_embed_fwd / _wgrad serve every other case. */
int pa_patch_cols_ok(int batch, int L, int P, int D);
int pa_patch_im2col(const float* imgs, const float* tgts, void* cols, int batch, int Hp, int Wp, int P, hipStream_t stream);
int pa_patch_embed_fwd_cols(const void* cols, const void* w /*bf16 [D, ldw]*/, int64_t ldw, const float* bias, const float* mask_token,
                            const float* seg_x, const float* seg_y, const float* pos, const unsigned char* mask, int mask_batch_stride,
                            const float* type_cls, const float* type_ins, const float* seg_type, float* tokens, int batch, int L, int K,
                            int D, hipStream_t stream);
int64_t pa_patch_embed_wgrad_workspace_bytes(int D, int P);
int pa_patch_embed_wgrad(int dtype, const void* dpe /*T [2BL, D]*/, const float* imgs, const float* tgts,
                         float* dw /*f32 [D, 3*P*P]*/, void* workspace, int batch, int Hp, int Wp, int P, int D,
                         hipStream_t stream);
/* input gradient of the patch embedding: the conv has stride = kernel, so d(imgs ; tgts) is one GEMM dcols = dPE . Wp followed by the
 * inverse of the im2col permutation, which the GEMM's epilogue applies while it stores (the zero-padding columns of Wp are dropped).
 * dpe: T [2BL, D] from pa_tokens_bwd (its y-stream rows already carry the (1 - w) factor of the mask blend); w: T [D, ldw] as for
 * pa_patch_embed_fwd.  dimgs / dtgts: f32 NCHW [B,3,Hp*P,Wp*P], either may be NULL (that stream's rows are then not contracted).
 * addend (optional, f32 NCHW like dtgts): dtgts = dcols(y rows) + alpha * addend.  Every pixel is written exactly once per stream (no
 * atomics, bitwise reproducible).  bf16 with P % 8 == 0 and D % 128 == 0: the 256x256 LDS-DMA kernel; every other case the generic engine. */
int pa_patch_embed_dgrad(int dtype, const void* dpe, const void* w, int64_t ldw, float* dimgs, float* dtgts, const float* addend,
                         float alpha, int batch, int Hp, int Wp, int P, int D, hipStream_t stream);
/* get_abs_pos (util/vitdet_utils.py:128-157) as the constant bicubic operator M [L, S] (host-built), in row-sparse form
 * (painter_amd/hostmath.py sparse_rows: int32 column indices + f32 values, K entries per row, zero-padded): pos = M . pe with
 * (idx, val, K) of M; dpe = M^T . (gx + gy) with those of M^T.  pe/dpe point at pos_embed[0, skip_cls:, :] ([S, D]). */
int pa_pos_fwd(const int* idx /*[L, K]*/, const float* val /*[L, K]*/, int K, const float* pe /*[S, D]*/, float* pos /*[L, D]*/, int L, int D,
               hipStream_t stream);
int pa_pos_bwd(const int* idxT /*[S, KT]*/, const float* valT /*[S, KT]*/, int KT, const float* gx /*[L, D]*/, const float* gy /*[L, D]*/,
               float* dpe /*[S, D]*/, int S, int D, hipStream_t stream);
/* backward of the token assembly: dpe T [2BL, D]; sums f32 [3, L, D] = sum_b dx | sum_b dy | sum_b w*dy */
int pa_tokens_bwd(int dtype, const float* dx0, const unsigned char* mask, int mask_batch_stride, void* dpe, float* sums,
                  int batch, int L, int D, hipStream_t stream);

/* ---- x = (x[:B] + x[B:]) * 0.5 after block merge_idx (models_painter.py:414-415) and its backward ---- */
int pa_merge_fwd(const float* x, float* out, int64_t n_out, hipStream_t stream);
int pa_merge_bwd(int dtype, const float* dmerged, float* dx, void* dxT, const float* rowscale, int rows_per_sample,
                 int64_t rows_half, int D, hipStream_t stream);
int pa_scale_cast(int dtype, const float* in, void* out, const float* rowscale, int rows_per_sample, int64_t rows, int D,
                  hipStream_t stream);
int pa_cast_bf16(const float* in, void* out, int64_t n, hipStream_t stream);
/* diagnostics only (tools/gradsync_overlap.py): scratch = 0.5 * (scratch + src), `passes` times, on exactly `nblocks` persistent
 * workgroups -- a stand-in for the CU / HBM footprint of a ring all-reduce with `nblocks` channels.  Never on the product path. */
int pa_debug_rmw(const float* src, float* scratch, int64_t n, int passes, int nblocks, hipStream_t stream);
/* SegGPT cross-prompt feature ensemble + residual (models_seggpt.py:220-232): x1 = x0 + ens(a), groups of `group` samples */
int pa_ensemble_resid(const float* x0, const float* a, float* x1, int batch, int group, int L, int D, hipStream_t stream);

/* ---- decoder_pred: Conv3x3(64->64) -> LayerNorm2D -> GELU -> Conv1x1(64->3), one fused kernel
 *      (models_painter.py:328-333,:430; util/vitdet_utils.py:204-209) and its backward pieces ---- */
int pa_conv3x3_pack(int dtype, const float* w3 /*[64,64,3,3]*/, void* w3r /*T [64][9][64]*/, void* wf /*T [64][9][64]*/,
                    hipStream_t stream);
int pa_decoder_tail_fwd(int dtype, const void* x_nhwc, const void* w3r, const float* b3, const float* ln_gamma,
                        const float* ln_beta, const float* w1 /*[3,64]*/, const float* b1, void* y3 /*T NHWC or NULL*/,
                        float* pred /*f32 NCHW [B,3,Hi,Wi]*/, int batch, int Hi, int Wi, float eps, hipStream_t stream);
int64_t pa_decoder_tail_bwd_workspace_bytes(int batch, int Hi, int Wi);
/* grads: f32 [324] = dgamma[64] | dbeta[64] | dW1[3*64] | db1[3] | pad; dy3: T NHWC gradient of the conv3x3 output */
int pa_decoder_tail_bwd_pointwise(int dtype, const float* dpred, const void* y3, const float* ln_gamma,
                                  const float* ln_beta, const float* w1, void* dy3, float* grads, void* workspace,
                                  int batch, int Hi, int Wi, float eps, hipStream_t stream);
/* dE: T [B*Hp*Wp, P*P*64] = gradient w.r.t. decoder_embed's output (pixel shuffle inverted in the epilogue) */
int pa_conv3x3_dgrad_unshuffle(int dtype, const void* dy3, const void* wf, void* dE, int batch, int Hp, int Wp, int P,
                               hipStream_t stream);
int64_t pa_conv3x3_wgrad_workspace_bytes(int batch, int Hi, int Wi);
int pa_conv3x3_wgrad(int dtype, const void* dy3, const void* x_nhwc, float* dw /*f32 [64,64,3,3]*/, void* workspace,
                     int batch, int Hi, int Wi, hipStream_t stream);

/* ---- decoder backward over the token rows the loss mask leaves live (bf16 256 x 256 / tile kernels only) ----
 * The loss is taken over masked patches only, so the gradient dE that enters decoder_embed is exactly zero on every token whose patch and
 * eight grid neighbours are unmasked (the tail is point-wise per pixel, the 3x3 conv has a one-pixel halo).  Nothing is read back to the host:
 * every kernel takes the live-row count through a device pointer, grids and buffers are sized for all B*L rows.
 *   pa_live_rows        token (b, i, j) is live when any mask byte of sample b in [i-1, i+1] x [j-1, j+1] is set (mask_batch_stride 0 = one
 *                       [1, L] mask for all samples).  rowmap int32 [B*L]: compact index or -1; live int32 [B*L]: token by compact index,
 *                       ascending; count int32 [1].  valid / the ignore rule are not consulted (they only zero more rows).
 *   pa_conv3x3_dgrad_unshuffle_live   pa_conv3x3_dgrad_unshuffle into the compact dE, bf16 [roundup(B*L, 128), P*P*64]: token row t at row
 *                       rowmap[t], nothing for dead tokens; rows [count, roundup(count, 128)) are zeroed, rows beyond are not touched.
 *   pa_gather_rows      dst row r = src row live[r] (r < count), zeros for r in [count, roundup(count, 128)); src NULL: the zero rows only.
 *                       Row pitches and the copied row length in bytes, multiples of 16; dst holds roundup(M, 128) rows.
 *   pa_linear_dgrad_live   dx[live[r]] = dy[r] . W for r < count (dy: compact bf16 [>= count rows, N]; each row in the dense launch's K order:
 *                       the same bits), exact zeros in the rows of dx whose rowmap entry is -1.  M = B*L rows of dx.
 *   pa_linear_wgrad_live   dW f32 [N, K] = dy^T . x over the first roundup(count, 128) rows of the compact dy [M, N] / x [M, K] (M % 128 == 0;
 *                       the rows between count and that bound must be zero in both); count = 0 writes a zero dW.
 *   pa_colsum_live      pa_colsum over the first count rows.
 *   pa_fill_dead_rows   zero the first row_bytes of the rows r of x (pitch_bytes apart, both % 16) with rowmap[r] < 0.
 *   pa_decoder_live_ok  host-only: 1 when the kernels take this decoder (Kin = decoder_embed's input width) and the switch is on --
 *                       pa_debug_set(17, v) / PAINTER_AMD_DECODER_ROWS: 0 default (on unless the environment says 0), 1 off, 2 on.
 * Non-finite values in a dead region no longer reach the gradients through 0 * inf (the same caveat as the DropPath skip). */
int pa_live_rows_max(void);       /* the largest B*L pa_live_rows takes (one workgroup, its flags in LDS) */
int pa_live_rows(const unsigned char* mask, int mask_batch_stride, int* rowmap, int* live, int* count, int batch, int Hp, int Wp,
                 hipStream_t stream);
int pa_conv3x3_dgrad_unshuffle_live(const void* dy3, const void* wf, void* dE_compact, const int* rowmap, const int* count, int batch,
                                    int Hp, int Wp, int P, hipStream_t stream);
int pa_gather_rows(const void* src, int64_t src_row_bytes, void* dst, int64_t dst_row_bytes, int64_t row_bytes, const int* live,
                   const int* count, int M, hipStream_t stream);
int pa_linear_dgrad_live(const void* dy, int64_t lddy, const void* w, void* dx, int64_t lddx, const int* live, const int* rowmap,
                         const int* count, int M, int N, int K, hipStream_t stream);
int pa_linear_wgrad_live(const void* dy, int64_t lddy, const void* x, int64_t ldx, float* dw, const int* count, int M, int N, int K,
                         hipStream_t stream);
int pa_colsum_live(int dtype, const void* x, int64_t ld, int M, int N, float* out, void* workspace, const int* count, hipStream_t stream);
int pa_fill_dead_rows(void* x, int64_t pitch_bytes, int64_t row_bytes, const int* rowmap, int M, hipStream_t stream);
int pa_decoder_live_ok(int dtype, int batch, int Hp, int Wp, int P, int Kin);

/* ---- forward_loss (models_painter.py:433-462; SegGPT models_seggpt.py:448-469) ----
 * out: f32 [2] = {loss, denominator}.  ignore_rule = 1 (Painter): samples whose unmasked de-normalised target sums
 * below 300 get valid := 0 IN PLACE (models_painter.py:444-448).  kind: 0 smoothl1(beta) 1 l1 2 l2 3 l1l2. */
int64_t pa_loss_workspace_bytes(int batch, int Hi, int Wi);
int pa_loss_fwd(const float* pred, const float* tgts, float* valid, const unsigned char* mask, int mask_batch_stride,
                float* out, void* workspace, int batch, int Hi, int Wi, int P, int ignore_rule, float eps_den, int kind,
                float beta, hipStream_t stream);
int pa_loss_bwd(const float* pred, const float* tgts, const float* valid, const unsigned char* mask,
                int mask_batch_stride, const float* dloss, const float* loss_out, float* dpred, int batch, int Hi, int Wi,
                int P, int kind, float beta, hipStream_t stream);
/* patchify (models_painter.py:355-368): f32 NCHW -> [B, L, P*P*3] */
int pa_patchify(const float* img, float* out, int batch, int Hp, int Wp, int P, hipStream_t stream);
/* gradient of pred when the returned prediction enters the objective, in one pass:
 *   dpred = [dloss != NULL] the pa_loss_bwd term (same arithmetic, same bits) + [dpatch != NULL] unpatchify(dpatch)
 * dpatch: f32 [B, L, P*P*3] (the gradient of pa_patchify's output); at least one of dloss / dpatch.  dpred_loss (optional, needs dloss)
 * receives the loss term alone: every loss kind depends on pred - tgts only, so the loss's direct gradient w.r.t. tgts is -dpred_loss. */
int pa_pred_bwd(const float* pred, const float* tgts, const float* valid, const unsigned char* mask, int mask_batch_stride,
                const float* dloss, const float* loss_out, const float* dpatch, float* dpred, float* dpred_loss, int batch, int Hi,
                int Wi, int P, int kind, float beta, hipStream_t stream);

/* ---- Optimizer step: GradScaler.unscale_ + clip_grad_norm_ + AdamW over the layer-decay groups in two passes.
 * Replaces Painter/util/misc.py:256-268 (NativeScalerWithGradNormCount.__call__) acting on the torch.optim.AdamW of
 * Painter/main_train.py:344-348 (parameter groups: util/lr_decay.py:15-61; schedule: util/lr_sched.py:9-21).
 * table: DEVICE array of ntensors records, first_chunk = running sum of ceil(n / pa_opt_chunk_elems()); nchunks = their total.
 * g == NULL marks a parameter without gradient (skipped).  All tensors fp32, contiguous. */
typedef struct PaOptTensor {
    void* p; const void* g; void* m; void* v;    /* parameter, gradient, exp_avg, exp_avg_sq */
    void* w16;                                   /* optional bf16 copy of p refreshed by pa_adamw_step, or NULL */
    int64_t n;                                   /* elements */
    int32_t group;                               /* index into PaOptGroups */
    int32_t first_chunk;
} PaOptTensor;
typedef struct PaOptGroups {                     /* HOST struct, passed by value to the kernel: at most 64 parameter groups */
    float lr[64], wd[64];                        /* learning rate (already times lr_scale), weight decay */
} PaOptGroups;
int pa_opt_chunk_elems(void);
int64_t pa_grad_sumsq_workspace_bytes(int nchunks);
/* out2 (device, 2 floats): [0] = sum over all gradients of g^2 (as stored, i.e. still multiplied by the loss scale),
 * [1] = 0 if every gradient is finite */
int pa_grad_sumsq(const PaOptTensor* table, int ntensors, int nchunks, float* out2, void* workspace, hipStream_t stream);
/* steps: DEVICE float[ntensors], one AdamW step count per table record, as torch.optim.AdamW keeps one per parameter: steps[t] is
 * advanced here exactly when record t has a gradient (g != NULL) and the step is not skipped, and record t's bias corrections
 * are taken from steps[t] alone -- a parameter that sits out a step keeps its count, whatever its group's other parameters do;
 * norm_info = out2 of pa_grad_sumsq or NULL (no clipping / no finiteness gate); grad_scale = device scalar the gradients are
 * divided by, or NULL; found_inf = device scalar, nonzero skips the step (torch GradScaler protocol), or NULL;
 * max_norm <= 0 disables clipping.  groups is a HOST pointer.  beta1 / beta2 are doubles: 1 - beta and 1 - beta^step are formed in
 * double from the unrounded values, as torch forms them, and only then rounded to float. */
int pa_adamw_step(const PaOptTensor* table, int ntensors, int nchunks, const PaOptGroups* groups, double beta1, double beta2,
                  float eps, float* steps, const float* norm_info, const float* grad_scale, const float* found_inf,
                  float max_norm, hipStream_t stream);

/* ---- SegGPT pre-/post-processing on the device.  Replaces the PIL / numpy / CPU-torch work of
 * SegGPT/SegGPT_inference/seggpt_engine.py: inference_image :56-103, inference_video :106-181, run_one_image :26-53.
 * Images are uint8 [H][W][C] (C <= 4), densely packed, in device memory; everything is bit-exact with the reference's host path:
 * integer arithmetic for the resize passes, float64 with one rounding per operation for normalise / de-normalise / blend. ---- */
/* One separable pass of Pillow's ImagingResample for 8-bit pixels (`Image.resize`, default BICUBIC; :62, :66, :117, :136):
 * out = clip8((2^21 + sum_t src[first + t] * coeffs[o][t]) >> 22) along the width (vertical = 0: dst is [src_h][dst_w]) or the
 * height (vertical = 1: dst is [dst_h][src_w]).  bounds: int32 [n_out][2] = (first, taps); coeffs: int32 [n_out][ksize]. */
int pa_resample_u8(const void* src, int src_h, int src_w, void* dst, int dst_h, int dst_w, int channels, const void* bounds,
                   const void* coeffs, int ksize, int vertical, hipStream_t stream);
/* `Image.resize(size, Image.NEAREST)` (:70, :121) and any other index-table gather: dst[y][x] = src[ytab[y]][xtab[x]], 0 where a
 * table entry is negative.  ytab: int32 [dst_h], xtab: int32 [dst_w]. */
int pa_gather_u8(const void* src, int src_h, int src_w, void* dst, int dst_h, int dst_w, int channels, const void* ytab,
                 const void* xtab, hipStream_t stream);
/* :73-92 + :28-34: imgs[n] = [prompt_n ; query], tgts[n] = [target_n ; target_n] along H, (v / div - mean) / std in float64, written
 * as float32 NCHW [n_prompts][3][2*res_h][res_w].  prompts / targets: uint8 [n_prompts][res_h][res_w][3]; query: uint8
 * [res_h][res_w][3]; target_div: DEVICE double [n_prompts] (255 for image-scale targets, 1 for the cached {0,1} masks, :166-171). */
int pa_seggpt_stitch(const void* prompts, const void* targets, const void* target_div, const void* query, float* imgs,
                     float* tgts, int n_prompts, int res_h, int res_w, hipStream_t stream);
/* :49-53: pred = the model's float32 tokens of sample 0, [2*res_h/patch * res_w/patch][patch*patch*3]; out = float64
 * [res_h][res_w][3] = clip((lower half of unpatchify(pred) * std + mean) * 255, 0, 255). */
int pa_seggpt_decode(const float* pred, void* out_f64, int res_h, int res_w, int patch, hipStream_t stream);
/* :166-171: out uint8 [res_h][res_w][3] = (mean over channels of the decoded picture > 128), the next video prompt target. */
int pa_seggpt_mask(const float* pred, void* out_u8, int res_h, int res_w, int patch, hipStream_t stream);
/* :95-102, :173-179 fused: decode, nearest-resize to out_h x out_w through ytab / xtab (int32 source rows / columns of the
 * res_h x res_w picture, F.interpolate(mode='nearest') rule), out = uint8(image * (0.6 * picture / 255 + 0.4)) (truncation).
 * image, out: uint8 [out_h][out_w][3]. */
int pa_seggpt_blend(const float* pred, const void* image, void* out, int out_h, int out_w, const void* ytab, const void* xtab,
                    int res_h, int res_w, int patch, hipStream_t stream);

/* ---- Painter training input pipeline, pixel work on the device.  Replaces, per sample, the PIL / CPU-torch work of
 * Painter/data/pairdataset.py:106-190 under the transform stack of Painter/main_train.py:232-251 (Painter/data/pair_transforms.py).
 * Random parameters (crop boxes, jitter order and factors, flip flags) are inputs: drawing them stays on the host. ---- */
/* RandomResizedCrop on decoded uint8 pictures (pair_transforms.py:152-163 -> PIL crop + resize): pa_resample_u8 / pa_gather_u8 on a
 * box of a larger picture -- src points at the box's first pixel, rows are src_row_bytes apart. */
int pa_resample_u8_box(const void* src, int64_t src_row_bytes, int src_h, int src_w, void* dst, int dst_h, int dst_w, int channels,
                       const void* bounds, const void* coeffs, int ksize, int vertical, hipStream_t stream);
int pa_gather_u8_box(const void* src, int64_t src_row_bytes, int src_h, int src_w, void* dst, int dst_h, int dst_w, int channels,
                     const void* ytab, const void* xtab, hipStream_t stream);
/* ColorJitter (pair_transforms.py:236-247 -> PIL ImageEnhance.Brightness / Contrast / Color and the HSV hue shift), in place on uint8
 * [batch][h][w][3].  ops: DEVICE int32 [batch][4], the op of each of the four slots in applied order (0 brightness, 1 contrast,
 * 2 saturation, 3 hue, negative = none); factors: DEVICE float [batch][4] (hue slot: the uint8 added to the H plane, as a float);
 * ops_host: HOST copy of ops, or NULL (then every slot and its mean pass is launched).  Bit-exact with Pillow. */
int64_t pa_color_jitter_workspace_bytes(int batch);
int pa_color_jitter(void* images, const void* ops, const void* factors, const void* ops_host, void* workspace, int batch, int h, int w,
                    hipStream_t stream);
/* RandomHorizontalFlip + ToTensor + Normalize (pair_transforms.py:199-203, :72, :101) and the two-pair stitch (pairdataset.py:100-104):
 * uint8 [batch][h][w][3] -> rows [row0, row0 + h) of float32 [batch][3][canvas_h][w]; flip: DEVICE int32 [batch]. */
int pa_to_tensor_normalize(const void* images, const void* flip, float* canvas, int batch, int h, int w, int canvas_h, int row0,
                           hipStream_t stream);
/* Second RandomResizedCrop on the float canvases (main_train.py:248-250): dst[b] = interpolate(src[b][:, top:top+bh, left:left+bw],
 * size = (h, w)), bicubic (A = -0.75, align_corners = False, no antialias) or nearest.  boxes: DEVICE int32 [batch][4] =
 * (top, left, bh, bw).  src != dst. */
int pa_resized_crop_f32(const float* src, float* dst, const void* boxes, int batch, int channels, int h, int w, int nearest,
                        hipStream_t stream);
/* The same with a per-sample mode: modes = DEVICE int32 [batch], 0 bicubic, 1 nearest, 2 the sample keeps its canvas (plain copy): the
 * samples of a step that take no second crop, or different interpolations (pairdataset.py:113-124), go through one launch. */
int pa_resized_crop_f32_modes(const float* src, float* dst, const void* boxes, const void* modes, int batch, int channels, int h, int w,
                              hipStream_t stream);
/* RandomResizedCrop (pair_transforms.py:152-163 -> PIL crop + resize) for every decoded picture of a step in two launches.  jobs: DEVICE
 * array of n_jobs descriptors; every pointer in a job is a device address.  Bicubic jobs: xbounds / ybounds = int32 [out][2] (first
 * tap, taps), xcoeffs / ycoeffs = int32 [out][ksize] -- Pillow's fixed-point tables (painter_amd.hostmath / RS.bicubic_tables), a pass
 * whose size does not change is skipped as in Pillow and its tables may be NULL.  Nearest jobs: xbounds = int32 [out_w] source column,
 * ybounds = int32 [out_h] source row (PIL nearest tables), unused when the size does not change.  mid: DEVICE scratch of
 * (sum of the bicubic jobs' h) * out_w * 3 bytes; a job's rows start at row mid_row0.  max_h / max_w: the largest box.  Bytes are
 * identical to pa_resample_u8_box / pa_gather_u8_box applied picture by picture. */
typedef struct pa_crop_job {
    const void* src;            /* first pixel of the crop box, uint8 RGB, rows src_row_bytes apart */
    void* dst;                  /* uint8 [out_h][out_w][3] */
    const void* xbounds;
    const void* xcoeffs;
    const void* ybounds;
    const void* ycoeffs;
    int64_t src_row_bytes;
    int32_t h, w;               /* box size */
    int32_t xksize, yksize;
    int32_t nearest;            /* 0 bicubic, 1 PIL nearest */
    int32_t mid_row0;
} pa_crop_job;
int pa_resized_crop_u8_batch(const pa_crop_job* jobs, void* mid, int n_jobs, int max_h, int max_w, int out_h, int out_w, hipStream_t stream);
/* `valid` rules (pairdataset.py:152-180) on float32 [batch][3][plane] targets.  modes: DEVICE int32 [batch] (0 ones; 1 target < thres
 * -> 0; 2 target > thres -> 10 and all 0 if fewer than 300 foreground elements; 3 all 0 if fewer than 300 foreground elements);
 * thres: DEVICE float [batch][3]. */
int64_t pa_pair_valid_workspace_bytes(int batch);
int pa_pair_valid(const float* tgts, float* valid, const void* modes, const void* thres, void* workspace, int batch, int plane,
                  hipStream_t stream);

/* ---- Painter task inference, pre-/post-processing on the device.  Replaces the numpy / CPU-torch work around the model call in the
 * eight scripts Painter/eval/<task>/painter_inference_*.py (ade20k_semantic/..._segm.py, coco_panoptic/..._pano_semseg.py and ..._pano_inst.py,
 * mmpose_custom/..._pose.py, nyuv2_depth/..._depth.py, derain/..._derain.py, lol/..._lol.py, sidd/..._sidd.py) and the colour -> class
 * decode of ade20k_semantic/ADE20kSemSegEvaluatorCustom.py, for a batch of pictures per launch.  uint8 / int32 outputs are bit-exact with
 * the scripts' host path (float64 throughout, CPU torch's bilinear operation order); the bicubic float64 output agrees to ~1e-13. ---- */
/* painter_inference_segm.py:150-162 for n_queries pictures: imgs[n] = [prompt ; query_n], tgts[n] = [prompt_target ; prompt_target]
 * along H ("tgt is not available"), (v / 255 - mean) / std in float64, written as float32 NCHW [n_queries][3][2*res_h][res_w].
 * prompt, prompt_target: uint8 [res_h][res_w][3]; queries: uint8 [n_queries][res_h][res_w][3]. */
int pa_painter_stitch(const void* prompt, const void* prompt_target, const void* queries, float* imgs, float* tgts, int n_queries,
                      int res_h, int res_w, hipStream_t stream);
/* One output picture of a decode launch.  The decode entry points take pred = the model's float32 tokens
 * [n_samples][2*res_h/patch * res_w/patch][patch*patch*3] and jobs = DEVICE array of n_jobs records; the source of a job is the lower
 * half of unpatchify(pred[sample]); max_h / max_w = the largest out_h / out_w of the table.  A job whose sample is outside
 * [0, n_samples) writes nothing. */
typedef struct pa_decode_job {
    void* out;                  /* device address of this picture's output, densely packed */
    void* out2;                 /* pa_painter_decode_f64: optional uint8 [out_h][out_w][3], or NULL; unused otherwise */
    int32_t sample;
    int32_t out_h, out_w;
    int32_t reserved;
} pa_decode_job;
/* ..._segm.py:88-92, ..._pano_semseg.py:88-92 (nearest = 0: F.interpolate bilinear), ..._pano_inst.py:88-92, ..._pose.py:86-91 (nearest = 1):
 * out = uint8 [out_h][out_w][3] = trunc(resize(clip((y * std + mean) * 255, 0, 255))). */
int pa_painter_decode_u8(const float* pred, const pa_decode_job* jobs, int n_jobs, int n_samples, int max_h, int max_w, int res_h,
                         int res_w, int patch, int nearest, hipStream_t stream);
/* ..._depth.py:69-73: out = int32 [out_h][out_w] = trunc(mean over channels of bilinear(clip((y * std + mean) * 10000, 0, 10000))). */
int pa_painter_decode_depth(const float* pred, const pa_decode_job* jobs, int n_jobs, int n_samples, int max_h, int max_w, int res_h,
                            int res_w, int patch, hipStream_t stream);
/* ..._derain.py:76-79, ..._lol.py:65-68, ..._sidd.py:81-84: out = float64 [out_h][out_w][3] = bicubic (A = -0.75, align_corners = False,
 * border indices clamped) resize of y * std + mean, no clip; out2 (if not NULL) = uint8(clip(out, 0, 1) * 255), the picture they save. */
int pa_painter_decode_f64(const float* pred, const pa_decode_job* jobs, int n_jobs, int n_samples, int max_h, int max_w, int res_h,
                          int res_w, int patch, hipStream_t stream);
/* ADE20kSemSegEvaluatorCustom.py:114-141: out = int32 [h][w] = index of the FIRST minimum over the n_colours (<= 4096) palette rows of
 * sum_c d(pixel_c - colour_c) in float32; dist_type 0 d = abs, 1 d = square, 2 d = (abs + square) / 2.  image: uint8 [h][w][3];
 * palette: float32 [n_colours][3]. */
int pa_palette_argmin(const void* image, const float* palette, void* out_i32, int h, int w, int n_colours, int dist_type,
                      hipStream_t stream);
/* Class-agnostic instance decode: coco_panoptic/COCOCAInstSegEvaluatorCustom.py:252-354 (post_process_segm_output_by_threshold, the
 * evaluator's default `--post_type threshold`) followed by util/matrix_nms.py:5-121 (mask_matrix_nms), csrc/painter_inst.hip.
 * image: uint8 [h][w][3]; palette: DEVICE float32 [n_colours][3] of integer values 0..255 (define_colors_per_location_r_gb, :42-67, without
 * the background row); thresholds: DEVICE float32 [n_thr].  Candidate t * n_colours + c is the mask  float(L1) / 3.0f < thresholds[t]
 * (:288-290), L1 = sum over channels of |pixel - colour|, with n pixels and S = sum of L1 over them; maskness = S / (3 n) (:296).
 * Where the reference leaves ties to float32 rounding and an unspecified sort, this path defines them: n, S, areas and intersections are
 * exact integers; the first sort (:319) compares S1 * n2 with S2 * n1 in int64, ties to the lower candidate index; the sorts of
 * matrix_nms.py:53 and :112 are descending, ties to the earlier position; the NMS arithmetic (:67-99) is float64; scores leave as float32.
 * Capacities: h, w <= 16384, h * w <= 2^24, n_thr <= 8, n_thr * n_colours <= 65536, nms_pre <= 4096, max_num <= nms_pre.  Null pointers,
 * sizes < 1 or sizes beyond a capacity return hipErrorInvalidValue before anything is launched. */
/* host only: bytes of the workspace of pa_inst_decode, -1 for bad arguments.  ~ nms_pre * h * w / 8 (bit masks) + 4 * nms_pre^2
 * (intersections) + 16 * n_thr * n_colours. */
int64_t pa_inst_workspace_bytes(int h, int w, int n_colours, int n_thr, int nms_pre);
/* host only, for tests and tools: byte offset of a section of that workspace after a decode.  0: n, uint32 [n_thr * n_colours];
 * 1: S, uint64 [n_thr * n_colours]; 2: int32 {live candidates, survivors}; 3: survivors' candidate indices in NMS order, int32 [nms_pre];
 * 4: their areas, int32; 5: their scores before the NMS, float64; 6: their bit masks, uint32 [nms_pre][stride]; 7: intersections,
 * int32 [nms_pre][nms_pre], defined for i < j < survivors; 8: scores after the NMS, float64; 9: not an offset, the stride of section 6 in
 * words (words rounded up to a multiple of 4). */
int64_t pa_inst_workspace_offset(int h, int w, int n_colours, int n_thr, int nms_pre, int section);
/* :288-296, the first stage alone: n_u32 = uint32 [n_thr][n_colours], s_u64 = uint64 [n_thr][n_colours] (both cleared first). */
int pa_inst_stats(const void* image, const float* palette, const float* thresholds, void* n_u32, void* s_u64, int h, int w, int n_colours,
                  int n_thr, hipStream_t stream);
/* matrix_nms.py:65-67 on bit masks: masks_u32 = uint32 [n_rows][words], bit b of word k = pixel 32 k + b, words a multiple of 4, 16-byte
 * aligned; inter_i32 = int32 [n_rows][ld] (cleared first), inter[i][j] = shared pixels for i < j, and for every i, j inside a diagonal
 * 64 x 64 tile; the rest of the lower triangle stays 0. */
int pa_inst_intersections(const void* masks_u32, int n_rows, int words, void* inter_i32, int ld, hipStream_t stream);
/* The whole decode, nothing but launches on `stream`.  nms_pre: the literal 2000 of :318; max_num: 100 of :332; kernel: 0 gaussian
 * (exp(-sigma iou^2), :333), 1 linear; workspace: pa_inst_workspace_bytes, 256-byte aligned.  DEVICE outputs: out_count int32 [1] =
 * number of instances n <= max_num (0: no candidate -- the reference then reports ONE all-zero mask with score 0 and label 0, :302-310,
 * which callers restate); out_scores float32 [max_num]; out_scores_f64 float64 [max_num] before the cast, or NULL; out_candidates int32
 * [max_num] = t * n_colours + c; out_masks uint32 [max_num][ceil(h * w / 32)]; out_masks_u8 uint8 [max_num][h * w], the same masks with one
 * byte (0 / 1) per pixel, or NULL.  Entries past n are 0. */
int pa_inst_decode(const void* image, const float* palette, const float* thresholds, int h, int w, int n_colours, int n_thr, int nms_pre,
                   int max_num, float sigma, int kernel, void* workspace, void* out_count, float* out_scores, void* out_scores_f64,
                   void* out_candidates, void* out_masks, void* out_masks_u8, hipStream_t stream);

/* Panoptic merge of a painted `coco_pano_semseg` picture with instances, csrc/painter_pano.hip: class vote
 * (coco_panoptic/COCOPanoEvaluatorCustom.py:259-276, COCOInstSegEvaluatorCustom.py:169-186), paste (COCOPanoEvaluatorCustom.py:69-109) and
 * stuff fill (:111-132) on integers and bit masks; tests/painter_pano_host.py is the definition.
 * image: uint8 [h][w][3]; palette: DEVICE float32 [n_colours][3] of integer values 0..255 (define_colors_by_mean_sep,
 * data/coco_semseg/gen_color_coco_panoptic_segm.py:31-54); labels < n_things are things; dist_type: the codes of pa_palette_argmin.
 * Instances: masks_u32 = uint32 [max_inst][ceil(h * w / 32)], bit b of word k = pixel 32 k + b (pa_inst_decode's out_masks; padding bits of
 * the last word are ignored); scores float32 [max_inst]; n_dev = DEVICE int32 [1], the number of instances (clamped to 0..max_inst).
 * Capacities: h * w <= 2^24, n_colours <= 1024, 2 <= n_things <= n_colours, 1 <= max_inst <= 1024.  Null required pointers, sizes beyond a
 * capacity, NaN thresholds or a workspace that is not 256-byte aligned return hipErrorInvalidValue before anything is launched. */
typedef struct pa_pano_segment {
    int id;              /* 1, 2, ...: the value of its pixels in the panoptic map */
    int isthing;
    int category_id;     /* voted (or given) class of a thing, semantic label of stuff */
    int instance_id;     /* index of the instance; -1 for stuff */
    int area;            /* pixels that finally carry the id (the reference reports it for stuff only, :130) */
    float score;         /* 0 for stuff */
} pa_pano_segment;
/* host only: bytes of the workspace of pa_pano_merge / pa_pano_decode, -1 for bad arguments.
 * ~ 8 * max_inst * n_things (vote sums) + h * w * (4 + 1/8) (semantic map, union bits) + 8 * n_colours + 4 * max_inst. */
int64_t pa_pano_workspace_bytes(int h, int w, int n_colours, int n_things, int max_inst);
/* masks_u8: uint8 / bool [n_rows][h * w], non-zero = set -> out_u32 = uint32 [n_rows][ceil(h * w / 32)] in the layout above, padding bits 0:
 * for masks that do not come from pa_inst_decode (the pre-computed route, COCOPanoEvaluatorCustom.py:229-248).  n_rows <= 1024. */
int pa_pack_mask_bits(const void* masks_u8, int n_rows, int h, int w, void* out_u32, hipStream_t stream);
/* :259-276 / COCOInstSegEvaluatorCustom.py:169-186 alone: out_s_u64 = uint64 [max_inst][n_things] (cleared first), S[i][k] = sum over the
 * pixels of mask i of d2(pixel, colour k), d2 = sum_c |d| (abs), sum_c d^2 (square), sum_c (|d| + d^2) (mean: twice the reference's);
 * out_classes = int32 [max_inst], first minimum of row i (= the reference's argmax of sum (1 - d / max d), and of its softmax); an empty mask
 * and the slots past the count get 0. */
int pa_pano_vote(const void* image, const float* palette, const void* masks_u32, const void* n_dev, int h, int w, int n_colours, int n_things,
                 int dist_type, int max_inst, void* out_s_u64, void* out_classes, hipStream_t stream);
/* :69-132 from a given semantic map (int32 [h][w], pa_palette_argmin's output) and classes (int32 [max_inst]).  Instances are visited in
 * descending score order, ties to the lower index (a NaN score last); stop at the first (double)score < instances_score_thresh; skip area 0
 * and (double)intersection / (double)area > overlap_threshold, intersection with the union of the masks accepted so far; an accepted
 * instance gets the next id from 1 and owns its pixels outside that union.  Then every label l >= n_things in ascending order whose count c
 * of pixels outside the union has not (double)c < stuff_area_thresh gets the next id (a threshold <= 0 therefore also keeps labels without
 * a pixel, which the reference's torch.unique never visits).  DEVICE outputs: out_panoptic int32 [h][w], 0 = unassigned; out_rgb uint8
 * [h][w][3] = panopticapi id2rgb (r = id % 256, g = id / 256 % 256, b = id / 65536), or NULL; out_count int32 [1] = segments;
 * out_segments pa_pano_segment [max_inst + n_colours - n_things], entries past the count 0. */
int pa_pano_merge(const void* semmap_i32, const void* masks_u32, const float* scores, const void* classes_i32, const void* n_dev, int h, int w,
                  int n_colours, int n_things, int max_inst, double overlap_threshold, double stuff_area_thresh, double instances_score_thresh,
                  void* workspace, void* out_panoptic, void* out_rgb, void* out_count, void* out_segments, hipStream_t stream);
/* The whole definition, nothing but launches on `stream`: pa_palette_argmin into the workspace, the vote (skipped when classes_i32, int32
 * [max_inst], is given: it is copied to out_classes), then the merge.  out_classes int32 [max_inst] is required. */
int pa_pano_decode(const void* image, const float* palette, const void* masks_u32, const float* scores, const void* n_dev,
                   const void* classes_i32, int h, int w, int n_colours, int n_things, int dist_type, int max_inst, double overlap_threshold,
                   double stuff_area_thresh, double instances_score_thresh, void* workspace, void* out_panoptic, void* out_rgb, void* out_count,
                   void* out_segments, void* out_classes, hipStream_t stream);

/* Keypoints of painted `coco_pose` pictures, csrc/painter_pose.hip: TopDownCustom.forward_pseudo_test (mmpose_custom/model/top_down.py:
 * 163-258) and mmpose's keypoints_from_heatmaps (post_process 'default', no UDP) without a heat map in memory; tests/painter_pose_host.py
 * is the definition.
 * pictures: uint8 [n][h][w][3]; flipped: the pictures painted for the mirrored boxes, same shape, or NULL for no flip test;
 * palette_i32: DEVICE int32 [n_keypoints + 1][2], the (G, B) colour of every channel, background LAST (define_colors_gb_mean_sep,
 * data/pipelines/custom_transform.py:10-33); pair_i32: DEVICE int32 [n_keypoints], the channel that a mirror swaps each channel with
 * (pair[pair[k]] == k; values outside 0..n_keypoints-1 are clamped).  A pixel's class is the first minimum of |G - g_c| + |B - b_c|; the
 * heat of channel k is float32(R) / 255 where the class is k, else 0.  With `flipped`: F_k(y, x) = heat of channel pair[k] of the flipped
 * picture at (y, w - 1 - x); shift != 0 moves F one column right (column 0 keeps its value); out = (heat + F) / 2 in float32 -- one float32
 * add of two table values and an exact halving, which decides ties exactly as the reference's arrays do.  Without: out = heat.
 * n, h, w >= 1, h * w < 2^31, 1 <= n_keypoints <= 32, n * ceil(h * w / 256) < 2^31; otherwise, or for a null required pointer,
 * hipErrorInvalidValue before anything is launched. */
/* host only: bytes of pa_pose_keypoints's workspace (one 64-bit key per box and channel), -1 for bad arguments. */
int64_t pa_pose_workspace_bytes(int n, int n_keypoints);
/* Per box and channel the first maximum of `out` in row-major order: out_maxvals float32 [n][n_keypoints], out_preds float32
 * [n][n_keypoints][2] = (x, y) in heat-map pixels, moved by 0.25 * sign(out[y][x + 1] - out[y][x - 1]) (and likewise over rows) where
 * 1 < x < w - 1 and 1 < y < h - 1; (-1, -1) and 0 for a channel without a positive value.  workspace: pa_pose_workspace_bytes, 8-byte
 * aligned.  Nothing but a memset and two launches on `stream`; deterministic. */
int pa_pose_keypoints(const void* pictures, const void* flipped, const void* palette_i32, const void* pair_i32, int n, int h, int w,
                      int n_keypoints, int shift, void* workspace, float* out_preds, float* out_maxvals, hipStream_t stream);
/* `out` itself, float32 [n][n_keypoints][h][w]: what forward_pseudo_test returns with return_heatmap=True. */
int pa_pose_heatmaps(const void* pictures, const void* flipped, const void* palette_i32, const void* pair_i32, int n, int h, int w,
                     int n_keypoints, int shift, float* out_heatmaps, hipStream_t stream);

/* Scoring of painted pictures against ground-truth maps, csrc/painter_score.hip: only the sums leave the device;
 * tests/painter_score_host.py is the definition.  The entry points take a DEVICE job table, one record per picture, pictures of any
 * sizes in one launch; null pointers, n_jobs outside 1 .. 65535 or the ranges named below return hipErrorInvalidValue before anything is
 * launched. */
typedef struct pa_score_job {
    const void* picture;        /* uint8 [h][w][3], the painted picture */
    const void* gt;             /* uint8 [h][w], the ground-truth labels */
    int32_t h, w;               /* a job with h < 1 or w < 1 adds nothing */
} pa_score_job;
/* SemSegEvaluatorCustom.process (ade20k_semantic/ADE20kSemSegEvaluatorCustom.py:75-112, coco_panoptic/COCOPanoSemSegEvaluatorCustom.py:
 * 67-106) without its boundary branch: for every pixel of every job conf[(n_colours + 1) * pred + gt'] += 1, pred = the class
 * pa_palette_argmin gives the pixel (the same float32 operations, first minimum; palette: DEVICE float32 [n_colours][3]; dist_type: its
 * codes), gt' = n_colours where gt == ignore_label, else gt.  A pixel whose gt >= n_colours is not the ignore label (the reference's
 * reshape fails on it) adds 1 to invalid[0] and to no bin.  conf_i64: int64 [(n_colours + 1)^2], invalid_i64: int64 [1], both 8-byte
 * aligned and ACCUMULATED in place: one buffer serves a data set.  total_pixels: the sum of h * w over the table, 1 .. 2^31 (it sizes the
 * grid; a workgroup counts into 32-bit bins in LDS, which a launch of at most 2^31 pixels cannot wrap).  1 <= n_colours <= 255 (gt is a
 * byte).  bins: 0 = the workgroups' private bins are in LDS whenever pa_semseg_lds_bins(n_colours) (n_colours <= 199: 12 n_colours
 * rounded up to 16, plus 4 (n_colours + 1)^2 bytes within 160 KB), else every run of equal neighbours adds to conf_i64 directly; 1 = the
 * direct form at any n_colours (measurements).  Integer atomics only: the result does not depend on their order.  The boundary branch
 * is pa_semseg_boundary_confusion below, which counts this matrix and the boundary matrix in one call. */
int pa_semseg_lds_bins(int n_colours);
int pa_semseg_confusion(const pa_score_job* jobs, int n_jobs, int64_t total_pixels, const float* palette, int n_colours, int dist_type,
                        int ignore_label, int bins, void* conf_i64, void* invalid_i64, hipStream_t stream);
typedef struct pa_boundary_job {
    const void* picture;        /* uint8 [h][w][3], the painted picture */
    const void* gt;             /* uint8 [h][w], the ground-truth labels */
    int32_t h, w;               /* a job with h < 1 or w < 1 adds nothing */
    int32_t d;                  /* the picture's dilation, >= 1: max(1, round(dilation_ratio * sqrt(h^2 + w^2))), computed by the caller */
    int32_t reserved;
} pa_boundary_job;
/* SemSegEvaluatorCustom.process WITH its boundary branch (ADE20kSemSegEvaluatorCustom.py:103-110, COCOPanoSemSegEvaluatorCustom.py:97-104;
 * detectron2's SemSegEvaluator._compute_boundary_iou, restated from detectron2's published source and unverified against detectron2 / cv2,
 * neither of which is available where this project is tested; tests/painter_boundary_host.py is the definition).  conf_i64 and invalid_i64
 * receive exactly what pa_semseg_confusion adds for the same pictures -- a pixel's class is evaluated once -- and for every pixel of every
 * job bconf[(n_colours + 1) * boundary(pred) + boundary(gt')] += 1, where boundary(m) = m - eroded(m) and eroded(m)[y][x] = the minimum of
 * the uint8 map m over rows y - d .. y + d and columns x - d .. x + d with every pixel outside the picture read as 0: cv2.erode by a 3 x 3
 * square, d iterations, of the map behind a ring of one zero pixel.  The minimum is over label VALUES, as detectron2 erodes the label map
 * itself.  Any d >= 1 (d >= w or d >= h: everything is boundary); a job with d < 1 enters conf_i64 only.  What a pixel counted in
 * invalid_i64 adds to bconf is unspecified.  1 <= n_colours <= 254 (detectron2 switches the branch off from 255 classes); bconf_i64:
 * int64 [(n_colours + 1)^2], 8-byte aligned, accumulated in place; bins as above, for both matrices.  workspace:
 * pa_semseg_boundary_workspace_bytes(total_pixels) bytes = four byte maps (pred, gt', their row minima) of total_pixels rounded up to 16;
 * total_pixels is the sum of h * w over the table, 1 .. 2^31, and jobs beyond it are counted in conf_i64 but not in bconf_i64.  Three
 * launches, integer atomics only. */
int64_t pa_semseg_boundary_workspace_bytes(int64_t total_pixels);          /* host only; -1 for bad arguments */
int pa_semseg_boundary_confusion(const pa_boundary_job* jobs, int n_jobs, int64_t total_pixels, const float* palette, int n_colours,
                                 int dist_type, int ignore_label, int bins, void* conf_i64, void* bconf_i64, void* invalid_i64,
                                 void* workspace, hipStream_t stream);
/* boundary(map) of one DEVICE uint8 map [h][w] as above -> out_u8 [h][w], through the scorer's own row and column passes.  h, w, d >= 1,
 * h * w <= 2^31; workspace: pa_semseg_boundary_workspace_bytes(h * w) (one map of it is used). */
int pa_label_boundary(const void* map_u8, int h, int w, int d, void* out_u8, void* workspace, hipStream_t stream);
typedef struct pa_depth_job {
    const void* pred;           /* int32 [h][w], what pa_painter_decode_depth writes */
    const void* gt;             /* uint16 [h][w], the ground-truth depth PNG's values */
    int32_t h, w;
    int32_t y0, y1, x0, x1;     /* the evaluated box, rows y0 .. y1 - 1 and columns x0 .. x1 - 1, clipped to the picture */
} pa_depth_job;
/* nyuv2_depth/eval_with_pngs.py:148-209 (eval, dataset nyu) and :50-71 (compute_errors) up to the sums.  Per pixel of the box, the
 * float32 steps in float32: p = float(pred) / divisor clamped to [min_depth, max_depth] (:100, :177-178), g = float(gt) / divisor (:136);
 * the pixel counts when min_depth < g < max_depth (:184); t = max(g / p, p / g) (:51).  out_f64: double [n_jobs][10] = n, the counts of
 * t < 1.25, t < 1.5625, t < 1.953125, then the float64 sums over float64 terms of (g - p)^2, (ln g - ln p)^2, |g - p| / g, (g - p)^2 / g,
 * ln p - ln g and |log10 p - log10 g|, from which the nine numbers of :71 follow.  The eigen crop of :205 is the box 45, 471, 41, 601; the
 * KITTI branches are not here.  divisor > 0 (1000 for NYU), 0 < min_depth < max_depth < inf.  workspace: pa_depth_workspace_bytes(n_jobs),
 * 8-byte aligned, as out_f64.  Two launches, no floating-point atomics: a workgroup's partial is summed in a fixed order and a job's
 * partials are added in index order, so two runs give the same bits. */
int64_t pa_depth_workspace_bytes(int n_jobs);     /* host only; -1 for bad arguments */
int pa_depth_errors(const pa_depth_job* jobs, int n_jobs, float divisor, float min_depth, float max_depth, void* out_f64, void* workspace,
                    hipStream_t stream);

/* PSNR and SSIM of restored pictures against their ground truth, csrc/painter_restore.hip: what painter_inference_lol.py:166-169 asks of
 * skimage and what derain's evaluate_PSNR_SSIM.m computes from the saved PNGs, up to the sums; tests/painter_restore_host.py is the
 * definition.  Pictures of any sizes in one call.  Unlike the tables above this one is a HOST array: the entry point reads it, so that a
 * picture smaller than the window is refused before anything is enqueued, and copies it into the workspace on the stream (keep it valid
 * until that copy has run; pinned memory makes the copy asynchronous). */
#define PA_RESTORE_RGB_F64 0    /* pred: float64 [h][w][3], clipped to [0, 1] in the kernel; gt: uint8 [h][w][3], gt / 255. in float64;
                                 * the three channels are scored separately */
#define PA_RESTORE_Y_U8 1       /* pred, gt: uint8 [h][w][3]; one channel, Y = 16 + (65481 R + 128553 G + 24966 B + 127500) / 255000 in
                                 * integers: the Y row of rgb2ycbcr rounded half up, exact */
typedef struct pa_restore_job {
    const void* pred;           /* DEVICE picture, by mode; float64 pictures 8-byte aligned */
    const void* gt;             /* DEVICE uint8 [h][w][3] */
    int32_t h, w;               /* both >= win */
} pa_restore_job;
/* host only: the side of a workgroup's tile of output windows (24).  A job of mode m has channels(m) * ceil((h - win + 1) / tile) *
 * ceil((w - win + 1) / tile) tiles; channels = 3 for PA_RESTORE_RGB_F64, 1 for PA_RESTORE_Y_U8. */
int pa_restore_tile(void);
/* host only: bytes of pa_restore_scores's workspace for a table of n_jobs jobs with total_tiles tiles in all (16 bytes per tile and the
 * device copy of the table); -1 for n_jobs outside 1 .. 1024 or total_tiles outside 1 .. 2^24. */
int64_t pa_restore_workspace_bytes(int n_jobs, int64_t total_tiles);
/* Per window of `win` x `win` pixels with the separable weights weights_f64[win] (HOST; 1/7 x 7 for skimage's uniform window, the
 * normalised 11-tap Gaussian of sigma 1.5 for SSIM_index), full windows only: ux, uy, uxx, uyy, uxy = the weighted means of x, y, x x,
 * y y, x y (x = prediction plane, y = ground-truth plane, rows first, then columns); vx = cov_norm (uxx - ux ux), vy likewise, vxy =
 * cov_norm (uxy - ux uy); S = (2 ux uy + c1)(2 vxy + c2) / ((ux ux + uy uy + c1)(vx + vy + c2)), float64 throughout, one IEEE division, no
 * fused multiply-add.  out_f64: double [n_jobs][8] = the element count channels * h * w; the sum of (x - y)^2 over all elements (Y mode:
 * accumulated as int64, so exact as a double up to 2^53); then per channel the sum of S and the window count (h - win + 1)(w - win + 1);
 * channels a mode does not have hold zeros.  Ratios and logarithms are the host's (painter_engine.restoration_metrics).
 * 1 <= win <= 11, finite weights, cov_norm, c1, c2 > 0 and finite, n_jobs 1 .. 1024 (every workgroup walks the table), at most 2^24 tiles
 * (2^32 work-items in the grid);
 * otherwise, for a null pointer (in the table too), a misaligned out_f64 / workspace / float64 picture, or a job with h < win or w < win:
 * hipErrorInvalidValue before anything is enqueued.  workspace: pa_restore_workspace_bytes, 8-byte aligned, as out_f64.  One copy of the
 * table and two launches; no floating-point atomics: a workgroup's partial is summed in a fixed order and a job's partials are added in
 * index order, so two runs give the same bits and a picture's numbers do not depend on which other pictures share the call. */
int pa_restore_scores(const pa_restore_job* jobs, int n_jobs, int mode, int win, const double* weights_f64, double cov_norm, double c1,
                      double c2, void* out_f64, void* workspace, hipStream_t stream);

/* Panoptic quality of panoptic maps against ground-truth annotations, csrc/painter_pq.hip: panopticapi's pq_compute_single_core per
 * picture and the sums of its PQStat over a data set, restated from panopticapi's published source and unverified against panopticapi;
 * tests/painter_pq_host.py is the definition.  A DEVICE job table, one record per picture, pictures of any sizes in one call; the map,
 * its segment table and the segment count may be the ones pa_pano_decode wrote and are read where it left them. */
typedef struct pa_pq_gt_segment {
    int id;              /* r + 256 g + 65536 b of its pixels in the annotation PNG, > 0 */
    int category;        /* index 0 .. n_classes - 1 */
    int iscrowd;
    int area;            /* the annotation's own number; < 0 = count it from the map */
    int rank;            /* position in the annotation's segments_info: of the crowd segments of a category the last one listed counts */
    int reserved;
} pa_pq_gt_segment;
typedef struct pa_pq_job {
    const void* pred;             /* int32 [h][w], 0 = VOID (pa_pano_decode's out_panoptic) */
    const void* gt;               /* int32 [h][w] = r + 256 g + 65536 b of the annotation PNG, or uint8 [h][w][3] (gt_rgb != 0); 0 = VOID */
    const void* pred_segments;    /* pa_pano_segment [p_cap]: id and category_id are read; ascending ids */
    const void* gt_segments;      /* pa_pq_gt_segment [n_gt]; ascending ids */
    const void* pred_count;       /* DEVICE int32 [1]: the number of predicted segments P, clamped to 0 .. p_cap */
    int32_t h, w;                 /* a job with h < 1, w < 1 or h * w > 2^31 counts no pixel */
    int32_t gt_rgb;
    int32_t n_gt;                 /* G, clamped to 0 .. g_cap */
    int32_t g_cap, p_cap;         /* what the job's tables hold; the call's capacities bound both once more */
} pa_pq_job;
/* 1 when a workgroup's private bins, 4 (g_cap + 2)(p_cap + 1) bytes, fit next to the two id maps (8 KB) in the 160 KB of LDS of a CU; 0
 * otherwise and for capacities outside 1 <= g_cap <= 254, 1 <= p_cap <= 255. */
int pa_pq_lds_bins(int g_cap, int p_cap);
/* host only: bytes of pa_pq_add's workspace (a uint32 matrix (g_cap + 2) x (p_cap + 1) per job, 12 bytes per job and g slot, 8 bytes per
 * job and category), -1 for n_jobs outside 1 .. 65535, capacities outside the ranges above or n_classes outside 1 .. 1024. */
int64_t pa_pq_workspace_bytes(int n_jobs, int g_cap, int p_cap, int n_classes);
/* Per job: C[g][p] = pixels with ground-truth row g (0 VOID, 1 .. G listed, G + 1 a non-zero id that is not listed) and predicted column
 * p (0 VOID, 1 .. P listed); parea[p] = sum_g C[g][p]; garea[g] = the annotation's area, or sum_p C[g][p].  For g, p >= 1 with C[g][p] > 0,
 * no crowd flag on g and equal categories: iou = (double)C[g][p] / (double)(parea[p] + garea[g] - C[g][p] - C[0][p]); iou > 0.5 is a match:
 * tp[cat] += 1, iou[cat] += iou.  An unmatched g without crowd flag: fn[cat] += 1.  An unmatched p: fp[cat] += 1 unless (double)(C[0][p] +
 * C[g_c][p]) / (double)parea[p] > 0.5, g_c = the crowd segment of cat[p] with the largest rank (of equal ranks the later entry).
 * acc_tp / acc_fp / acc_fn: int64 [n_classes], acc_iou: float64 [n_classes], 8-byte aligned, ACCUMULATED in place: one set serves a data
 * set.  The float64 additions are made by one thread per category, jobs in table order, matches in ascending g: two runs give the same
 * bits, and so does the host statement.  Integer atomics only.
 * flags_u32: uint32 [n_jobs], written.  A job with a non-zero flag word adds nothing: bit 0 a non-zero predicted id that is not listed (its
 * pixels are not counted), 1 a listed predicted segment without a pixel, 2 a category outside [0, n_classes), 3 union <= 0, 4 a segment
 * matched twice (both only with inconsistent annotation areas), 5 a table whose ids are not ascending from above 0.  With bit 2 or 5 nothing
 * is matched, so bits 3 and 4 stay clear.
 * max_pixels: the largest h * w of the table, 1 .. 2^31 (it sizes the grid only).  bins: 0 = the count kernel's private bins are in LDS
 * whenever pa_pq_lds_bins(g_cap, p_cap), else every run of equal neighbours adds to the job's matrix directly; 1 = the direct form at any
 * capacities (measurements).  workspace: pa_pq_workspace_bytes, 16-byte aligned.  Null pointers, sizes outside the ranges named here or
 * misaligned buffers return hipErrorInvalidValue before anything is enqueued.  Two clears and three launches on `stream`. */
int pa_pq_add(const pa_pq_job* jobs, int n_jobs, int64_t max_pixels, int g_cap, int p_cap, int n_classes, int bins, void* acc_tp_i64,
              void* acc_fp_i64, void* acc_fn_i64, void* acc_iou_f64, void* flags_u32, void* workspace, hipStream_t stream);

/* COCO instance mask AP up to the per-detection match flags, csrc/painter_ap.hip: COCOeval.computeIoU and COCOeval.evaluateImg (iouType
 * "segm") per picture, restated from pycocotools' published source and unverified against pycocotools; tests/painter_ap_host.py is the
 * definition.  A DEVICE job table, one record per picture, pictures of any sizes in one call; the detections' bit masks, scores and count
 * may be the ones pa_inst_decode wrote, their classes the ones pa_pano_decode wrote, and are read where those left them. */
#define PA_AP_AGNOSTIC 1        /* bits of `modes`: useCats = 0, every detection against every ground truth */
#define PA_AP_PER_CLASS 2       /* useCats = 1, a detection against the ground truths of its class */
typedef struct pa_ap_gt {
    int32_t category;    /* index 0 .. n_classes - 1 */
    int32_t iscrowd;
    double area;         /* the annotation's own number, which decides the area ranges; < 0 = the pixel count of the mask */
} pa_ap_gt;
typedef struct pa_ap_job {
    const void* det_masks;      /* uint32 [d_cap][words] in pa_inst_decode's bit layout (pixel p = bit p % 32 of word p / 32), words = ceil(h w / 32) */
    const void* det_scores;     /* float32 [d_cap] */
    const void* det_classes;    /* int32 [d_cap], or NULL: every class is 0 (agnostic only) */
    const void* det_count;      /* DEVICE int32 [1]: the number of detections D, clamped to 0 .. d_cap */
    const void* gt_masks;       /* uint32 [n_gt][words] */
    const void* gt_table;       /* pa_ap_gt [n_gt] */
    int32_t h, w;               /* a job with h < 1, w < 1 or h * w >= 2^31 has neither detections nor ground truths */
    int32_t n_gt;               /* G, clamped to 0 .. the call's g_cap */
    int32_t d_cap;              /* rows the job's detection buffers hold; the call's d_cap bounds it once more */
    int32_t empty_as_one;       /* != 0: with D == 0 the job emits the reference's single empty detection (score 0, area 0, class 0) */
    int32_t reserved;
} pa_ap_job;
typedef struct pa_ap_record {
    float score;
    int32_t area;               /* the pixels of its mask */
    int32_t category;
    int32_t index;              /* its row in the job's detection buffers */
    uint64_t matched[2];        /* [0] agnostic, [1] per class: bit a * n_thrs + t = matched in area range a at threshold t */
    uint64_t ignored[2];        /* likewise: matched to an ignored ground truth, or unmatched with an area outside the range */
} pa_ap_record;
/* host only: bytes of pa_ap_add's workspace (per job a uint32 matrix d_cap x g_cap, 40 bytes per detection slot, 4 per ground-truth slot),
 * -1 for n_jobs outside 1 .. 65535 or capacities outside 1 .. 128. */
int64_t pa_ap_workspace_bytes(int n_jobs, int d_cap, int g_cap);
/* host only: where a section of that workspace starts; which = 0 the intersections uint32 [n_jobs][d_cap][g_cap], 1 the detections' pixel
 * counts uint32 [n_jobs][d_cap], 2 the ground truths' pixel counts uint32 [n_jobs][g_cap], 3 the sorted order int32 [n_jobs][d_cap]
 * (rank -> row), 4 the bit words uint64 [n_jobs][4][d_cap] (matched agnostic, matched per class, ignored agnostic, ignored per class, by
 * rank); -1 for bad arguments. */
int64_t pa_ap_workspace_offset(int n_jobs, int d_cap, int g_cap, int which);
/* Per job: detections in stable order of descending score (ties to the lower row).  I[d][g] = common pixels, area(d) and pixels(g) the
 * pixel counts (padding bits of a last word never count).  iou[d][g] = 0.0 where I = 0, else (double)I / (double)U, U = area(d) for a crowd
 * ground truth, else area(d) + pixels(g) - I.  For every area range a = (lo, hi) of area_ranges_f64 (DEVICE double [n_ranges][2]): a
 * ground truth is ignored when it is crowd or its area (pa_ap_gt.area) is < lo or > hi; the ground truths are walked with the ignored
 * ones last, otherwise in table order.  For every threshold t of iou_thrs_f64 (DEVICE double [n_thrs]) and every detection in order:
 * best = min(t, 1 - 1e-10), m = none; a ground truth already matched at t that is not crowd is skipped; the walk ends when m is a
 * non-ignored one and an ignored one comes up; one with iou < best is skipped; otherwise best = iou, m = it.  With m: matched, ignored =
 * m's flag, m is taken.  Without: ignored = area(d) < lo or > hi.  PA_AP_PER_CLASS does the same among the detections and ground truths
 * of each class.  records: pa_ap_record [n_jobs][d_cap], the first record_counts[j] (int32 [n_jobs], written) of job j are written, in
 * sorted order; cutting to maxDets is the host's (a prefix of the order is matched as it would be alone).
 * flags_u32: uint32 [n_jobs], written.  A job with a non-zero flag word emits nothing: bit 0 a NaN score, 1 a detection class outside
 * [0, n_classes) while PA_AP_PER_CLASS is asked for, 2 a ground-truth class outside that range.
 * max_words: the largest ceil(h w / 32) of the table, 1 .. 2^26 (it sizes the grid only).  1 <= d_cap, g_cap <= 128, n_ranges * n_thrs
 * <= 64, 1 <= n_classes <= 1024, modes 1 .. 3.  workspace: pa_ap_workspace_bytes, 16-byte aligned; the job table, thresholds, ranges and
 * records 8-byte aligned.  Null pointers, sizes outside the ranges named here or misaligned buffers return hipErrorInvalidValue before
 * anything is enqueued.  One clear and three launches on `stream`; integer atomics only, so two runs give the same bytes. */
int pa_ap_add(const pa_ap_job* jobs, int n_jobs, int64_t max_words, int d_cap, int g_cap, int n_classes, int modes, const double* iou_thrs_f64,
              int n_thrs, const double* area_ranges_f64, int n_ranges, pa_ap_record* records, void* record_counts, void* flags_u32,
              void* workspace, hipStream_t stream);

/* COCO keypoint AP up to the per-detection match flags, csrc/painter_kpt.hip: what TopDownCocoDatasetCustom.evaluate
 * (mmpose_custom/data/topdown_coco_dataset.py:194-315) does after the decode -- photo coordinates, rescoring, OKS NMS -- and COCOeval's
 * computeOks and evaluateImg (iouType "keypoints") per photo.  mmpose's oks_iou / oks_nms and xtcocotools' COCOeval are restated from
 * their published source and unverified against mmpose / xtcocotools; tests/painter_kpt_host.py is the definition and states every
 * operation.  Both entry points are stream-ordered, allocate nothing and never synchronise; null, misaligned or out-of-range arguments
 * return hipErrorInvalidValue before anything is enqueued. */
typedef struct pa_kpt_gt {
    double area;              /* the annotation's own number: the OKS denominator and the area ranges */
    double bbox[4];           /* x, y, w, h: the box-distance branch of a ground truth without a labelled keypoint */
    int32_t iscrowd;
    int32_t num_keypoints;    /* 0: ignored */
} pa_kpt_gt;
typedef struct pa_kpt_job {
    const void* rows;         /* int32 [n_box]: rows of the pose table, de-duplicated and in ascending bbox_id */
    const void* gt_keypoints; /* double [n_gt][n_keypoints][3] = x, y, v */
    const void* gt_table;     /* pa_kpt_gt [n_gt] */
    int32_t n_box;            /* D, clamped to 0 .. the call's d_cap */
    int32_t n_gt;             /* G, clamped to 0 .. the call's g_cap */
} pa_kpt_job;
typedef struct pa_kpt_record {
    float score;              /* the rescored score */
    int32_t row;              /* its row in the pose table */
    double area;              /* (max x - min x) * (max y - min y) of its keypoints, float64: loadRes' area */
    uint64_t matched;         /* bit a * n_thrs + t = matched in area range a at threshold t */
    uint64_t ignored;         /* likewise: matched to an ignored ground truth, or unmatched with an area outside the range */
} pa_kpt_record;
/* Per box, chained behind pa_pose_keypoints: preds float32 [n][n_keypoints][2] (8-byte aligned) and maxvals float32 [n][n_keypoints] are
 * read where the decode left them; boxes_f32: DEVICE float32 [n][5] = center x, y, scale x, y (box size / 200), box score.
 * out_poses float32 [n][n_keypoints][3] = (x, y, maxval) with x = float32(((double)p * (full / heat_w) + (double)cx) - full * 0.5), full =
 * (double)sx * 200 (painter_engine.to_image, bit for bit), y likewise; out_scores float32 [n]: the float32 running sum of the maxvals >
 * vis_thr in joint order, one float32 division by their count (0 without any), one float32 multiply by the box score; out_areas float32
 * [n] = float32(sx * 200) * float32(sy * 200).  1 <= n <= 2^24, 1 <= n_keypoints <= 32, heat_w, heat_h >= 1.  One launch, one wave per
 * box. */
int pa_kpt_poses(const float* preds, const float* maxvals, const float* boxes_f32, int n, int n_keypoints, int heat_w, int heat_h,
                 float vis_thr, float* out_poses, float* out_scores, float* out_areas, hipStream_t stream);
/* host only: bytes of pa_kpt_evaluate's workspace (8 bytes per job and box slot, 8 per job, evaluated detection and ground-truth slot), -1
 * for n_jobs outside 1 .. 65535, d_cap outside 1 .. 1024, g_cap outside 1 .. 128 or max_det outside 1 .. 64. */
int64_t pa_kpt_workspace_bytes(int n_jobs, int d_cap, int g_cap, int max_det);
/* host only: where a section of that workspace starts; which = 0 the NMS order int32 [n_jobs][d_cap] (rank -> position in the job's
 * rows), 1 the survivor flags int32 [n_jobs][d_cap] by rank, 2 the evaluation OKS doubles [n_jobs][max_det][g_cap]; only the entries of a
 * job's own boxes / evaluated detections and ground truths are written.  -1 for bad arguments. */
int64_t pa_kpt_workspace_offset(int n_jobs, int d_cap, int g_cap, int max_det, int which);
/* One workgroup per job (photo) over a DEVICE job table; poses / scores / areas: the pose table pa_kpt_poses wrote, n_rows rows.  Per job:
 * the boxes in descending score, equal scores to the higher position (argsort(kind="stable")[::-1]); greedy OKS NMS: a surviving box i
 * suppresses a later box j when float32(oks) > oks_thr, oks = (sum_k exp(-e_k)) / K over all K keypoints in ascending k, e_k =
 * (double)d2_k / (2 sigma_k)^2 / den / 2, d2_k = dx^2 + dy^2 in float32, den = (double)float32((a_i + a_j) / 2) + 2^-52.  oks_thr < 0: no
 * NMS, the order is descending score with equal scores to the LOWER position.  The first max_det survivors are evaluated in that order:
 * area = (max x - min x)(max y - min y) of its keypoints; against ground truth g with k1 = #(v > 0): k1 > 0: e_k = (dx^2 + dy^2) / (2
 * sigma_k)^2 / (area_g + 2^-52) / 2 over the keypoints with v > 0, oks = sum exp(-e_k) / k1; k1 == 0: dx = max(0, x0 - xd) + max(0, xd -
 * x1) with x0 = bx - bw, x1 = bx + 2 bw (y likewise) over all K, divided by K; float64 throughout, no fused multiply-add.  A ground truth
 * is ignored when iscrowd or num_keypoints == 0, per area range (area_ranges_f64, DEVICE double [n_ranges][2]) also when its area is < lo
 * or > hi.  Matching per range and threshold (iou_thrs_f64, DEVICE double [n_thrs]) is pa_ap_add's: best = min(t, 1 - 1e-10), ignored
 * ground truths last, a matched ground truth stays open only when it is crowd, an unmatched detection is ignored when its area is outside
 * the range.  records: pa_kpt_record [n_jobs][max_det], the first record_counts[j] of job j written; survivor_counts[j]: how many boxes
 * the NMS kept (both int32 [n_jobs], written).  flags_u32: uint32 [n_jobs], written; a job with a non-zero word emits nothing: bit 0 a NaN
 * among its poses, scores or areas, 1 a ground truth whose area + 2^-52 is not a positive finite number, 2 a row outside the pose table.
 * 1 <= d_cap <= 1024, 1 <= g_cap <= 128, 1 <= n_keypoints <= 32 (sigmas_f64: DEVICE double [n_keypoints]), n_ranges * n_thrs <= 64, 1 <=
 * max_det <= 64, 1 <= n_jobs <= 65535, 1 <= n_rows <= 2^24.  workspace: pa_kpt_workspace_bytes, 16-byte aligned; tables of doubles and
 * records 8-byte aligned.  One launch; no floating-point atomics, so two runs give the same bytes. */
int pa_kpt_evaluate(const pa_kpt_job* jobs, int n_jobs, const float* poses, const float* scores, const float* areas, int n_rows, int d_cap,
                    int g_cap, int n_keypoints, const double* sigmas_f64, float oks_thr, int max_det, const double* iou_thrs_f64, int n_thrs,
                    const double* area_ranges_f64, int n_ranges, pa_kpt_record* records, void* record_counts, void* survivor_counts,
                    void* flags_u32, void* workspace, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PAINTER_HIP_H */
