/* painter_anysize_grad.h -- C ABI of libpainter_hip.so, sixth header: the BACKWARD at a run-time input size other than the constructed one on
 * the MI355X (gfx950), csrc/attn_any_bwd.hip.  The conventions are those of painter_hip.h: plain DEVICE pointers + sizes, every function
 * only ENQUEUES work on `stream`, allocates nothing and returns a hipError_t as int (0 = success).  PA_ABI_VERSION stays 9: these entry
 * points are purely additive; pa_attn_bwd keeps its contract, its refusals included, and painter_anysize.h keeps its three symbols.
 *
 * The reference is size-agnostic under autograd too: gradients flow through get_rel_pos's F.interpolate(mode="linear") into the stored
 * rel-pos tables (util/vitdet_utils.py:63-93).  pa_attn_any_bwd gives the table gradient at the run-time lengths, pa_relpos_resize_bwd
 * carries it back to the stored ones. */
#ifndef PAINTER_ANYSIZE_GRAD_H
#define PAINTER_ANYSIZE_GRAD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

/* host only: bytes of pa_attn_any_bwd's workspace (Delta, the transposed bias tables the dK/dV kernel reads, the per-query bias gradients
 * dG, the split-K slabs of the table contraction; every section starts on 256 bytes; the workspace itself on 16).  0 for arguments
 * pa_attn_any_bwd refuses. */
int64_t pa_attn_any_bwd_workspace_bytes(int dtype, int batch, int L, int heads, int Hp, int Wp, int head_dim);

/* Fused attention backward for ANY token grid Hp, Wp >= 1 (L = Hp * Wp), head_dim 64 or 80, dtype PA_F32 (0) / PA_BF16 (1; MFMA).
 * Operands as pa_attn_any_fwd / pa_attn_bwd: qkv [batch, L, 3, heads, head_dim] T at row pitch ldq (elements; 16-byte aligned rows), rcat T
 * [NRP, head_dim] and rcatT T [head_dim, NRP] (NRP = pa_relpos_rows_padded(Hp, Wp)) packed for the RUN-TIME grid, out and dout
 * [batch * L, heads * head_dim] T at row pitches ldo / lddo, lse f32 [batch * heads, L] as pa_attn_any_fwd wrote it.
 * Results: dqkv T in qkv's layout at qkv's pitch ldq (the three head_dim-wide fields of every head of every row; nothing between or behind
 * them), and -- unless drcat is NULL (frozen tables: the contraction is not launched) -- drcat f32 [NRP, head_dim] =
 * [d rel_pos_h (2Hp - 1 rows) ; d rel_pos_w (2Wp - 1 rows) ; zeros] for the run-time grid.
 *   - a key's (row, column) is kept per key, in the bias read and in the scatter of dS into the per-query (kh | kw) gradient tables;
 *   - keys >= L of the last 32-key tile get weight exactly 0 and dS exactly 0; their K and V rows are ZEROED WHILE STAGED, never read;
 *   - query rows >= L of the last 32-row tile: the dK/dV kernel stages zeros for their Q and dO rows and forces their P and dS to 0; the
 *     dQ kernel neither loads nor stores them, and they enter neither dG nor the table gradient;
 *   - no floating-point atomics anywhere: the same input gives the same bits.
 * Five launches (Delta, dQ + dG, dK/dV, the table contraction and its slab sum), three with drcat == NULL.
 * hipErrorInvalidValue BEFORE ANY LAUNCH for a null pointer, L != Hp * Wp, sizes < 1, another head_dim, a misaligned pitch or pointer, or
 * a grid whose tables do not fit LDS.  With TS = (Hp + Wp + 3) | 1, TG = (Hp + Wp) | 1 and e = sizeof(T) the limits are
 *     Hp + Wp <= 126                                                    (the dK/dV kernel's table tile), and
 *     2 * stage + NW * max(128 * (TS + TG), 32 * head_dim * e) <= 160 KiB  (the dQ kernel), NW = 4, 3 or -- head_dim 64 only -- 2 waves,
 *     stage = 96 * head_dim * e for head_dim 64 and 32 * (2 * (80 * e + 16) + 96 * e) for head_dim 80.
 * 70 x 35 tokens (Hp + Wp = 105) is accepted at both head dims and both dtypes. */
int pa_attn_any_bwd(int dtype, const void* qkv, int64_t ldq, const void* rcat, const void* rcatT, const void* out, int64_t ldo,
                    const void* dout, int64_t lddo, const float* lse, void* dqkv, float* drcat, void* workspace, int batch, int L, int heads,
                    int Hp, int Wp, int head_dim, float scale, hipStream_t stream);

/* host only: the number of accepted pa_attn_any_bwd calls since process start (pa_attn_launch_counts and pa_attn_any_launches are untouched). */
int64_t pa_attn_any_bwd_launches(void);

/* The adjoint of pa_relpos_resize for ONE block, fp32: the table gradient at the run-time lengths carried back to the stored lengths,
 *     d t[i][d] = sum_j w(j, i) * d out[j][d],   w(j, i) = (1 - lambda_j) [i == i0_j] + lambda_j [i == i1_j]
 * with exactly pa_relpos_resize's i0, i1, lambda per j.  Gather form: one thread per stored element adds its contributions in ascending
 * j (per j the i0 term before the i1 term) -- no atomics, the same input gives the same bits.  A length that stays is copied bit for bit.
 * drcat: f32 [>= dst_h + dst_w, head_dim], d rel_pos_h rows then d rel_pos_w rows (pa_attn_any_bwd's result).
 * dtab:  f32 [out_rows, head_dim], out_rows >= src_h + src_w: d rel_pos_h at the stored length, d rel_pos_w behind it, zero rows behind
 * that (a block's flat gradient buffer keeps pa_relpos_rows_padded rows).  Written completely.  One launch. */
int pa_relpos_resize_bwd(const float* drcat, float* dtab, int out_rows, int src_h, int src_w, int dst_h, int dst_w, int head_dim,
                         hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
