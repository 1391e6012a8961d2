/* painter_anysize.h -- C ABI of libpainter_hip.so, fifth header: the forward at a run-time input size other than the constructed one on
 * the MI355X (gfx950), csrc/attn_any.hip.  The conventions are those of painter_hip.h: plain DEVICE pointers + sizes, every function only
 * ENQUEUES work on `stream`, allocates nothing and returns a hipError_t as int (0 = success).  PA_ABI_VERSION stays 9: these entry points
 * are purely additive, and pa_attn_fwd keeps its contract, its refusals included.
 *
 * The reference runs at any input size (util/vitdet_utils.py:63-93: get_rel_pos resizes a block's rel-pos tables with
 * F.interpolate(mode="linear") whenever 2 * max(q, k) - 1 differs from the stored length); the token grid Hp x Wp of such a run need not
 * be a multiple of anything (COCO panoptic at 1120 x 560: 70 x 35 tokens, L = 2450). */
#ifndef PAINTER_ANYSIZE_H
#define PAINTER_ANYSIZE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

/* Fused attention forward for ANY token grid Hp, Wp >= 1 (L = Hp * Wp), head_dim 64 or 80, dtype PA_F32 (0) / PA_BF16 (1), forward only.
 * Operands as pa_attn_fwd: qkv [batch, L, 3, heads, head_dim] T at row pitch ldq (elements; 16-byte aligned rows), rcat T
 * [pa_relpos_rows_padded(Hp, Wp), head_dim] from pa_relpos_pack / pa_relpos_pack_batch, out [batch * L, heads * head_dim] T at row pitch
 * ldo, lse f32 [batch * heads, L].  Both are written completely and nothing else is.
 *   - a key's (row, column) is kept per key: runs of keys cross key rows;
 *   - keys >= L of the last 32-key tile get weight exactly 0, and their K and V rows are ZEROED WHILE STAGED (in a batch they are the next
 *     sample's first tokens, behind the last sample they are not the caller's memory): nothing of them is read;
 *   - query rows >= L of the last 32-row tile are neither loaded nor stored.
 * One launch.  hipErrorInvalidValue for a null pointer, L != Hp * Wp, sizes < 1, another head_dim, a misaligned pitch, or a grid whose
 * bias tables do not fit LDS (32 * ((Hp + Wp + 3) | 1) * 4 bytes per wave, 4 waves). */
int pa_attn_any_fwd(int dtype, const void* qkv, int64_t ldq, const void* rcat, void* out, int64_t ldo, float* lse, int batch, int L,
                    int heads, int Hp, int Wp, int head_dim, float scale, hipStream_t stream);

/* host only: the number of pa_attn_any_fwd launches since process start (tests assert with it which route a model took; the counters of
 * pa_attn_launch_counts are untouched by this header). */
int64_t pa_attn_any_launches(void);

/* Every block's rel-pos tables resized in one launch, fp32, the rule of F.interpolate(mode="linear", align_corners=False) along the
 * table's length, per column d:  s = max((n_src / n_dst) * (j + 0.5) - 0.5, 0), i0 = min(floor(s), n_src - 1), i1 = min(i0 + 1, n_src - 1),
 * out[j][d] = (1 - (s - i0)) * t[i0][d] + (s - i0) * t[i1][d].
 * src_tabs: device array of 2 * nblocks pointers -- rel_pos_h [src_h, head_dim] of every block, then rel_pos_w [src_w, head_dim] of every
 * block (the array pa_relpos_pack_batch takes).  dst: f32 [nblocks][dst_h + dst_w][head_dim]: block b's resized rel_pos_h, its resized
 * rel_pos_w right behind it -- pa_relpos_pack_batch then packs them for the run-time grid through a second pointer array.  A length that
 * stays (n_src == n_dst) is copied bit for bit.  1 <= nblocks <= 65535, every length >= 1, head_dim >= 1. */
int pa_relpos_resize(const void* src_tabs, void* dst, int nblocks, int src_h, int src_w, int dst_h, int dst_w, int head_dim,
                     hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
