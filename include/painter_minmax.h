/* painter_minmax.h -- C ABI of libpainter_hip.so, fourth header: instance decode by nearest colour on the MI355X (gfx950),
 * csrc/painter_minmax.hip.  The conventions are those of painter_hip.h: plain DEVICE pointers + sizes, every function only ENQUEUES work
 * on `stream`, allocates nothing and returns a hipError_t as int (0 = success), *_workspace_bytes() are host-only helpers (-1 for bad
 * arguments).  PA_ABI_VERSION stays 9: these entry points are purely additive.
 *
 * The route is COCOEvaluatorCustom.post_process_segm_output_by_minmax (Painter/eval/coco_panoptic/COCOCAInstSegEvaluatorCustom.py:172-250),
 * the evaluator's `post_type="minmax"`, restated on integers; tests/painter_minmax_host.py is the definition:
 *   image   uint8 [h][w][3]; palette float32 [K][3] of integer values 0..255, K = n_colours, its LAST row is the background;
 *   L1(p, c) = sum over the channels of |p_ch - c_ch|, an integer 0..765;
 *   label(p) = the LOWEST c that attains min_c L1(p, c); dist(p) = that minimum;
 *   n_c = number of pixels with label c (32 bits), S_c = sum of their dist (64 bits);
 *   the instances are the colours with n_c > 0 in ascending c (torch.unique's order); instance i is "slot" i;
 *   neg_c = (float)((double)S_c / (double)n_c); m = max(max_c neg_c, 1.0f); score_c = 1.0f - neg_c / m (one float32 division, one float32
 *   subtraction); class = c == K - 1 ? 0 : 1.
 * There is no NMS, no top-k and no truncation: up to K instances come out.  Only integer atomics are used, so two runs give the same bytes.
 * Capacities: 1 <= h, w <= 16384, h * w <= 2^24, 1 <= n_colours <= 16384.  Null pointers, sizes beyond a capacity or a misaligned buffer
 * return hipErrorInvalidValue before anything is launched. */
#ifndef PAINTER_MINMAX_H
#define PAINTER_MINMAX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

/* One per instance, 32 bytes, 8-byte aligned; records >= count are not written. */
typedef struct pa_minmax_record {
    int32_t colour;     /* the palette row */
    int32_t cls;        /* 0 for the background row K - 1, otherwise 1 */
    uint32_t n;         /* pixels */
    uint32_t reserved;  /* written as 0 */
    uint64_t S;         /* sum of their distances */
    float neg;          /* (float)((double)S / (double)n) */
    float score;        /* 1.0f - neg / max(largest neg, 1.0f) */
} pa_minmax_record;

/* image -> out_label uint16 [h * w] and out_dist uint16 [h * w] (2-byte aligned).  The palette is packed to one dword per colour in LDS;
 * a thread keeps its pixel as a packed dword, one broadcast LDS read brings four colours; the running minimum is one unsigned minimum
 * over the key (L1 << 16) + c, so the lowest index wins a tie.  One launch. */
int pa_minmax_nearest(const void* image, const void* palette, int h, int w, int n_colours, void* out_label, void* out_dist,
                      hipStream_t stream);

/* host only: bytes of pa_minmax_decode's workspace = 8 * n_colours (S) + 4 * n_colours (n), each rounded up to 16.  -1 for h, w,
 * n_colours < 1 or beyond a capacity. */
int64_t pa_minmax_workspace_bytes(int h, int w, int n_colours);

/* pa_minmax_nearest, then the statistics (runs of equal labels folded in the wave, private bins in LDS, integer atomics), then one
 * workgroup that compacts: out_count int32 [1] = the number of instances; out_records pa_minmax_record [n_colours] (8-byte aligned), the
 * first `count` written in ascending colour; out_slot int32 [n_colours], colour -> slot, -1 for a colour without a pixel.  workspace:
 * pa_minmax_workspace_bytes, 16-byte aligned; it holds S uint64 [n_colours] at byte 0 and n uint32 [n_colours] behind it afterwards.
 * A clear and three launches. */
int pa_minmax_decode(const void* image, const void* palette, int h, int w, int n_colours, void* workspace, void* out_label, void* out_dist,
                     void* out_count, void* out_records, void* out_slot, hipStream_t stream);

/* The masks of slots [first, first + n_cap) from the label map and the slot table of pa_minmax_decode: out_bits uint32
 * [n_cap][ceil(h * w / 32)] in pa_inst_decode's bit layout (pixel p = y * w + x is bit p % 32 of word p / 32, padding bits 0; 4-byte
 * aligned) and, unless out_bytes is null, the same masks as uint8 [n_cap][h * w] of 0 / 1.  Both are cleared first; the masks partition
 * the picture, so the thread of a 32-pixel word writes at most 32 words and nothing else touches them.  first >= 0, 1 <= n_cap <= 16384;
 * slots that no colour has stay empty.  The clears and one launch. */
int pa_minmax_masks(const void* label, const void* slot, int h, int w, int n_colours, int first, int n_cap, void* out_bits, void* out_bytes,
                    hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
