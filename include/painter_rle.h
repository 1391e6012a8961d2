/* painter_rle.h -- C ABI of libpainter_hip.so, second header: COCO run-length encoding of bit masks on the MI355X (gfx950) and its
 * inverse, csrc/painter_rle.hip.  The conventions are those of painter_hip.h: plain DEVICE pointers + sizes, every function only
 * ENQUEUES work on `stream` and returns a hipError_t as int (0 = success), *_workspace_bytes() are host-only helpers (-1 for bad
 * arguments).  PA_ABI_VERSION stays 9: these entry points are purely additive.
 *
 * The format is the one of pycocotools' published common/maskApi.c (rleEncode, rleToString, rleFrString, rleArea, rleToBbox), restated
 * in tests/painter_rle_host.py -- the definition -- and unverified against pycocotools itself:
 *   - pixels are walked column-major, j = x * h + y; `counts` are the lengths of alternating runs, starting with a run of zeros (the
 *     first count is 0 when pixel 0 is set); m = transitions + 1 with v(-1) = 0; the bottom pixel of column x and the top pixel of column
 *     x + 1 are neighbours;
 *   - string: for count i, x = cnts[i] - (i > 2 ? cnts[i - 2] : 0) (signed) leaves as groups of 5 bits, lowest first, c = x & 0x1f,
 *     x >>= 5 (arithmetic), more = (c & 0x10) ? x != -1 : x != 0, c |= 0x20 if more, character c + 48: at most 7 characters per count;
 *   - area = sum of the odd counts; bbox = x, y, w, h of the set pixels, zeros for an empty mask.
 * Masks are bit masks in pa_inst_decode's layout: uint32 [n][words], words = ceil(h * w / 32), pixel p = y * w + x is bit p % 32 of word
 * p / 32; rows are not word aligned.  Everything is integer arithmetic without floating point; the atomics are integer OR / min / max /
 * add, so the output is a pure function of the input bits and two runs give the same bytes.
 * Capacities: h, w >= 1, h * w < 2^31, 1 <= n_cap (n) <= 65535.  Null pointers, sizes beyond a capacity or a misaligned buffer return
 * hipErrorInvalidValue before anything is launched. */
#ifndef PAINTER_RLE_H
#define PAINTER_RLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

/* pa_rle_encode's header, int64 [4], 8-byte aligned. */
typedef struct pa_rle_header {
    int64_t runs;       /* sum of the masks' run counts */
    int64_t chars;      /* sum of the masks' string lengths: exact, whether or not the pool could hold them */
    int64_t overflow;   /* 1: chars > char_cap, the pool was not written */
    int64_t count;      /* the device count as it was used (clamped to 0 .. n_cap) */
} pa_rle_header;
/* One per mask slot, 40 bytes, 8-byte aligned; slots >= count are not written. */
typedef struct pa_rle_record {
    int64_t char_offset;    /* of the mask's string in the pool: the exclusive sum of char_count over the masks before it */
    int64_t char_count;
    uint32_t runs;          /* m of maskApi.c, transitions + 1 */
    uint32_t area;
    int32_t bbox[4];        /* x, y, w, h */
} pa_rle_record;

/* host only: bytes of pa_rle_encode's workspace = 48 * n_cap * w (per column: transition count, set pixels, row extent, the three
 * transitions before it, its base in the mask's runs, its characters, its base in the mask's string) + 20 * n_cap, every section rounded
 * up to 16.  -1 for h, w, n_cap < 1, h * w >= 2^31, n_cap > 65535. */
int64_t pa_rle_encode_workspace_bytes(int h, int w, int n_cap);
/* masks_u32: uint32 [n_cap][ceil(h * w / 32)]; count: DEVICE int32 [1], read where pa_inst_decode / pa_pano_decode left it (clamped to
 * 0 .. n_cap), slots >= count are never read; workspace: pa_rle_encode_workspace_bytes, 16-byte aligned.  Outputs: out_header
 * (pa_rle_header, 8-byte aligned); out_records (pa_rle_record [n_cap], 8-byte aligned); out_pool uint8 [char_cap], the strings of
 * masks 0 .. count - 1 one after the other without terminators.  There is no pool of runs: a column's thread knows the three transitions
 * before its column (a scan over the columns carries them), so characters are counted and then written straight from the bits, and
 * char_cap (>= 0) is the one capacity.  When the strings do not fit, header.overflow = 1, header and records are complete and exact and
 * not one byte of the pool is written; the caller launches again with char_cap >= header.chars.  Six launches. */
int pa_rle_encode(const void* masks_u32, const void* count, int h, int w, int n_cap, void* workspace, int64_t char_cap, void* out_header,
                  void* out_records, void* out_pool, hipStream_t stream);

/* host only: bytes of pa_rle_decode's workspace = 8 * run_cap (a value, then the end position of a run, per input element) + 4 * n,
 * rounded up to 16.  -1 for h, w, n < 1, h * w >= 2^31, n > 65535, run_cap < 0. */
int64_t pa_rle_decode_workspace_bytes(int n, int h, int w, int64_t run_cap);
/* The inverse.  pool: compressed != 0: uint8 [pool_len], the characters of the strings; compressed == 0: uint32 [pool_len], uncompressed
 * counts (COCO's crowd annotations), 4-byte aligned.  spans: DEVICE int64 [n][2] = (offset, length) of mask i in the pool, in elements,
 * 8-byte aligned.  Mask i uses workspace elements [offset, offset + length): run_cap >= pool_len holds every mask.  workspace:
 * pa_rle_decode_workspace_bytes, 16-byte aligned.  out_bits: uint32 [n][ceil(h * w / 32)], cleared first, padding bits stay 0;
 * out_flags: int32 [n].  A malformed mask is refused: its bits stay zero and its flag says why; whatever the bytes are, nothing outside
 * the mask's own words is written and nothing outside its own span is read.  Checks in this order, the first that fails is the flag:
 *   6  the span does not lie inside the pool
 *   5  more runs than the workspace was sized for (offset + length > run_cap), or 2^27 or more input elements
 *   7  a byte outside '0' .. 'o' (48 .. 111)
 *   4  a value has more than 7 groups
 *   3  the string ends inside a value
 *   2  a count is negative after the delta (x += cnts[i - 2] for i > 2)
 *   1  the counts do not sum to h * w (the empty string included)
 * Zero counts inside a string are legal, as they are for maskApi.c.  Two launches behind the clear. */
int pa_rle_decode(const void* pool, int compressed, const void* spans, int n, int h, int w, int64_t pool_len, int64_t run_cap,
                  void* workspace, void* out_bits, void* out_flags, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
