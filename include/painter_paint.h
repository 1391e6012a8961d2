/* painter_paint.h -- C ABI of libpainter_hip.so, third header: painting task TARGETS from annotations on the MI355X (gfx950),
 * csrc/painter_paint.hip -- the direction opposite to the decoders of painter_hip.h.  The conventions are those of painter_hip.h: plain
 * DEVICE pointers + sizes, every function only ENQUEUES work on `stream` and returns a hipError_t as int (0 = success),
 * *_workspace_bytes() are host-only helpers (-1 for bad arguments).  PA_ABI_VERSION stays 9: these entry points are purely additive.
 *
 * tests/painter_paint_host.py is the definition; the pictures equal the reference's offline generators byte for byte
 * (tests/golden/make_golden_painter_paint.py).  Pictures are uint8 [h][w][3], contiguous, 16-byte aligned.  Every atomic is an integer
 * add, so the output is a pure function of the input and two runs give the same bytes.
 * Capacities: h, w >= 1, h * w < 2^31; semantic palette 1 .. 1024 colours, 0 .. 1024 segments per picture, 1 .. 65535 jobs; instance
 * targets 0 .. 4096 masks (PA_PAINT_MAX_MASKS) over a palette of exactly 6400 cells; pose 1 .. 65535 boxes of 1 .. 32 joints
 * (PA_PAINT_MAX_JOINTS), a distance table of 1 .. 1024 entries.  Null pointers, sizes beyond a capacity or a misaligned buffer return
 * hipErrorInvalidValue before anything is launched. */
#ifndef PAINTER_PAINT_H
#define PAINTER_PAINT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

#define PA_PAINT_MAX_COLOURS 1024
#define PA_PAINT_MAX_SEGMENTS 1024
#define PA_PAINT_MAX_MASKS 4096
#define PA_PAINT_CELLS 6400
#define PA_PAINT_MAX_JOINTS 32
#define PA_PAINT_MAX_TABLE 1024

/* kinds of a semantic job's source */
#define PA_PAINT_LABELS_U8 0    /* uint8 [h][w] labels: 0 paints black, l paints palette[l - 1] */
#define PA_PAINT_LABELS_I32 1   /* int32 [h][w] labels: l <= 0 paints black */
#define PA_PAINT_IDS_I32 2      /* int32 [h][w] segment ids, looked up in the job's table */
#define PA_PAINT_IDS_RGB 3      /* uint8 [h][w][3] annotation PNG: id = r + 256 g + 65536 b, looked up in the job's table */

/* One picture of pa_paint_semantic, 40 bytes, 8-byte aligned. */
typedef struct pa_paint_job {
    const void* src;      /* by `kind`; int32 sources 4-byte aligned */
    void* dst;            /* uint8 [h][w][3]; dword stores where it is 4-byte aligned, byte stores otherwise */
    const void* table;    /* kinds 2, 3: int32 [n_table][2] = (segment id, colour index); a later row wins over an earlier one with the
                             same id; ids in no row paint black; colour indices outside the palette paint black.  kinds 0, 1: unused */
    int32_t h, w;
    int32_t kind;
    int32_t n_table;      /* 0 .. PA_PAINT_MAX_SEGMENTS */
} pa_paint_job;

/* jobs: DEVICE pa_paint_job [n_jobs]; max_pixels: the largest h * w of the table, as the host knows it (a job with more pixels is painted
 * up to max_pixels only: the host states what it put in the table); palette_u8: uint8 [n_colours][3]; out_bad: int32 [n_jobs], cleared
 * first, per job the number of pixels whose label lies above n_colours -- they paint black (the reference raises IndexError).  One launch
 * behind the clear: the palette and the job's table sit in LDS, a thread paints 4 pixels and stores 3 dwords. */
int pa_paint_semantic(const void* jobs, int n_jobs, int64_t max_pixels, const void* palette_u8, int n_colours, void* out_bad,
                      hipStream_t stream);

/* host only: 24 * max(n, 1) bytes (per mask the int64 sums n, sum x, sum y) + 4 * max(n, 1) (its colour), each rounded up to 16.  -1 for
 * n < 0 or n > PA_PAINT_MAX_MASKS. */
int64_t pa_paint_instances_workspace_bytes(int n);
/* masks_u32: uint32 [n][ceil(h * w / 32)] in pa_inst_decode's bit layout (pixel p = y * w + x is bit p % 32 of word p / 32); the padding
 * bits of the last word may hold anything and no slot >= n is read.  palette_u8: uint8 [6400][3] in location_palette()'s order.
 * cells_in: null (the mass centre: per mask the integers n, sum x, sum y, then norm = n or 1e-6, cx = double(sum x) / norm,
 * ax = (int)(cx / w * 79), ay likewise with h) or int32 [n][2] = (ax, ay) computed by the caller (geo_center), each 0 .. 79.
 * Outputs: out_picture uint8 [h][w][3], 16-byte aligned, every byte written; out_cells int32 [n][2]; out_empty int32 [1]: 1 when no
 * painted byte is non-zero (the reference's "pure black label", not saved).  Where masks overlap the highest index wins.  Workspace:
 * pa_paint_instances_workspace_bytes, 16-byte aligned.  Three launches behind a clear (two with cells_in): sums, colours, paint. */
int pa_paint_instances(const void* masks_u32, int n, int h, int w, const void* palette_u8, const void* cells_in, void* workspace,
                       void* out_picture, void* out_cells, void* out_empty, hipStream_t stream);

/* rects: int32 [n_boxes][2][n_joints][4] = (ul_x, ul_y, br_x, br_y) of mmpose's MSRA target, set [0] for the class sigma (G, B), set [1]
 * for the kernel sigma (R); the painted rectangle is [ul, br) clipped to the picture, a joint that paints nothing has br_x <= ul_x.
 * c_kernel: the patch centre, size // 2, of the kernel sigma; colours_u8: uint8 [n_joints][2] = (G, B); table_u8: uint8
 * [table_len], R by d^2 = (x - ul_x - c_kernel)^2 + (y - ul_y - c_kernel)^2, strictly decreasing before its rounding to bytes (indices beyond the
 * table read its last entry).  R = table[min d^2] over the kernel rectangles that hold the pixel, 0 without one; (G, B) = black without
 * a class rectangle, the joint's colour with exactly one, and with several the colour of the kernel rectangle of the smallest d^2
 * (lowest joint among equals; joint 0 when no kernel rectangle holds the pixel).  out: uint8 [n_boxes][h][w][3], 4-byte aligned.
 * One launch, integers only. */
int pa_paint_pose(const void* rects, int n_boxes, int n_joints, int h, int w, int c_kernel, const void* colours_u8,
                  const void* table_u8, int table_len, void* out, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
