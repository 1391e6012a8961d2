// Painting task targets from annotations (include/painter_paint.h; tests/painter_paint_host.py is the definition).
//
//   paint_semantic_kernel   one workgroup per 1024 pixels of a job: palette (and the job's id -> colour table) in LDS, a thread paints 4
//                           pixels = 3 dwords; labels above the palette are counted per job with one integer atomic per thread that met one
//   inst_sums_kernel        one thread per 32-pixel word of a mask: n = popcount, sum of pixel indices = n * p0 + (five masked
//                           popcounts), sum y by splitting the word at its row boundaries, sum x = sum p - w * sum y; reduced in the
//                           wave, then one 64-bit integer atomic add per wave and sum
//   inst_colour_kernel      one thread per mask: the reference's three float64 operations per axis -> cell -> palette row
//   inst_paint_kernel       one thread per 32-pixel word: walks the masks from the last to the first until every bit is owned, colours of
//                           all masks in LDS, 96 bytes leave as six 16-byte stores
//   pose_paint_kernel       one workgroup per 1024 pixels of a box: rectangles, colours and the d^2 -> R table in LDS, integers only
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/painter_paint.h"
#include "common.h"

namespace {

constexpr int TPB = 256;
constexpr int PPT = 4;                                     // pixels per thread of the semantic and pose kernels
constexpr int MAX_JOBS = 65535;

bool shape_ok(int h, int w) { return h >= 1 && w >= 1 && (int64_t)h * w < ((int64_t)1 << 31); }

// 4 pixels (r | g << 8 | b << 16 each) at pixel p of a picture of npix pixels: 3 dwords where the group is whole and `aligned`
DEVI void store_pixels(uint8_t* __restrict__ dst, uint32_t p, uint32_t npix, const uint32_t (&c)[PPT], bool aligned) {
    if (aligned && p + PPT <= npix) {
        uint32_t* d = (uint32_t*)(dst + (size_t)p * 3);
        d[0] = (c[0] & 0xffffffu) | (c[1] << 24);
        d[1] = ((c[1] >> 8) & 0xffffu) | (c[2] << 16);
        d[2] = ((c[2] >> 16) & 0xffu) | (c[3] << 8);
    } else {
#pragma unroll
        for (int i = 0; i < PPT; ++i)
            if (p + i < npix) {
                uint8_t* d = dst + (size_t)(p + i) * 3;
                d[0] = (uint8_t)c[i]; d[1] = (uint8_t)(c[i] >> 8); d[2] = (uint8_t)(c[i] >> 16);
            }
    }
}

// ---- semantic
__global__ __launch_bounds__(TPB) void paint_semantic_kernel(const pa_paint_job* __restrict__ jobs, int64_t max_pixels,
                                                            const uint8_t* __restrict__ palette, int n_colours, int* __restrict__ bad) {
    __shared__ uint32_t s_pal[PA_PAINT_MAX_COLOURS];
    __shared__ int s_id[PA_PAINT_MAX_SEGMENTS], s_colour[PA_PAINT_MAX_SEGMENTS];
    const pa_paint_job jb = jobs[blockIdx.y];
    const int64_t npix64 = min((int64_t)jb.h * jb.w, max_pixels);
    if (jb.h < 1 || jb.w < 1 || (int64_t)blockIdx.x * (TPB * PPT) >= npix64) return;               // uniform
    const uint32_t npix = (uint32_t)npix64;
    const int t = threadIdx.x;
    const bool ids = jb.kind == PA_PAINT_IDS_I32 || jb.kind == PA_PAINT_IDS_RGB;
    const int n_table = ids ? clampi(jb.n_table, 0, PA_PAINT_MAX_SEGMENTS) : 0;
    for (int i = t; i < n_colours; i += TPB)
        s_pal[i] = (uint32_t)palette[3 * i] | ((uint32_t)palette[3 * i + 1] << 8) | ((uint32_t)palette[3 * i + 2] << 16);
    for (int i = t; i < n_table; i += TPB) {
        s_id[i] = ((const int*)jb.table)[2 * i];
        s_colour[i] = ((const int*)jb.table)[2 * i + 1];
    }
    __syncthreads();
    const uint32_t p = (blockIdx.x * TPB + t) * PPT;
    if (p >= npix) return;
    uint32_t c[PPT];
    int n_bad = 0, last_id = 0, last_colour = -1;
    bool have_last = false;
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
        c[i] = 0;
        if (p + i >= npix) continue;
        const size_t q = (size_t)p + i;
        int colour = -1;                                     // palette row, -1 = black
        if (!ids) {
            const int label = jb.kind == PA_PAINT_LABELS_U8 ? (int)((const uint8_t*)jb.src)[q] : ((const int*)jb.src)[q];
            if (label > n_colours) ++n_bad;
            else if (label > 0) colour = label - 1;
        } else {
            int id;
            if (jb.kind == PA_PAINT_IDS_I32) id = ((const int*)jb.src)[q];
            else {
                const uint8_t* s = (const uint8_t*)jb.src + 3 * q;
                id = (int)s[0] | ((int)s[1] << 8) | ((int)s[2] << 16);
            }
            if (have_last && id == last_id) colour = last_colour;
            else {
                for (int k = n_table - 1; k >= 0; --k)       // a later row wins
                    if (s_id[k] == id) { colour = s_colour[k]; break; }
                have_last = true; last_id = id; last_colour = colour;
            }
            if (colour >= n_colours) colour = -1;
        }
        if (colour >= 0) c[i] = s_pal[colour];
    }
    store_pixels((uint8_t*)jb.dst, p, npix, c, ((uintptr_t)jb.dst & 3) == 0);
    if (n_bad) atomicAdd(&bad[blockIdx.y], n_bad);
}

// ---- instances
DEVI int64_t wave_sum_i64(int64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down((long long)v, d, 64);
    return v;                                                // lane 0 holds the sum
}

__global__ __launch_bounds__(TPB) void inst_sums_kernel(const uint32_t* __restrict__ masks, int h, int w, int words, u64* __restrict__ sums) {
    const int m = blockIdx.y;
    const int64_t wi64 = (int64_t)blockIdx.x * TPB + threadIdx.x;
    const uint32_t npix = (uint32_t)h * (uint32_t)w;
    int64_t cnt = 0, sp = 0, sy = 0;
    if (wi64 < words) {
        const uint32_t wi = (uint32_t)wi64, p0 = wi * 32u;
        uint32_t bits = masks[(size_t)m * words + wi];
        const uint32_t live = npix - p0;                     // >= 1
        if (live < 32u) bits &= (1u << live) - 1u;           // the padding bits hold anything
        if (bits) {
            const uint32_t n = __popc(bits);
            const uint32_t sk = __popc(bits & 0xaaaaaaaau) + 2u * __popc(bits & 0xccccccccu) + 4u * __popc(bits & 0xf0f0f0f0u) +
                                8u * __popc(bits & 0xff00ff00u) + 16u * __popc(bits & 0xffff0000u);
            cnt = n;
            sp = (int64_t)n * p0 + sk;
            uint32_t y = p0 / (uint32_t)w;
            uint32_t row_end = (y + 1u) * (uint32_t)w;       // <= npix + w: h * w < 2^31 keeps it inside 32 bits
            uint32_t lo = 0;                                 // bit of the word where row y's part begins
            const uint32_t end = min(32u, live);
            while (lo < end) {
                const uint32_t hi = min(end, row_end - p0);
                const uint32_t seg = hi - lo >= 32u ? 0xffffffffu : ((1u << (hi - lo)) - 1u) << lo;
                sy += (int64_t)y * __popc(bits & seg);
                lo = hi; ++y; row_end += (uint32_t)w;
            }
        }
    }
    cnt = wave_sum_i64(cnt);
    sp = wave_sum_i64(sp);
    sy = wave_sum_i64(sy);
    if ((threadIdx.x & 63) == 0 && cnt) {
        atomicAdd(&sums[3 * m], (u64)cnt);
        atomicAdd(&sums[3 * m + 1], (u64)(sp - (int64_t)w * sy));
        atomicAdd(&sums[3 * m + 2], (u64)sy);
    }
}

__global__ __launch_bounds__(TPB) void inst_colour_kernel(const u64* __restrict__ sums, const int* __restrict__ cells_in, int n, int h, int w,
                                                         const uint8_t* __restrict__ palette, uint32_t* __restrict__ colours,
                                                         int* __restrict__ cells, int* __restrict__ empty) {
    const int m = blockIdx.x * TPB + threadIdx.x;
    if (m == 0) empty[0] = 1;
    if (m >= n) return;
    int ax, ay;
    if (cells_in) {
        ax = clampi(cells_in[2 * m], 0, 79);
        ay = clampi(cells_in[2 * m + 1], 0, 79);
    } else {
        const double norm = sums[3 * m] ? (double)sums[3 * m] : 1e-6;
        const double cx = (double)sums[3 * m + 1] / norm, cy = (double)sums[3 * m + 2] / norm;
        ax = clampi((int)(cx / (double)w * 79.0), 0, 79);    // the clamp never acts: cx <= w - 1
        ay = clampi((int)(cy / (double)h * 79.0), 0, 79);
    }
    cells[2 * m] = ax;
    cells[2 * m + 1] = ay;
    const int row = (((ay / 20) * 4 + ax / 20) * 20 + ay % 20) * 20 + ax % 20;
    colours[m] = (uint32_t)palette[3 * row] | ((uint32_t)palette[3 * row + 1] << 8) | ((uint32_t)palette[3 * row + 2] << 16);
}

__global__ __launch_bounds__(TPB) void inst_paint_kernel(const uint32_t* __restrict__ masks, int n, int words, uint32_t npix,
                                                        const uint32_t* __restrict__ colours, uint8_t* __restrict__ out, int* __restrict__ empty) {
    __shared__ uint32_t s_colour[PA_PAINT_MAX_MASKS];
    for (int i = threadIdx.x; i < n; i += TPB) s_colour[i] = colours[i];
    __syncthreads();
    const int64_t wi64 = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (wi64 >= words) return;
    const uint32_t wi = (uint32_t)wi64, p0 = wi * 32u, live = npix - p0;
    const uint32_t valid = live < 32u ? (1u << live) - 1u : 0xffffffffu;
    uint32_t px[32];
#pragma unroll
    for (int b = 0; b < 32; ++b) px[b] = 0;
    uint32_t owned = 0, any = 0;
    for (int m = n - 1; m >= 0 && owned != valid; --m) {
        const uint32_t bits = masks[(size_t)m * words + wi] & valid & ~owned;
        if (!bits) continue;
        const uint32_t c = s_colour[m];
        any |= c;
        owned |= bits;
#pragma unroll
        for (int b = 0; b < 32; ++b)
            if ((bits >> b) & 1u) px[b] = c;
    }
    uint32_t d[24];                                          // 32 pixels of 3 bytes
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        const uint32_t a = px[4 * g], b = px[4 * g + 1], c = px[4 * g + 2], e = px[4 * g + 3];
        d[3 * g] = (a & 0xffffffu) | (b << 24);
        d[3 * g + 1] = ((b >> 8) & 0xffffu) | (c << 16);
        d[3 * g + 2] = ((c >> 16) & 0xffu) | (e << 8);
    }
    uint8_t* dst = out + (size_t)p0 * 3;                     // 96 * wi from a 16-byte aligned base
    if (live >= 32u) {
        uint4* q = (uint4*)dst;
#pragma unroll
        for (int i = 0; i < 6; ++i) q[i] = make_uint4(d[4 * i], d[4 * i + 1], d[4 * i + 2], d[4 * i + 3]);
    } else {
        const uint32_t nbytes = live * 3u;                   // the last word: not one byte beyond the picture
#pragma unroll
        for (int i = 0; i < 24; ++i) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if ((uint32_t)(4 * i + k) < nbytes) dst[4 * i + k] = (uint8_t)(d[i] >> (8 * k));
        }
    }
    if (any) empty[0] = 0;                                   // every writer stores the same value
}

// ---- pose
__global__ __launch_bounds__(TPB) void pose_paint_kernel(const int* __restrict__ rects, int n_joints, int h, int w, int c_kernel,
                                                        const uint8_t* __restrict__ colours, const uint8_t* __restrict__ table, int table_len,
                                                        uint8_t* __restrict__ out) {
    __shared__ int s_rect[2 * PA_PAINT_MAX_JOINTS * 4];      // (x0, y0, x1, y1) clipped, then the unclipped ul in s_ul
    __shared__ int s_ul[2 * PA_PAINT_MAX_JOINTS * 2];
    __shared__ uint32_t s_gb[PA_PAINT_MAX_JOINTS];
    __shared__ uint8_t s_table[PA_PAINT_MAX_TABLE];
    const int t = threadIdx.x, box = blockIdx.y;
    const uint32_t npix = (uint32_t)h * (uint32_t)w;
    const int* r = rects + (size_t)box * 2 * n_joints * 4;
    if (t < 2 * n_joints) {
        const int ulx = r[4 * t], uly = r[4 * t + 1], brx = r[4 * t + 2], bry = r[4 * t + 3];
        const bool some = brx > ulx && bry > uly;
        s_rect[4 * t] = some ? max(ulx, 0) : 0;
        s_rect[4 * t + 1] = some ? max(uly, 0) : 0;
        s_rect[4 * t + 2] = some ? min(brx, w) : 0;
        s_rect[4 * t + 3] = some ? min(bry, h) : 0;
        s_ul[2 * t] = ulx;
        s_ul[2 * t + 1] = uly;
    }
    if (t < n_joints) s_gb[t] = ((uint32_t)colours[2 * t] << 8) | ((uint32_t)colours[2 * t + 1] << 16);
    for (int i = t; i < table_len; i += TPB) s_table[i] = table[i];
    __syncthreads();
    const uint32_t p = (blockIdx.x * TPB + t) * PPT;
    if (p >= npix) return;
    uint32_t c[PPT];
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
        c[i] = 0;
        if (p + i >= npix) continue;
        const int y = (int)((p + i) / (uint32_t)w), x = (int)((p + i) - (uint32_t)y * (uint32_t)w);
        int n_class = 0, one = 0, best = 0;
        int64_t best_d2 = -1;
        for (int k = 0; k < n_joints; ++k) {
            const int* a = s_rect + 4 * k;
            if (x >= a[0] && x < a[2] && y >= a[1] && y < a[3]) { if (!n_class) one = k; ++n_class; }
            const int* b = s_rect + 4 * (n_joints + k);
            if (x >= b[0] && x < b[2] && y >= b[1] && y < b[3]) {
                const int64_t dx = (int64_t)x - s_ul[2 * (n_joints + k)] - c_kernel, dy = (int64_t)y - s_ul[2 * (n_joints + k) + 1] - c_kernel;
                const int64_t d2 = dx * dx + dy * dy;
                if (best_d2 < 0 || d2 < best_d2) { best_d2 = d2; best = k; }
            }
        }
        uint32_t v = 0;
        if (best_d2 >= 0) v = s_table[best_d2 < table_len ? (int)best_d2 : table_len - 1];
        if (n_class == 1) v |= s_gb[one];
        else if (n_class > 1) v |= s_gb[best];
        c[i] = v;
    }
    const size_t base = (size_t)box * npix * 3;
    store_pixels(out + base, p, npix, c, (base & 3) == 0);
}

}  // namespace

extern "C" {

int pa_paint_semantic(const void* jobs, int n_jobs, int64_t max_pixels, const void* palette_u8, int n_colours, void* out_bad,
                      hipStream_t stream) {
    if (!jobs || !palette_u8 || !out_bad || n_jobs < 1 || n_jobs > MAX_JOBS || max_pixels < 1 || max_pixels >= ((int64_t)1 << 31) ||
        n_colours < 1 || n_colours > PA_PAINT_MAX_COLOURS || ((uintptr_t)jobs & 7) || ((uintptr_t)out_bad & 3))
        return (int)hipErrorInvalidValue;
    PA_TRY(hipMemsetAsync(out_bad, 0, 4 * (size_t)n_jobs, stream));
    const unsigned gx = (unsigned)((max_pixels + TPB * PPT - 1) / (TPB * PPT));
    PA_LAUNCH(paint_semantic_kernel, dim3(gx, (unsigned)n_jobs), dim3(TPB), 0, stream, (const pa_paint_job*)jobs, max_pixels,
              (const uint8_t*)palette_u8, n_colours, (int*)out_bad);
    LAUNCH_CHECK();
}

int64_t pa_paint_instances_workspace_bytes(int n) {
    if (n < 0 || n > PA_PAINT_MAX_MASKS) return -1;
    const int64_t m = n > 1 ? n : 1;
    return up16(24 * m) + up16(4 * m);
}

int pa_paint_instances(const void* masks_u32, int n, int h, int w, const void* palette_u8, const void* cells_in, void* workspace,
                       void* out_picture, void* out_cells, void* out_empty, hipStream_t stream) {
    if (!masks_u32 || !palette_u8 || !workspace || !out_picture || !out_cells || !out_empty || n < 0 || n > PA_PAINT_MAX_MASKS ||
        !shape_ok(h, w) || ((uintptr_t)masks_u32 & 3) || ((uintptr_t)workspace & 15) || ((uintptr_t)out_picture & 15) ||
        ((uintptr_t)out_cells & 3) || ((uintptr_t)out_empty & 3) || ((uintptr_t)cells_in & 3))
        return (int)hipErrorInvalidValue;
    const int64_t m = n > 1 ? n : 1;
    const uint32_t npix = (uint32_t)h * (uint32_t)w;
    const int words = (int)(((int64_t)npix + 31) / 32);
    u64* sums = (u64*)workspace;
    uint32_t* colours = (uint32_t*)((char*)workspace + up16(24 * m));
    const unsigned gw = (unsigned)((words + TPB - 1) / TPB);
    if (n && !cells_in) {
        PA_TRY(hipMemsetAsync(sums, 0, 24 * (size_t)n, stream));
        PA_LAUNCH_TRY(inst_sums_kernel, dim3(gw, (unsigned)n), dim3(TPB), 0, stream, (const uint32_t*)masks_u32, h, w, words, sums);
    }
    PA_LAUNCH_TRY(inst_colour_kernel, dim3((unsigned)((m + TPB - 1) / TPB)), dim3(TPB), 0, stream, (const u64*)sums, (const int*)cells_in, n, h, w,
                  (const uint8_t*)palette_u8, colours, (int*)out_cells, (int*)out_empty);
    PA_LAUNCH(inst_paint_kernel, dim3(gw), dim3(TPB), 0, stream, (const uint32_t*)masks_u32, n, words, npix, (const uint32_t*)colours,
              (uint8_t*)out_picture, (int*)out_empty);
    LAUNCH_CHECK();
}

int pa_paint_pose(const void* rects, int n_boxes, int n_joints, int h, int w, int c_kernel, const void* colours_u8,
                  const void* table_u8, int table_len, void* out, hipStream_t stream) {
    if (!rects || !colours_u8 || !table_u8 || !out || n_boxes < 1 || n_boxes > MAX_JOBS || n_joints < 1 || n_joints > PA_PAINT_MAX_JOINTS ||
        !shape_ok(h, w) || table_len < 1 || table_len > PA_PAINT_MAX_TABLE || c_kernel < 0 || ((uintptr_t)rects & 3) ||
        ((uintptr_t)out & 3))
        return (int)hipErrorInvalidValue;
    const unsigned gx = (unsigned)(((int64_t)h * w + TPB * PPT - 1) / (TPB * PPT));
    PA_LAUNCH(pose_paint_kernel, dim3(gx, (unsigned)n_boxes), dim3(TPB), 0, stream, (const int*)rects, n_joints, h, w, c_kernel,
              (const uint8_t*)colours_u8, (const uint8_t*)table_u8, table_len, (uint8_t*)out);
    LAUNCH_CHECK();
}

}  // extern "C"
