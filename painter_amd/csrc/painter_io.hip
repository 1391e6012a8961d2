// Painter task inference, pre-/post-processing on the device: what the eight scripts Painter/eval/*/painter_inference_*.py do around
// the model call with numpy and CPU torch, and the colour -> class decode of ADE20kSemSegEvaluatorCustom.py, for a whole batch of
// pictures at once.
//
//   stitch        : 1 prompt pair + N queries -> the two normalised float32 canvases            (painter_inference_segm.py:150-162)
//   decode_u8     : tokens -> clip((y * std + mean) * 255, 0, 255) -> bilinear / nearest resize -> trunc -> uint8     (:88-92)
//   decode_depth  : tokens -> clip(. * 10000, 0, 10000) -> bilinear -> mean over channels -> trunc -> int32 (…_depth.py:69-73)
//   decode_f64    : tokens -> y * std + mean -> bicubic resize -> float64 (+ the saved uint8 picture)    (…_derain.py:76-79)
//   palette_argmin: uint8 picture -> index of the nearest palette colour            (ADE20kSemSegEvaluatorCustom.py:114-141)
//
// The decode kernels read the model's float32 tokens directly (unpatchify is index math, image_io.h) and walk a job table in device
// memory, one record per picture, so that pictures of different sizes are one launch and no float64 canvas ever goes to HBM: a thread
// produces one output pixel from the 4 (bilinear), 1 (nearest) or 16 (bicubic) source pixels it needs, which it de-normalises itself.
// The 448 x 448 x 3 float32 source of a sample is 2.4 MB and stays in L2 while its picture is written.  Everything is float64 VALU work
// and byte stores: HBM- and launch-bound, no MFMA.
//
// Bit-exactness with the scripts' files is the contract for the uint8 / int32 outputs.  They are trunc() of float64 values that sit
// exactly on 0 / 255 / 10000 over whole saturated regions, so one ulp flips a byte.  CPU torch's float64 bilinear kernel is
// reproduced by this operation order (tests/painter_eval_host.py states and checks it):
//     scale = in / out;  p = max(fma(scale, dst + 0.5, -0.5), 0);  i0 = min(floor(p), in - 1);  i1 = min(i0 + 1, in - 1);
//     l = p - i0;  w0 = 1 - l;  w1 = l;  row_k = fma(wx0, src[y_k][x0], wx1 * src[y_k][x1]);  out = fma(wy0, row_0, wy1 * row_1)
// The fma() calls below are therefore deliberate and the ONLY fused operations of this file (-ffp-contract=off in build.py and the
// pragma below keep the compiler from adding others).  Bicubic is a plain restatement (weights, then sum over x inside sum over y)
// and agrees with torch to ~1e-13, not to the bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/painter_hip.h"
#include "common.h"
#include "image_io.h"
#include "painter_post.h"

#pragma clang fp contract(off)

namespace {

inline dim3 grid2(int w, int h, int z = 1) { return dim3((unsigned)((w + 255) / 256), (unsigned)h, (unsigned)z); }

// grid: x = blocks of 256 columns, y = row of the stitched 2R x W canvas, z = query.
__global__ __launch_bounds__(256) void painter_stitch_kernel(const uint8_t* __restrict__ prompt, const uint8_t* __restrict__ target,
                                                             const uint8_t* __restrict__ queries, float* __restrict__ imgs,
                                                             float* __restrict__ tgts, int R, int W) {
    const int x = blockIdx.x * 256 + threadIdx.x, row = blockIdx.y, n = blockIdx.z;
    if (x >= W) return;
    const int r = row < R ? row : row - R;
    const size_t px = ((size_t)r * W + x) * 3, img_sz = (size_t)R * W * 3;
    const uint8_t* a = row < R ? prompt + px : queries + n * img_sz + px;
    const uint8_t* t = target + px;                           // "tgt is not available": the prompt's target fills both halves
    const size_t plane = (size_t)2 * R * W;
    const size_t o = (size_t)n * 3 * plane + (size_t)row * W + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        imgs[o + c * plane] = normalise(a[c], 255.0, c);
        tgts[o + c * plane] = normalise(t[c], 255.0, c);
    }
}

// aten area_pixel_compute_source_index (align_corners = False, not cubic) + the index / weight lines of the CPU bilinear kernel.
struct Lin {
    int i0, i1;
    double w0, w1;
};
DEVI Lin lin_coord(int dst, int in, int out) {
    const double scale = (double)in / (double)out;
    double p = fma(scale, (double)dst + 0.5, -0.5);
    p = p < 0.0 ? 0.0 : p;
    Lin c;
    c.i0 = min((int)floor(p), in - 1);
    c.i1 = min(c.i0 + 1, in - 1);
    const double l = p - (double)c.i0;
    c.w0 = 1.0 - l;
    c.w1 = l;
    return c;
}

// F.interpolate(mode='nearest'): scale * dst in double, narrowed to float32, floored, clamped (resample.torch_nearest_table).
DEVI int nearest_coord(int dst, int in, int out) {
    const double scale = (double)in / (double)out;
    return min((int)floorf((float)(scale * (double)dst)), in - 1);
}

// aten get_cubic_upsample_coefficients, A = -0.75
DEVI double cubic1(double x) { return ((-0.75 + 2.0) * x - (-0.75 + 3.0)) * x * x + 1.0; }
DEVI double cubic2(double x) { return ((-0.75 * x - 5.0 * -0.75) * x + 8.0 * -0.75) * x - 4.0 * -0.75; }
struct Cub {
    int i;
    double w[4];
};
DEVI Cub cub_coord(int dst, int in, int out) {
    const double scale = (double)in / (double)out;
    const double p = scale * ((double)dst + 0.5) - 0.5;
    const double f = floor(p), t = p - f;
    Cub c;
    c.i = (int)f;
    c.w[0] = cubic2(t + 1.0);
    c.w[1] = cubic1(t);
    const double u = 1.0 - t;
    c.w[2] = cubic1(u);
    c.w[3] = cubic2(u + 1.0);
    return c;
}

enum { MODE_U8_BILINEAR = 0, MODE_U8_NEAREST = 1, MODE_DEPTH = 2, MODE_F64 = 3 };

// grid: x = blocks of 256 output columns, y = output rows, z = job; both padded to the largest picture of the table.
template <int MODE>
__global__ __launch_bounds__(256) void painter_decode_kernel(const float* __restrict__ pred, const pa_decode_job* __restrict__ jobs, int n_samples,
                                                             int res_h, int res_w, int P) {
    const pa_decode_job jb = jobs[blockIdx.z];
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= jb.out_w || y >= jb.out_h || jb.sample < 0 || jb.sample >= n_samples) return;
    const int wp = res_w / P;
    const float* s = pred + (size_t)jb.sample * (2 * (res_h / P) * wp) * (P * P * 3);
    const size_t px = (size_t)y * jb.out_w + x;
    if constexpr (MODE == MODE_U8_NEAREST) {
        const int sy = nearest_coord(y, res_h, jb.out_h), sx = nearest_coord(x, res_w, jb.out_w);
        uint8_t* d = (uint8_t*)jb.out + px * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) d[c] = (uint8_t)(int)decoded_scaled(s, sy, sx, c, res_h, wp, P, 255.0);
    } else if constexpr (MODE == MODE_U8_BILINEAR || MODE == MODE_DEPTH) {
        const double scale = MODE == MODE_DEPTH ? 10000.0 : 255.0;
        const Lin cy = lin_coord(y, res_h, jb.out_h), cx = lin_coord(x, res_w, jb.out_w);
        double v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double r0 = fma(cx.w0, decoded_scaled(s, cy.i0, cx.i0, c, res_h, wp, P, scale),
                                  cx.w1 * decoded_scaled(s, cy.i0, cx.i1, c, res_h, wp, P, scale));
            const double r1 = fma(cx.w0, decoded_scaled(s, cy.i1, cx.i0, c, res_h, wp, P, scale),
                                  cx.w1 * decoded_scaled(s, cy.i1, cx.i1, c, res_h, wp, P, scale));
            v[c] = fma(cy.w0, r0, cy.w1 * r1);
        }
        if constexpr (MODE == MODE_DEPTH) {
            double m = v[0] + v[1];                                  // torch .mean(-1) of 3 float64 values: ((c0 + c1) + c2) / 3
            m = m + v[2];
            m = m / 3.0;
            ((int32_t*)jb.out)[px] = (int32_t)m;
        } else {
            uint8_t* d = (uint8_t*)jb.out + px * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) d[c] = (uint8_t)(int)v[c];   // .int() then astype(uint8) of a value in [0, 255]
        }
    } else {
        const Cub cy = cub_coord(y, res_h, jb.out_h), cx = cub_coord(x, res_w, jb.out_w);
        int xs[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) xs[k] = min(max(cx.i - 1 + k, 0), res_w - 1);
        double* d = (double*)jb.out + px * 3;
        uint8_t* d8 = jb.out2 == nullptr ? nullptr : (uint8_t*)jb.out2 + px * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int yy = min(max(cy.i - 1 + j, 0), res_h - 1);
                double rowv = 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) rowv = rowv + denormalised(s, yy, xs[k], c, res_h, wp, P) * cx.w[k];
                acc = acc + rowv * cy.w[j];
            }
            d[c] = acc;
            if (d8 != nullptr) {                                     // np.clip(., 0, 1) * 255 -> astype(uint8)
                double u = acc < 0.0 ? 0.0 : acc;
                u = u > 1.0 ? 1.0 : u;
                d8[c] = (uint8_t)(int)(u * 255.0);
            }
        }
    }
}

// One pixel per lane, the palette staged in LDS once per workgroup; the distance and the first minimum are nearest_colour of
// painter_post.h, which pa_semseg_confusion (painter_score.hip) shares.
template <int DIST>
__global__ __launch_bounds__(256) void palette_argmin_kernel(const uint8_t* __restrict__ image, const float* __restrict__ palette,
                                                             int32_t* __restrict__ out, int64_t n_pixels, int K) {
    extern __shared__ float pal_lds[];
    for (int i = threadIdx.x; i < K * 3; i += 256) pal_lds[i] = palette[i];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pixels) return;
    out[i] = nearest_colour<DIST>((float)image[i * 3], (float)image[i * 3 + 1], (float)image[i * 3 + 2], pal_lds, K);
}

bool decode_args_ok(int n_jobs, int n_samples, int max_h, int max_w, int res_h, int res_w, int patch) {
    return n_jobs >= 1 && n_jobs <= 65535 && n_samples >= 1 && max_h >= 1 && max_h <= 65535 && max_w >= 1 && patch >= 1 && res_h >= 1 &&
           res_w >= 1 && res_h % patch == 0 && res_w % patch == 0;
}

template <int MODE>
int launch_decode(const float* pred, const pa_decode_job* jobs, int n_jobs, int n_samples, int max_h, int max_w, int res_h, int res_w,
                  int patch, hipStream_t stream) {
    if (!decode_args_ok(n_jobs, n_samples, max_h, max_w, res_h, res_w, patch)) return (int)hipErrorInvalidValue;
    PA_LAUNCH(painter_decode_kernel<MODE>, grid2(max_w, max_h, n_jobs), dim3(256), 0, stream, pred, jobs, n_samples, res_h, res_w, patch);
    LAUNCH_CHECK();
}

}  // namespace

extern "C" {

int pa_painter_stitch(const void* prompt, const void* prompt_target, const void* queries, float* imgs, float* tgts, int n_queries,
                      int res_h, int res_w, hipStream_t stream) {
    if (n_queries < 1 || n_queries > 65535 || res_h < 1 || res_w < 1 || 2 * res_h > 65535) return (int)hipErrorInvalidValue;
    PA_LAUNCH(painter_stitch_kernel, grid2(res_w, 2 * res_h, n_queries), dim3(256), 0, stream, (const uint8_t*)prompt,
              (const uint8_t*)prompt_target, (const uint8_t*)queries, imgs, tgts, res_h, res_w);
    LAUNCH_CHECK();
}

int pa_painter_decode_u8(const float* pred, const pa_decode_job* jobs, int n_jobs, int n_samples, int max_h, int max_w, int res_h,
                         int res_w, int patch, int nearest, hipStream_t stream) {
    if (nearest) return launch_decode<MODE_U8_NEAREST>(pred, jobs, n_jobs, n_samples, max_h, max_w, res_h, res_w, patch, stream);
    return launch_decode<MODE_U8_BILINEAR>(pred, jobs, n_jobs, n_samples, max_h, max_w, res_h, res_w, patch, stream);
}

int pa_painter_decode_depth(const float* pred, const pa_decode_job* jobs, int n_jobs, int n_samples, int max_h, int max_w, int res_h,
                            int res_w, int patch, hipStream_t stream) {
    return launch_decode<MODE_DEPTH>(pred, jobs, n_jobs, n_samples, max_h, max_w, res_h, res_w, patch, stream);
}

int pa_painter_decode_f64(const float* pred, const pa_decode_job* jobs, int n_jobs, int n_samples, int max_h, int max_w, int res_h,
                          int res_w, int patch, hipStream_t stream) {
    return launch_decode<MODE_F64>(pred, jobs, n_jobs, n_samples, max_h, max_w, res_h, res_w, patch, stream);
}

int pa_palette_argmin(const void* image, const float* palette, void* out_i32, int h, int w, int n_colours, int dist_type,
                      hipStream_t stream) {
    if (h < 1 || w < 1 || n_colours < 1 || n_colours > 4096 || dist_type < 0 || dist_type > 2) return (int)hipErrorInvalidValue;
    const int64_t n = (int64_t)h * w;
    if ((n + 255) / 256 > 0x7fffffff) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)((n + 255) / 256));
    const size_t lds = (size_t)n_colours * 3 * sizeof(float);
    const uint8_t* img = (const uint8_t*)image;
    int32_t* o = (int32_t*)out_i32;
    if (dist_type == 0) PA_LAUNCH(palette_argmin_kernel<0>, grid, dim3(256), lds, stream, img, palette, o, n, n_colours);
    else if (dist_type == 1) PA_LAUNCH(palette_argmin_kernel<1>, grid, dim3(256), lds, stream, img, palette, o, n, n_colours);
    else PA_LAUNCH(palette_argmin_kernel<2>, grid, dim3(256), lds, stream, img, palette, o, n, n_colours);
    LAUNCH_CHECK();
}

}  // extern "C"
