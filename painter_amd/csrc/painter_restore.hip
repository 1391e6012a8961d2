// PSNR and SSIM of restored pictures against their ground truth on the device: what painter_inference_lol.py:166-169 leaves to
// skimage (peak_signal_noise_ratio / structural_similarity on float64 [H][W][3] pictures, six 7 x 7 uniform filters per channel in scipy)
// and what derain's evaluate_PSNR_SSIM.m does with the saved PNGs (Y of rgb2ycbcr, SSIM_index with an 11 x 11 Gaussian).  Both are a
// separable window stencil over two planes followed by a sum; only eight doubles per picture leave the device.
// tests/painter_restore_host.py is the definition.
//
//   tiles   : a workgroup of 256 threads owns TILE x TILE output windows of one channel of one job; workgroup t of the launch is tile t of
//             the job table (jobs in order; per job channel, tile row, tile column), which it finds by walking the table.  It stages the
//             (TILE + win - 1)^2 halo of both planes into LDS as float64 -- the clip / the division by 255 / the integer Y happen here, and
//             every input pixel is read from memory once per tile that touches it -- and adds (x - y)^2 over the pixels it owns (its
//             TILE x TILE corner, up to the picture's edge in the last tile row / column: every pixel has one owner).  The horizontal pass
//             writes the five moment rows sum_k w[k] {x, y, x x, y y, x y} to LDS, the vertical pass finishes them in registers, S is
//             formed in float64 with one IEEE division, and the workgroup's sum of S is reduced in the wave (shuffles), then across the
//             waves (LDS), in a fixed order.  One partial (squared sum, sum of S) per workgroup goes to the workspace.
//   reduce  : one thread per (job, output number) adds the job's partials in index order.  No floating-point atomics: two runs give the
//             same bits, and a picture's numbers do not depend on which other pictures share the launch.
//
// LDS: 2 planes of 34 x 34 and 5 moment planes of 34 x 24 doubles = 51,136 bytes, plus 11 weights and 8 wave partials: three workgroups
// (12 waves) per CU within 160 KB.  DESIGN.md section 4.13 has the choice of TILE.
//
// The job table is a HOST array: the entry point checks every picture against the window before anything is enqueued, counts the tiles,
// and copies the table into the workspace on the stream.  Stream-ordered, allocates nothing, never waits for the device.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "../../include/painter_hip.h"
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int TILE = 24;                          // output windows per tile side
constexpr int MAX_WIN = 11;
constexpr int EDGE = TILE + MAX_WIN - 1;          // 34: the largest halo side, and the row stride of the staged planes
constexpr int THREADS = 256;
constexpr int OUT = 8;                            // count, squared sum, (sum of S, windows) x 3 channels
constexpr int MAX_JOBS = 1024;                    // every workgroup walks the table
constexpr int64_t MAX_TILES = (int64_t)1 << 24;      // x 256 threads = 2^32 work-items, the most a grid dimension is asked for

struct Weights {
    double w[MAX_WIN];
};

__host__ __device__ inline int64_t tiles_along(int n, int win) { return ((int64_t)n - win + 1 + TILE - 1) / TILE; }
__host__ __device__ inline int64_t job_tiles(int h, int w, int win, int channels) {
    return channels * tiles_along(h, win) * tiles_along(w, win);
}

// Walks the table: -> the job that holds tile `t` of the launch and t's index within it, or -1.
DEVI int find_job(const pa_restore_job* __restrict__ jobs, int n_jobs, int win, int channels, int64_t& t) {
    for (int j = 0; j < n_jobs; ++j) {
        const int64_t nt = job_tiles(jobs[j].h, jobs[j].w, win, channels);
        if (t < nt) return j;
        t -= nt;
    }
    return -1;
}

DEVI int luma(const uint8_t* __restrict__ p) {                     // Y of rgb2ycbcr, rounded half up, exact
    return 16 + (65481 * (int)p[0] + 128553 * (int)p[1] + 24966 * (int)p[2] + 127500) / 255000;
}

// grid: x = tile of the launch.  partials: [total_tiles][2] 8-byte slots: the squared sum (a double; int64 in Y mode), the sum of S.
template <int MODE>
__global__ __launch_bounds__(THREADS) void restore_tiles_kernel(const pa_restore_job* __restrict__ jobs, int n_jobs, int win, Weights wts,
                                                                double cov_norm, double c1, double c2, double* __restrict__ partials) {
    __shared__ double sx[EDGE * EDGE], sy[EDGE * EDGE];
    __shared__ double mom[5][EDGE * TILE];
    __shared__ double sw[MAX_WIN];
    __shared__ double s_part[THREADS / 64][2];
    constexpr int CH = MODE == PA_RESTORE_RGB_F64 ? 3 : 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t t = blockIdx.x;
    const int j = find_job(jobs, n_jobs, win, CH, t);
    if (j < 0) return;                                                        // uniform over the workgroup
    const int h = jobs[j].h, w = jobs[j].w;
    const void* __restrict__ pred = jobs[j].pred;
    const uint8_t* __restrict__ gt = static_cast<const uint8_t*>(jobs[j].gt);
    const int nwy = h - win + 1, nwx = w - win + 1;                           // windows of the picture
    const int tiles_x = (int)tiles_along(w, win), tiles_y = (int)tiles_along(h, win);
    const int ch = (int)(t / ((int64_t)tiles_y * tiles_x));
    const int ty = (int)(t / tiles_x % tiles_y), tx = (int)(t % tiles_x);
    const int y0 = ty * TILE, x0 = tx * TILE;
    const int ny = nwy - y0 < TILE ? nwy - y0 : TILE, nx = nwx - x0 < TILE ? nwx - x0 : TILE;      // windows of this tile
    const int eh = ny + win - 1, ew = nx + win - 1;                           // its halo: rows y0 .. y0 + eh - 1 <= h - 1
    const int own_h = ty == tiles_y - 1 ? eh : TILE, own_w = tx == tiles_x - 1 ? ew : TILE;
    if (tid < MAX_WIN) sw[tid] = tid < win ? wts.w[tid] : 0.0;

    double ssd = 0.0;
    long long ssd_i = 0;
    for (int i = tid; i < eh * ew; i += THREADS) {
        const int r = i / ew, c = i % ew;
        const int64_t p = (int64_t)(y0 + r) * w + x0 + c;
        const bool own = r < own_h && c < own_w;
        double xv, yv;
        if (MODE == PA_RESTORE_RGB_F64) {
            const double v = static_cast<const double*>(pred)[3 * p + ch];
            xv = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);                         // np.clip: a NaN stays
            yv = (double)gt[3 * p + ch] / 255.0;
            const double d = xv - yv;
            if (own) ssd += d * d;
        } else {
            const int yp = luma(static_cast<const uint8_t*>(pred) + 3 * p);
            const int yg = luma(gt + 3 * p);
            xv = (double)yp;
            yv = (double)yg;
            if (own) ssd_i += (long long)((yp - yg) * (yp - yg));
        }
        sx[r * EDGE + c] = xv;
        sy[r * EDGE + c] = yv;
    }
    __syncthreads();

    // horizontal: five moment rows per halo row
    for (int i = tid; i < eh * nx; i += THREADS) {
        const int r = i / nx, c = i % nx;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0;
        for (int k = 0; k < win; ++k) {
            const double xv = sx[r * EDGE + c + k], yv = sy[r * EDGE + c + k], wk = sw[k];
            a0 += wk * xv;
            a1 += wk * yv;
            a2 += wk * (xv * xv);
            a3 += wk * (yv * yv);
            a4 += wk * (xv * yv);
        }
        mom[0][r * TILE + c] = a0;
        mom[1][r * TILE + c] = a1;
        mom[2][r * TILE + c] = a2;
        mom[3][r * TILE + c] = a3;
        mom[4][r * TILE + c] = a4;
    }
    __syncthreads();

    // vertical, then S
    double acc = 0.0;
    for (int i = tid; i < ny * nx; i += THREADS) {
        const int r = i / nx, c = i % nx;
        double ux = 0.0, uy = 0.0, uxx = 0.0, uyy = 0.0, uxy = 0.0;
        for (int k = 0; k < win; ++k) {
            const double wk = sw[k];
            const int at = (r + k) * TILE + c;
            ux += wk * mom[0][at];
            uy += wk * mom[1][at];
            uxx += wk * mom[2][at];
            uyy += wk * mom[3][at];
            uxy += wk * mom[4][at];
        }
        const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
        acc += ((2.0 * (ux * uy) + c1) * (2.0 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2));
    }

#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        acc += __shfl_down(acc, off, 64);
        if (MODE == PA_RESTORE_RGB_F64) ssd += __shfl_down(ssd, off, 64);
        else ssd_i += __shfl_down(ssd_i, off, 64);
    }
    if (lane == 0) {
        s_part[wave][0] = MODE == PA_RESTORE_RGB_F64 ? ssd : __longlong_as_double(ssd_i);
        s_part[wave][1] = acc;
    }
    __syncthreads();
    if (tid == 0) {
        double s = s_part[0][1];
        for (int k = 1; k < THREADS / 64; ++k) s += s_part[k][1];
        partials[2 * (int64_t)blockIdx.x + 1] = s;
        if (MODE == PA_RESTORE_RGB_F64) {
            double d = s_part[0][0];
            for (int k = 1; k < THREADS / 64; ++k) d += s_part[k][0];
            partials[2 * (int64_t)blockIdx.x] = d;
        } else {
            long long d = __double_as_longlong(s_part[0][0]);
            for (int k = 1; k < THREADS / 64; ++k) d += __double_as_longlong(s_part[k][0]);
            partials[2 * (int64_t)blockIdx.x] = __longlong_as_double(d);
        }
    }
}

// One thread per (job, output number): the partials of a job in index order.
template <int MODE>
__global__ __launch_bounds__(256) void restore_reduce_kernel(const pa_restore_job* __restrict__ jobs, int n_jobs, int win,
                                                             const double* __restrict__ partials, double* __restrict__ out) {
    constexpr int CH = MODE == PA_RESTORE_RGB_F64 ? 3 : 1;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_jobs * OUT) return;
    const int j = i / OUT, k = i % OUT;
    int64_t first = 0;
    for (int q = 0; q < j; ++q) first += job_tiles(jobs[q].h, jobs[q].w, win, CH);
    const int h = jobs[j].h, w = jobs[j].w;
    const int64_t per_channel = job_tiles(h, w, win, 1);
    double v = 0.0;
    if (k == 0) {
        v = (double)((int64_t)CH * h * w);
    } else if (k == 1) {
        if (MODE == PA_RESTORE_RGB_F64) {
            for (int64_t t = first; t < first + CH * per_channel; ++t) v += partials[2 * t];
        } else {
            long long d = 0;
            for (int64_t t = first; t < first + per_channel; ++t) d += __double_as_longlong(partials[2 * t]);
            v = (double)d;
        }
    } else if ((k - 2) / 2 < CH) {
        const int c = (k - 2) / 2;
        if (k & 1) {
            v = (double)((int64_t)(h - win + 1) * (w - win + 1));
        } else {
            for (int64_t t = first + c * per_channel; t < first + (c + 1) * per_channel; ++t) v += partials[2 * t + 1];
        }
    }
    out[i] = v;
}

template <int MODE>
int launch_restore(const pa_restore_job* table, int n_jobs, int64_t total, int win, const Weights& wts, double cov_norm, double c1, double c2,
                   double* partials, double* out, hipStream_t stream) {
    PA_LAUNCH_TRY(restore_tiles_kernel<MODE>, dim3((unsigned)total), dim3(THREADS), 0, stream, table, n_jobs, win, wts, cov_norm, c1, c2,
                  partials);
    PA_LAUNCH(restore_reduce_kernel<MODE>, dim3((unsigned)((n_jobs * OUT + 255) / 256)), dim3(256), 0, stream, table, n_jobs, win,
              (const double*)partials, out);
    LAUNCH_CHECK();
}

}  // namespace

extern "C" {

int pa_restore_tile(void) { return TILE; }

int64_t pa_restore_workspace_bytes(int n_jobs, int64_t total_tiles) {
    if (n_jobs < 1 || n_jobs > MAX_JOBS || total_tiles < 1 || total_tiles > MAX_TILES) return -1;
    return total_tiles * 16 + (int64_t)n_jobs * (int64_t)sizeof(pa_restore_job);
}

int pa_restore_scores(const pa_restore_job* jobs, int n_jobs, int mode, int win, const double* weights_f64, double cov_norm, double c1,
                      double c2, void* out_f64, void* workspace, hipStream_t stream) {
    if (!jobs || !weights_f64 || !out_f64 || !workspace || n_jobs < 1 || n_jobs > MAX_JOBS ||
        (mode != PA_RESTORE_RGB_F64 && mode != PA_RESTORE_Y_U8) || win < 1 || win > MAX_WIN || !(cov_norm > 0.0) || !(cov_norm < INFINITY) ||
        !(c1 > 0.0) || !(c1 < INFINITY) || !(c2 > 0.0) || !(c2 < INFINITY) || (((uintptr_t)out_f64 | (uintptr_t)workspace) & 7) != 0)
        return (int)hipErrorInvalidValue;
    Weights wts;
    for (int k = 0; k < MAX_WIN; ++k) {
        wts.w[k] = k < win ? weights_f64[k] : 0.0;
        if (!(wts.w[k] == wts.w[k]) || wts.w[k] == INFINITY || wts.w[k] == -INFINITY) return (int)hipErrorInvalidValue;
    }
    const int channels = mode == PA_RESTORE_RGB_F64 ? 3 : 1;
    int64_t total = 0;
    for (int j = 0; j < n_jobs; ++j) {
        if (!jobs[j].pred || !jobs[j].gt || jobs[j].h < win || jobs[j].w < win) return (int)hipErrorInvalidValue;
        if (mode == PA_RESTORE_RGB_F64 && ((uintptr_t)jobs[j].pred & 7) != 0) return (int)hipErrorInvalidValue;
        total += job_tiles(jobs[j].h, jobs[j].w, win, channels);
        if (total > MAX_TILES) return (int)hipErrorInvalidValue;
    }
    double* partials = (double*)workspace;
    pa_restore_job* table = (pa_restore_job*)(partials + 2 * total);
    PA_TRY(hipMemcpyAsync(table, jobs, (size_t)n_jobs * sizeof(pa_restore_job), hipMemcpyHostToDevice, stream));
    if (mode == PA_RESTORE_RGB_F64)
        return launch_restore<PA_RESTORE_RGB_F64>(table, n_jobs, total, win, wts, cov_norm, c1, c2, partials, (double*)out_f64, stream);
    return launch_restore<PA_RESTORE_Y_U8>(table, n_jobs, total, win, wts, cov_norm, c1, c2, partials, (double*)out_f64, stream);
}

}  // extern "C"
