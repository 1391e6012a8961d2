// Scoring of painted pictures against ground-truth maps on the device: what the two semantic evaluators do per picture with a float32
// [H][W][K][3] difference tensor, a copy of the arg-min to the host and np.bincount (Painter/eval/ade20k_semantic/
// ADE20kSemSegEvaluatorCustom.py:75-141, eval/coco_panoptic/COCOPanoSemSegEvaluatorCustom.py:67-136), and what the NYUv2 depth evaluation
// does with the PNG it reads back (eval/nyuv2_depth/eval_with_pngs.py:50-71, 148-217).  Both are reductions of a picture that is already
// in device memory against a map of its size; only the sums leave the device.
//
//   confusion : conf[(K + 1) * pred + gt'] += 1 over the pixels of a whole job table in ONE launch.  Workgroups of 1024 threads stride
//               over chunks of 1024 pixels, numbered through all jobs.  A lane's class is nearest_colour of painter_post.h (the palette in
//               LDS, the float32 operations of pa_palette_argmin).  Lanes are consecutive pixels, and painted segmentations are coherent,
//               so a wave first folds runs of equal (pred, gt') neighbours: the first lane of a run adds the run's length -- one LDS
//               atomic per run instead of up to 64 on one address.  The workgroup counts into (K + 1)^2 private 32-bit bins in LDS
//               (91 KB at K = 150; a launch holds at most 2^31 pixels, so no bin wraps) and adds its non-zero bins to `conf` with 64-bit
//               integer atomics at the end.  Where palette and bins exceed 160 KB of LDS (K >= 200) the run heads add straight to `conf`:
//               the same kernel, BINS_IN_LDS = false.  Integer counts only: the result does not depend on the order of the atomics.
//   depth     : per picture n, three threshold counts and six float64 sums over the valid pixels of a crop box.  grid = (DEPTH_PARTS,
//               jobs): a workgroup takes every DEPTH_PARTS-th chunk of 256 box pixels, reduces in the wave (shuffles) and across its waves
//               (LDS) in a fixed order and stores its partial; a second launch adds the DEPTH_PARTS partials of a job in index order.  No
//               floating-point atomics: two runs give the same bits.  The float32 steps of the reference (the two divisions by 1000, the
//               clamp, the validity test, max(g / p, p / g)) are float32 here, so the counts are its own; the sums are float64 of float64
//               terms where the reference sums float32 terms in float32.
//
// Everything is stream-ordered, allocates nothing and never returns to the host.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "../../include/painter_hip.h"
#include "painter_post.h"

#pragma clang fp contract(off)

namespace {

constexpr int CONF_THREADS = 1024;                // = pixels of a chunk
constexpr int CONF_CUS = 256;                     // the grid is what is resident at once: a workgroup zeroes and flushes its bins once
constexpr int LDS_BYTES = 160 * 1024;
constexpr int64_t MAX_LAUNCH_PIXELS = (int64_t)1 << 31;
constexpr int DEPTH_THREADS = 256;
constexpr int DEPTH_PARTS = 32;                   // partials per job: 8 jobs fill the chip
constexpr int DEPTH_OUT = 10;                     // n, three counts, six sums

inline int64_t conf_lds_bytes(int K) { return up16(12 * (int64_t)K) + 4 * (int64_t)(K + 1) * (K + 1); }

// Keys of a lane: >= 0 a bin, KEY_NONE no pixel, KEY_INVALID a ground-truth value >= K that is not the ignore label.
constexpr int KEY_NONE = -1, KEY_INVALID = -2;

template <int DIST, bool BINS_IN_LDS>
__global__ __launch_bounds__(CONF_THREADS) void semseg_confusion_kernel(const pa_score_job* __restrict__ jobs, int n_jobs,
                                                                        const float* __restrict__ palette, int K, int ignore_label,
                                                                        u64* __restrict__ conf, u64* __restrict__ invalid) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* pal = reinterpret_cast<float*>(smem);
    uint32_t* bins = reinterpret_cast<uint32_t*>(smem + ((12 * K + 15) & ~15));
    const int tid = threadIdx.x, lane = tid & 63, n_bins = (K + 1) * (K + 1);
    for (int i = tid; i < 3 * K; i += CONF_THREADS) pal[i] = palette[i];
    if (BINS_IN_LDS)
        for (int i = tid; i < n_bins; i += CONF_THREADS) bins[i] = 0u;
    __syncthreads();
    uint32_t bad = 0;
    const int64_t G = gridDim.x;
    int64_t chunk0 = 0;                                           // number of this job's first chunk in the launch
    for (int j = 0; j < n_jobs; ++j) {                            // every branch on j, c is uniform over the workgroup
        const int h = jobs[j].h, w = jobs[j].w;
        if (h < 1 || w < 1) continue;
        const uint8_t* __restrict__ pic = static_cast<const uint8_t*>(jobs[j].picture);
        const uint8_t* __restrict__ gt = static_cast<const uint8_t*>(jobs[j].gt);
        const int64_t npix = (int64_t)h * w, n_chunks = (npix + CONF_THREADS - 1) / CONF_THREADS;
        for (int64_t c = ((int64_t)blockIdx.x - chunk0 % G + G) % G; c < n_chunks; c += G) {
            const int64_t p = c * CONF_THREADS + tid;
            int key = KEY_NONE;
            if (p < npix) {
                const int g = gt[p];
                const int pred = nearest_colour<DIST>((float)pic[3 * p], (float)pic[3 * p + 1], (float)pic[3 * p + 2], pal, K);
                key = g == ignore_label ? pred * (K + 1) + K : (g < K ? pred * (K + 1) + g : KEY_INVALID);
            }
            bad += key == KEY_INVALID ? 1u : 0u;
            // runs of equal keys among the wave's lanes: the head of a run adds its length
            const int before = __shfl_up(key, 1, 64);
            const bool head = lane == 0 || before != key;
            const u64 heads = __ballot(head);
            if (head && key >= 0) {
                const u64 later = lane == 63 ? 0ull : heads >> (lane + 1);
                const uint32_t len = later ? (uint32_t)__builtin_ctzll(later) + 1u : (uint32_t)(64 - lane);
                if (BINS_IN_LDS) atomicAdd(&bins[key], len);
                else atomicAdd(&conf[key], (u64)len);
            }
        }
        chunk0 += n_chunks;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) bad += __shfl_down(bad, off, 64);
    if (lane == 0 && bad) atomicAdd(invalid, (u64)bad);
    if (BINS_IN_LDS) {
        __syncthreads();
        for (int i = tid; i < n_bins; i += CONF_THREADS) {
            const uint32_t v = bins[i];
            if (v) atomicAdd(&conf[i], (u64)v);
        }
    }
}

template <int DIST>
int launch_confusion(const pa_score_job* jobs, int n_jobs, int64_t total, const float* palette, int K, int ignore_label, bool lds_bins,
                     u64* conf, u64* invalid, hipStream_t stream) {
    const int64_t chunks = (total + CONF_THREADS - 1) / CONF_THREADS;
    // two workgroups of 1024 threads fill a CU; bins beyond 80 KB leave room for one
    const int64_t resident = CONF_CUS * (lds_bins && 2 * conf_lds_bytes(K) > LDS_BYTES ? 1 : 2);
    const dim3 grid((unsigned)(chunks < resident ? chunks : resident));
    if (lds_bins) {
        static bool attr_done = false;
        if (!attr_done) {
            PA_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(semseg_confusion_kernel<DIST, true>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
            attr_done = true;
        }
        PA_LAUNCH((semseg_confusion_kernel<DIST, true>), grid, dim3(CONF_THREADS), (size_t)conf_lds_bytes(K), stream, jobs,
                  n_jobs, palette, K, ignore_label, conf, invalid);
    } else {
        PA_LAUNCH((semseg_confusion_kernel<DIST, false>), grid, dim3(CONF_THREADS), (size_t)up16(12 * (int64_t)K), stream, jobs,
                  n_jobs, palette, K, ignore_label, conf, invalid);
    }
    LAUNCH_CHECK();
}

// The ten numbers of a pixel set, and their fixed-order sums.
struct DepthAcc {
    uint32_t n, c1, c2, c3;
    double s[6];
};

DEVI void depth_wave_sum(DepthAcc& a) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        a.n += __shfl_down(a.n, off, 64);
        a.c1 += __shfl_down(a.c1, off, 64);
        a.c2 += __shfl_down(a.c2, off, 64);
        a.c3 += __shfl_down(a.c3, off, 64);
#pragma unroll
        for (int k = 0; k < 6; ++k) a.s[k] += __shfl_down(a.s[k], off, 64);
    }
}

// grid: x = part of the job (DEPTH_PARTS), y = job.  partials: double [jobs][DEPTH_PARTS][DEPTH_OUT].
__global__ __launch_bounds__(DEPTH_THREADS) void depth_errors_kernel(const pa_depth_job* __restrict__ jobs, float divisor, float min_depth,
                                                                     float max_depth, double* __restrict__ partials) {
    __shared__ double s_part[DEPTH_THREADS / 64][DEPTH_OUT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = blockIdx.y;
    const int h = jobs[j].h, w = jobs[j].w;
    const int y0 = jobs[j].y0 > 0 ? jobs[j].y0 : 0, x0 = jobs[j].x0 > 0 ? jobs[j].x0 : 0;      // the box never leaves the picture
    const int y1 = jobs[j].y1 < h ? jobs[j].y1 : h, x1 = jobs[j].x1 < w ? jobs[j].x1 : w;
    const int32_t* __restrict__ pred = static_cast<const int32_t*>(jobs[j].pred);
    const uint16_t* __restrict__ gt = static_cast<const uint16_t*>(jobs[j].gt);
    DepthAcc a = {0u, 0u, 0u, 0u, {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}};
    if (y1 > y0 && x1 > x0) {
        const int bw = x1 - x0;
        const int64_t nbox = (int64_t)(y1 - y0) * bw;
        for (int64_t q = (int64_t)blockIdx.x * DEPTH_THREADS + tid; q < nbox; q += (int64_t)DEPTH_PARTS * DEPTH_THREADS) {
            const int64_t at = (int64_t)(y0 + (int)(q / bw)) * w + x0 + (int)(q % bw);
            const float g = (float)gt[at] / divisor;
            if (!(g > min_depth && g < max_depth)) continue;
            float p = (float)pred[at] / divisor;
            p = p < min_depth ? min_depth : p;
            p = p > max_depth ? max_depth : p;
            const float t = fmaxf(g / p, p / g);
            a.n += 1u;
            a.c1 += t < 1.25f ? 1u : 0u;
            a.c2 += t < 1.5625f ? 1u : 0u;
            a.c3 += t < 1.953125f ? 1u : 0u;
            const double gd = (double)g, pd = (double)p, d = gd - pd, lg = log(gd), lp = log(pd), dl = lg - lp;
            a.s[0] += d * d;
            a.s[1] += dl * dl;
            a.s[2] += fabs(d) / gd;
            a.s[3] += (d * d) / gd;
            a.s[4] += lp - lg;
            a.s[5] += fabs(log10(pd) - log10(gd));
        }
    }
    depth_wave_sum(a);
    if (lane == 0) {
        s_part[wave][0] = (double)a.n; s_part[wave][1] = (double)a.c1; s_part[wave][2] = (double)a.c2; s_part[wave][3] = (double)a.c3;
#pragma unroll
        for (int k = 0; k < 6; ++k) s_part[wave][4 + k] = a.s[k];
    }
    __syncthreads();
    if (tid < DEPTH_OUT) {
        double v = s_part[0][tid];
        for (int k = 1; k < DEPTH_THREADS / 64; ++k) v += s_part[k][tid];
        partials[((int64_t)j * DEPTH_PARTS + blockIdx.x) * DEPTH_OUT + tid] = v;
    }
}

// One thread per (job, number): the partials of a job in index order.
__global__ __launch_bounds__(256) void depth_reduce_kernel(const double* __restrict__ partials, double* __restrict__ out, int n_values) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_values) return;
    const int j = i / DEPTH_OUT, k = i % DEPTH_OUT;
    double v = partials[(int64_t)j * DEPTH_PARTS * DEPTH_OUT + k];
    for (int part = 1; part < DEPTH_PARTS; ++part) v += partials[((int64_t)j * DEPTH_PARTS + part) * DEPTH_OUT + k];
    out[i] = v;
}

}  // namespace

extern "C" {

int pa_semseg_lds_bins(int n_colours) { return n_colours >= 1 && n_colours <= 255 && conf_lds_bytes(n_colours) <= LDS_BYTES ? 1 : 0; }

int pa_semseg_confusion(const pa_score_job* jobs, int n_jobs, int64_t total_pixels, const float* palette, int n_colours, int dist_type,
                        int ignore_label, int bins, void* conf_i64, void* invalid_i64, hipStream_t stream) {
    if (!jobs || !palette || !conf_i64 || !invalid_i64 || n_jobs < 1 || n_jobs > 65535 || total_pixels < 1 ||
        total_pixels > MAX_LAUNCH_PIXELS || n_colours < 1 || n_colours > 255 || dist_type < 0 || dist_type > 2 || bins < 0 || bins > 1 ||
        (((uintptr_t)conf_i64 | (uintptr_t)invalid_i64) & 7) != 0)
        return (int)hipErrorInvalidValue;
    const bool lds_bins = bins == 0 && pa_semseg_lds_bins(n_colours);
    u64* conf = (u64*)conf_i64;
    u64* invalid = (u64*)invalid_i64;
    if (dist_type == 0) return launch_confusion<0>(jobs, n_jobs, total_pixels, palette, n_colours, ignore_label, lds_bins, conf, invalid, stream);
    if (dist_type == 1) return launch_confusion<1>(jobs, n_jobs, total_pixels, palette, n_colours, ignore_label, lds_bins, conf, invalid, stream);
    return launch_confusion<2>(jobs, n_jobs, total_pixels, palette, n_colours, ignore_label, lds_bins, conf, invalid, stream);
}

int64_t pa_depth_workspace_bytes(int n_jobs) {
    if (n_jobs < 1 || n_jobs > 65535) return -1;
    return (int64_t)n_jobs * DEPTH_PARTS * DEPTH_OUT * 8;
}

int pa_depth_errors(const pa_depth_job* jobs, int n_jobs, float divisor, float min_depth, float max_depth, void* out_f64, void* workspace,
                    hipStream_t stream) {
    if (!jobs || !out_f64 || !workspace || n_jobs < 1 || n_jobs > 65535 || !(divisor > 0.f) || !(divisor < INFINITY) ||
        !(min_depth < max_depth) || !(min_depth > 0.f) || !(max_depth < INFINITY) || (((uintptr_t)out_f64 | (uintptr_t)workspace) & 7) != 0)
        return (int)hipErrorInvalidValue;
    PA_LAUNCH_TRY(depth_errors_kernel, dim3(DEPTH_PARTS, (unsigned)n_jobs), dim3(DEPTH_THREADS), 0, stream, jobs, divisor, min_depth,
                  max_depth, (double*)workspace);
    const int n_values = n_jobs * DEPTH_OUT;
    PA_LAUNCH(depth_reduce_kernel, dim3((unsigned)((n_values + 255) / 256)), dim3(256), 0, stream, (const double*)workspace, (double*)out_f64,
              n_values);
    LAUNCH_CHECK();
}

}  // extern "C"
