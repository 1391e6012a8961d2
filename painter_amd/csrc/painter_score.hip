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
//   boundary  : the evaluators' boundary-IoU branch (ADE20kSemSegEvaluatorCustom.py:103-110, COCOPanoSemSegEvaluatorCustom.py:97-104;
//               detectron2's _compute_boundary_iou restated, unverified against detectron2 / cv2): both label maps are eroded d times by a
//               3 x 3 square behind a ring of zeros -- ONE minimum over a (2d + 1)^2 window with everything outside the picture read as 0
//               -- and bconf[(K + 1) * (pred - eroded pred) + (gt' - eroded gt')] += 1.  Three launches over the job table, each job with
//               its own d, on four byte maps of the workspace:
//                 1. the confusion kernel above with SIDE = true: the arg-min is evaluated once, counted into `conf` as ever and written
//                    with gt' as bytes (maps 0, 1; a job's pixels start where the earlier jobs' end).
//                 2. row minimum (maps 2, 3): a WAVE takes T = min(64, 2d + 1) consecutive outputs of a row.  Every one of their windows
//                    holds the columns lo = x0 + T - 1 - d .. hi = x0 + d (T <= 2d + 1, so there is at least one), which the lanes stream
//                    and reduce; output i adds the T - 1 - i columns left of lo that are its own -- a suffix minimum over the lanes, one
//                    load per lane, six shuffles -- and the i columns right of hi, a prefix minimum (van Herk / Gil-Werman with the
//                    wave as the block).  1 + 2d / T loads per output: about 2 up to d = 31, 1 + d / 32 from there.
//                 3. column minimum and count: a thread owns a column, a wave 64 consecutive columns and R = min(32, 2d + 1) output
//                    rows.  The same split down the column: the R - 1 suffix minima of the rows above lo stay in registers, the rows
//                    lo .. hi common to all R windows are streamed once (any d: nothing is staged in LDS, so nothing caps it), then
//                    one row per output for the prefix minimum; 1 + 2d / R loads per output and map (about 2 up to d = 15, 1 + d / 16
//                    from there) and the centre, each row read by 64 lanes at consecutive bytes.  An output row is then 64 consecutive
//                    pixels in the lanes, so the runs fold as above ((0, 0) is the hot bin: a wave inside a region adds 64 once) into
//                    (K + 1)^2 private 32-bit LDS bins, or straight to `bconf`.
//               pa_label_boundary runs 2 and 3 on one map through the same device functions and stores centre - minimum instead.
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

// The side outputs of the confusion kernel (SIDE): a pixel's class and gt' as bytes, job after job; `capacity` pixels fit.
struct SideMaps {
    uint8_t* pred;
    uint8_t* gt;
    int64_t capacity;
};

// Runs of equal keys among the wave's lanes (every lane of the wave calls this): the head of a run adds its length.
template <bool BINS_IN_LDS> DEVI void count_runs(int key, int lane, uint32_t* bins, u64* __restrict__ conf) {
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

// JOB: pa_score_job, or with SIDE pa_boundary_job (the same first four fields).
template <int DIST, bool BINS_IN_LDS, typename JOB, bool SIDE>
__global__ __launch_bounds__(CONF_THREADS) void semseg_confusion_kernel(const JOB* __restrict__ jobs, int n_jobs,
                                                                        const float* __restrict__ palette, int K, int ignore_label,
                                                                        u64* __restrict__ conf, u64* __restrict__ invalid, SideMaps side) {
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
    int64_t pix0 = 0;                                             // SIDE: number of this job's first pixel in the maps
    for (int j = 0; j < n_jobs; ++j) {                            // every branch on j, c is uniform over the workgroup
        const int h = jobs[j].h, w = jobs[j].w;
        if (h < 1 || w < 1) continue;
        const uint8_t* __restrict__ pic = static_cast<const uint8_t*>(jobs[j].picture);
        const uint8_t* __restrict__ gt = static_cast<const uint8_t*>(jobs[j].gt);
        const int64_t npix = (int64_t)h * w, n_chunks = (npix + CONF_THREADS - 1) / CONF_THREADS;
        const bool mapped = SIDE && pix0 + npix <= side.capacity;  // a table that holds more than total_pixels: counted, not mapped
        for (int64_t c = ((int64_t)blockIdx.x - chunk0 % G + G) % G; c < n_chunks; c += G) {
            const int64_t p = c * CONF_THREADS + tid;
            int key = KEY_NONE;
            if (p < npix) {
                const int g = gt[p];
                const int pred = nearest_colour<DIST>((float)pic[3 * p], (float)pic[3 * p + 1], (float)pic[3 * p + 2], pal, K);
                key = g == ignore_label ? pred * (K + 1) + K : (g < K ? pred * (K + 1) + g : KEY_INVALID);
                if (mapped) {
                    side.pred[pix0 + p] = (uint8_t)pred;
                    side.gt[pix0 + p] = (uint8_t)(g < K && g != ignore_label ? g : K);
                }
            }
            bad += key == KEY_INVALID ? 1u : 0u;
            count_runs<BINS_IN_LDS>(key, lane, bins, conf);
        }
        chunk0 += n_chunks;
        pix0 += npix;
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

template <int DIST, typename JOB, bool SIDE>
int launch_confusion(const JOB* jobs, int n_jobs, int64_t total, const float* palette, int K, int ignore_label, bool lds_bins,
                     u64* conf, u64* invalid, SideMaps side, hipStream_t stream) {
    const int64_t chunks = (total + CONF_THREADS - 1) / CONF_THREADS;
    // two workgroups of 1024 threads fill a CU; bins beyond 80 KB leave room for one
    const int64_t resident = CONF_CUS * (lds_bins && 2 * conf_lds_bytes(K) > LDS_BYTES ? 1 : 2);
    const dim3 grid((unsigned)(chunks < resident ? chunks : resident));
    if (lds_bins) {
        static bool attr_done = false;
        if (!attr_done) {
            PA_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(semseg_confusion_kernel<DIST, true, JOB, SIDE>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
            attr_done = true;
        }
        PA_LAUNCH((semseg_confusion_kernel<DIST, true, JOB, SIDE>), grid, dim3(CONF_THREADS), (size_t)conf_lds_bytes(K), stream, jobs,
                  n_jobs, palette, K, ignore_label, conf, invalid, side);
    } else {
        PA_LAUNCH((semseg_confusion_kernel<DIST, false, JOB, SIDE>), grid, dim3(CONF_THREADS), (size_t)up16(12 * (int64_t)K), stream, jobs,
                  n_jobs, palette, K, ignore_label, conf, invalid, side);
    }
    LAUNCH_CHECK();
}

// ---- the boundary branch: window minimum of byte maps, everything outside the picture read as 0
constexpr int ERODE_THREADS = 256, ERODE_WAVES = ERODE_THREADS / 64;
constexpr int STRIP_ROWS = 32;                    // output rows of a column strip: their suffix minima live in registers
constexpr int ERODE_WGS = 256 * 8;                // eight workgroups of four waves per CU

DEVI int mini(int a, int b) { return b < a ? b : a; }

// NMAPS bytes, one per map, each in its own 16 bits of a word; min_each is the minimum per map.
template <int NMAPS> DEVI uint32_t min_each(uint32_t a, uint32_t b) {
    uint32_t r = (uint32_t)mini((int)(a & 0xffffu), (int)(b & 0xffffu));
    if (NMAPS == 2) r |= (uint32_t)mini((int)(a >> 16), (int)(b >> 16)) << 16;
    return r;
}
constexpr uint32_t EACH_255 = 0x00ff00ffu;

// The minimum of row[x - d .. x + d] for the T = min(64, 2d + 1) outputs x = x0 + lane of a wave (every lane calls this; lanes >= T get
// something).  a: the T - 1 columns left of lo, suffix minimum over the lanes; b: the T - 1 columns right of hi, prefix minimum; c: lo .. hi,
// common to all T windows -- 0 at once where it leaves the row.  Output i's window is a[i ..] + c + b[.. i], nothing else is looked at.
DEVI int row_min_tile(const uint8_t* __restrict__ row, int64_t w, int64_t d, int64_t x0, int T, int lane) {
    const int64_t ia = x0 - d + lane, ib = x0 + d + lane, lo = x0 + T - 1 - d, hi = x0 + d;
    int a = lane < T - 1 ? (ia < 0 || ia >= w ? 0 : (int)row[ia]) : 255;
    int b = lane >= 1 && lane < T ? (ib >= w ? 0 : (int)row[ib]) : 255;
    int c = lo < 0 || hi >= w ? 0 : 255;
    if (c)
        for (int64_t k = lo + lane; k <= hi; k += 64) c = mini(c, (int)row[k]);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {                      // a shuffle past the wave's end returns the lane's own value
        a = mini(a, __shfl_down(a, off, 64));
        b = mini(b, __shfl_up(b, off, 64));
        c = mini(c, __shfl_xor(c, off, 64));
    }
    return mini(mini(a, b), c);
}

// Pass 2 for one picture: out[m] = row minimum of in[m].  Units = (row, tile of T columns), numbered from unit0 through the launch; wave gw
// of GW takes every GW-th.  -> the picture's number of units.
template <int NMAPS>
DEVI int64_t erode_rows(const uint8_t* const (&in)[NMAPS], uint8_t* const (&out)[NMAPS], int64_t h, int64_t w, int64_t d, int64_t unit0,
                        int64_t gw, int64_t GW, int lane) {
    const int T = d >= 32 ? 64 : 2 * (int)d + 1;
    const int64_t tiles = (w + T - 1) / T, units = h * tiles;
    for (int64_t u = (gw - unit0 % GW + GW) % GW; u < units; u += GW) {
        const int64_t y = u / tiles, x0 = (u % tiles) * T;
#pragma unroll
        for (int m = 0; m < NMAPS; ++m) {
            const int v = row_min_tile(in[m] + y * w, w, d, x0, T, lane);
            if (lane < T && x0 + lane < w) out[m][y * w + x0 + lane] = (uint8_t)v;
        }
    }
    return units;
}

// The minimum of rows y - d .. y + d of column x of the row-minimum maps rm[m], for the R <= STRIP_ROWS output rows y = y0 .. y0 + R - 1
// (R <= 2d + 1), one thread: emit(y, minima) is called for every y < h in rising order, by every lane of the wave (`live`: the lane has a
// column), so that emit may shuffle.  The split of row_min_tile, down the column: sa[i] = the rows above lo that output i sees.
template <int NMAPS, class Emit>
DEVI void col_min_strip(const uint8_t* const (&rm)[NMAPS], int64_t h, int64_t w, int64_t d, int64_t y0, int R, int64_t x, bool live, Emit emit) {
    const int64_t first = y0 > d ? y0 : d, last = y0 + R - 1 < h - 1 - d ? y0 + R - 1 : h - 1 - d;      // the rows whose window stays inside
    if (first > last) {
        for (int i = 0; i < R && y0 + i < h; ++i) emit(y0 + i, 0u);
        return;
    }
    auto at = [&](int64_t r) -> uint32_t {
        if (!live || r < 0 || r >= h) return 0u;
        uint32_t v = rm[0][r * w + x];
        if (NMAPS == 2) v |= (uint32_t)rm[NMAPS - 1][r * w + x] << 16;
        return v;
    };
    uint32_t sa[STRIP_ROWS], run = EACH_255;
#pragma unroll
    for (int i = STRIP_ROWS - 1; i >= 0; --i) {
        if (i < R - 1) run = min_each<NMAPS>(run, at(y0 - d + i));
        sa[i] = run;
    }
    const int64_t lo = y0 + R - 1 - d, hi = y0 + d;
    uint32_t c = lo < 0 || hi >= h ? 0u : EACH_255;
    if (c)
        for (int64_t r = lo; r <= hi; ++r) c = min_each<NMAPS>(c, at(r));
    run = EACH_255;
#pragma unroll
    for (int i = 0; i < STRIP_ROWS; ++i) {
        if (i < R && y0 + i < h) {
            if (i >= 1) run = min_each<NMAPS>(run, at(y0 + d + i));
            emit(y0 + i, min_each<NMAPS>(min_each<NMAPS>(sa[i], c), run));
        }
    }
}

// Pass 3 for one picture.  Units = (strip of R rows, 64 columns), numbered and dealt to the waves as in erode_rows.
template <int NMAPS, class Emit>
DEVI int64_t erode_cols(const uint8_t* const (&rm)[NMAPS], int64_t h, int64_t w, int64_t d, int64_t unit0, int64_t gw, int64_t GW, int lane,
                        Emit emit) {
    const int R = d >= STRIP_ROWS / 2 ? STRIP_ROWS : 2 * (int)d + 1;
    const int64_t groups = (w + 63) / 64, units = (h + R - 1) / R * groups;
    for (int64_t u = (gw - unit0 % GW + GW) % GW; u < units; u += GW) {
        const int64_t x = (u % groups) * 64 + lane;
        col_min_strip<NMAPS>(rm, h, w, d, (u / groups) * R, R, x, x < w, [&](int64_t y, uint32_t m) { emit(y, x, x < w, m); });
    }
    return units;
}

// maps: four byte maps of `plane` bytes each -- pred, gt', and their row minima.
__global__ __launch_bounds__(ERODE_THREADS) void boundary_rows_kernel(const pa_boundary_job* __restrict__ jobs, int n_jobs, int64_t capacity,
                                                                      uint8_t* __restrict__ maps, int64_t plane) {
    const int lane = threadIdx.x & 63;
    const int64_t gw = (int64_t)blockIdx.x * ERODE_WAVES + (threadIdx.x >> 6), GW = (int64_t)gridDim.x * ERODE_WAVES;
    int64_t unit0 = 0, pix0 = 0;
    for (int j = 0; j < n_jobs; ++j) {                            // every branch on j, u is uniform over the wave
        const int64_t h = jobs[j].h, w = jobs[j].w, d = jobs[j].d;
        if (h < 1 || w < 1) continue;
        if (pix0 + h * w > capacity) break;
        if (d >= 1) {
            const uint8_t* const in[2] = {maps + pix0, maps + plane + pix0};
            uint8_t* const out[2] = {maps + 2 * plane + pix0, maps + 3 * plane + pix0};
            unit0 += erode_rows<2>(in, out, h, w, d, unit0, gw, GW, lane);
        }
        pix0 += h * w;
    }
}

template <bool BINS_IN_LDS>
__global__ __launch_bounds__(ERODE_THREADS) void boundary_count_kernel(const pa_boundary_job* __restrict__ jobs, int n_jobs, int64_t capacity,
                                                                       const uint8_t* __restrict__ maps, int64_t plane, int K,
                                                                       u64* __restrict__ bconf) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint32_t* bins = reinterpret_cast<uint32_t*>(smem);
    const int tid = threadIdx.x, lane = tid & 63, n_bins = (K + 1) * (K + 1);
    if (BINS_IN_LDS) {
        for (int i = tid; i < n_bins; i += ERODE_THREADS) bins[i] = 0u;
        __syncthreads();
    }
    const int64_t gw = (int64_t)blockIdx.x * ERODE_WAVES + (tid >> 6), GW = (int64_t)gridDim.x * ERODE_WAVES;
    int64_t unit0 = 0, pix0 = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const int64_t h = jobs[j].h, w = jobs[j].w, d = jobs[j].d;
        if (h < 1 || w < 1) continue;
        if (pix0 + h * w > capacity) break;
        if (d >= 1) {
            const uint8_t* __restrict__ pred = maps + pix0;
            const uint8_t* __restrict__ gt = maps + plane + pix0;
            const uint8_t* const rm[2] = {maps + 2 * plane + pix0, maps + 3 * plane + pix0};
            unit0 += erode_cols<2>(rm, h, w, d, unit0, gw, GW, lane, [&](int64_t y, int64_t x, bool live, uint32_t m) {
                // centre - minimum >= 0: the window holds the centre
                const int key = live ? (K + 1) * ((int)pred[y * w + x] - (int)(m & 0xffffu)) + ((int)gt[y * w + x] - (int)(m >> 16)) : KEY_NONE;
                count_runs<BINS_IN_LDS>(key, lane, bins, bconf);
            });
        }
        pix0 += h * w;
    }
    if (BINS_IN_LDS) {
        __syncthreads();
        for (int i = tid; i < n_bins; i += ERODE_THREADS) {
            const uint32_t v = bins[i];
            if (v) atomicAdd(&bconf[i], (u64)v);
        }
    }
}

__global__ __launch_bounds__(ERODE_THREADS) void label_rows_kernel(const uint8_t* __restrict__ map, int h, int w, int d, uint8_t* __restrict__ rowmin) {
    const uint8_t* const in[1] = {map};
    uint8_t* const out[1] = {rowmin};
    erode_rows<1>(in, out, h, w, d, 0, (int64_t)blockIdx.x * ERODE_WAVES + (threadIdx.x >> 6), (int64_t)gridDim.x * ERODE_WAVES, threadIdx.x & 63);
}

__global__ __launch_bounds__(ERODE_THREADS) void label_cols_kernel(const uint8_t* __restrict__ map, const uint8_t* __restrict__ rowmin, int h, int w,
                                                                   int d, uint8_t* __restrict__ boundary) {
    const uint8_t* const rm[1] = {rowmin};
    erode_cols<1>(rm, h, w, d, 0, (int64_t)blockIdx.x * ERODE_WAVES + (threadIdx.x >> 6), (int64_t)gridDim.x * ERODE_WAVES, threadIdx.x & 63,
                  [&](int64_t y, int64_t x, bool live, uint32_t m) {
                      if (live) boundary[y * w + x] = (uint8_t)((int)map[y * w + x] - (int)m);
                  });
}

// The grid of passes 2 and 3: a unit is at most 64 x STRIP_ROWS pixels; what is resident at once bounds it.
inline unsigned erode_grid(int64_t pixels, int64_t resident) {
    const int64_t wgs = (pixels + 64 * ERODE_WAVES - 1) / (64 * ERODE_WAVES);
    return (unsigned)(wgs < resident ? wgs : resident);
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
    const SideMaps none = {nullptr, nullptr, 0};
    if (dist_type == 0)
        return launch_confusion<0, pa_score_job, false>(jobs, n_jobs, total_pixels, palette, n_colours, ignore_label, lds_bins, conf, invalid, none, stream);
    if (dist_type == 1)
        return launch_confusion<1, pa_score_job, false>(jobs, n_jobs, total_pixels, palette, n_colours, ignore_label, lds_bins, conf, invalid, none, stream);
    return launch_confusion<2, pa_score_job, false>(jobs, n_jobs, total_pixels, palette, n_colours, ignore_label, lds_bins, conf, invalid, none, stream);
}

int64_t pa_semseg_boundary_workspace_bytes(int64_t total_pixels) {
    if (total_pixels < 1 || total_pixels > MAX_LAUNCH_PIXELS) return -1;
    return 4 * up16(total_pixels);
}

int pa_semseg_boundary_confusion(const pa_boundary_job* jobs, int n_jobs, int64_t total_pixels, const float* palette, int n_colours,
                                 int dist_type, int ignore_label, int bins, void* conf_i64, void* bconf_i64, void* invalid_i64,
                                 void* workspace, hipStream_t stream) {
    if (!jobs || !palette || !conf_i64 || !bconf_i64 || !invalid_i64 || !workspace || n_jobs < 1 || n_jobs > 65535 || total_pixels < 1 ||
        total_pixels > MAX_LAUNCH_PIXELS || n_colours < 1 || n_colours > 254 || dist_type < 0 || dist_type > 2 || bins < 0 || bins > 1 ||
        (((uintptr_t)conf_i64 | (uintptr_t)bconf_i64 | (uintptr_t)invalid_i64) & 7) != 0)
        return (int)hipErrorInvalidValue;
    const bool lds_bins = bins == 0 && pa_semseg_lds_bins(n_colours);
    const int K = n_colours;
    u64* conf = (u64*)conf_i64;
    u64* bconf = (u64*)bconf_i64;
    u64* invalid = (u64*)invalid_i64;
    uint8_t* maps = (uint8_t*)workspace;
    const int64_t plane = up16(total_pixels);
    const SideMaps side = {maps, maps + plane, total_pixels};
    if (dist_type == 0)
        PA_TRY((launch_confusion<0, pa_boundary_job, true>(jobs, n_jobs, total_pixels, palette, K, ignore_label, lds_bins, conf, invalid, side, stream)));
    else if (dist_type == 1)
        PA_TRY((launch_confusion<1, pa_boundary_job, true>(jobs, n_jobs, total_pixels, palette, K, ignore_label, lds_bins, conf, invalid, side, stream)));
    else
        PA_TRY((launch_confusion<2, pa_boundary_job, true>(jobs, n_jobs, total_pixels, palette, K, ignore_label, lds_bins, conf, invalid, side, stream)));
    PA_LAUNCH_TRY(boundary_rows_kernel, dim3(erode_grid(total_pixels, ERODE_WGS)), dim3(ERODE_THREADS), 0, stream, jobs, n_jobs, total_pixels,
                  maps, plane);
    if (lds_bins) {
        const int64_t bin_bytes = 4 * (int64_t)(K + 1) * (K + 1), per_cu = LDS_BYTES / bin_bytes;
        static bool attr_done = false;
        if (!attr_done) {
            PA_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(boundary_count_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       LDS_BYTES));
            attr_done = true;
        }
        PA_LAUNCH((boundary_count_kernel<true>), dim3(erode_grid(total_pixels, CONF_CUS * (per_cu < 8 ? per_cu : 8))), dim3(ERODE_THREADS),
                  (size_t)bin_bytes, stream, jobs, n_jobs, total_pixels, maps, plane, K, bconf);
    } else {
        PA_LAUNCH((boundary_count_kernel<false>), dim3(erode_grid(total_pixels, ERODE_WGS)), dim3(ERODE_THREADS), 0, stream, jobs, n_jobs,
                  total_pixels, maps, plane, K, bconf);
    }
    LAUNCH_CHECK();
}

int pa_label_boundary(const void* map_u8, int h, int w, int d, void* out_u8, void* workspace, hipStream_t stream) {
    if (!map_u8 || !out_u8 || !workspace || h < 1 || w < 1 || d < 1 || (int64_t)h * w > MAX_LAUNCH_PIXELS) return (int)hipErrorInvalidValue;
    const unsigned grid = erode_grid((int64_t)h * w, ERODE_WGS);
    PA_LAUNCH_TRY(label_rows_kernel, dim3(grid), dim3(ERODE_THREADS), 0, stream, (const uint8_t*)map_u8, h, w, d, (uint8_t*)workspace);
    PA_LAUNCH(label_cols_kernel, dim3(grid), dim3(ERODE_THREADS), 0, stream, (const uint8_t*)map_u8, (const uint8_t*)workspace, h, w, d,
              (uint8_t*)out_u8);
    LAUNCH_CHECK();
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
