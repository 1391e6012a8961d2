// Instance decode by nearest colour on the device: the evaluator's `post_type="minmax"` route
// (Painter/eval/coco_panoptic/COCOCAInstSegEvaluatorCustom.py:172-250, post_process_segm_output_by_minmax), which the reference runs as four
// [H/4][W][K][3] float32 difference tensors, one torch.min, one boolean mask and one torch.mean per colour found and a float32 [n][H][W]
// mask stack -- restated on integers (include/painter_minmax.h states the definitions, tests/painter_minmax_host.py is the statement):
//
//   nearest : label(p) = lowest c with minimal L1(p, c), dist(p) = that L1.  The palette sits in LDS as one packed dword per colour
//             (R | G << 8 | B << 16); a thread keeps its pixel as a packed dword; one wave-uniform 16-byte LDS read (a broadcast) brings
//             four colours; an update is v_sad_hi_u8 -- (L1 << 16) + c in ONE instruction -- and an unsigned minimum (v_min3_u32 takes
//             two keys at once), so a lower index wins a tie at no cost: 1.75 VALU operations per (pixel, colour).
//   stats   : n_c, S_c from the label and distance maps: runs of equal labels are folded in the wave (ballot + prefix sum), added to the
//             workgroup's private LDS bins, and the non-empty bins leave as integer atomics (n: 32 bits, S: 64 bits).
//   compact : ONE workgroup scans the K presence flags: count, one record per instance in ascending colour, the colour -> slot table;
//             neg = (float)((double)S / n), their maximum by an integer maximum over the (non-negative) float bits, the score.
//   masks   : one thread per 32-pixel word of the picture: its pixels belong to at most 32 slots, it alone writes word w of every row.
//
// Everything is stream-ordered and allocates nothing; the instance count stays on the device.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/painter_minmax.h"
#include "painter_post.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAX_SIDE = 16384;          // h, w
constexpr int64_t MAX_PIX = 1 << 24;     // h * w: S <= 765 * 2^24 < 2^34
constexpr int MAX_COL = 16384;           // K with the background row: a packed palette is 64 KiB of LDS, a label fits 16 bits
constexpr int TPB = 256;
constexpr int PPT = 1;                   // pixels a thread of the nearest kernel owns.  Measured at 480 x 640 x 6401: 0.205 / 0.146 / 0.118 ms
                                         // for 4 / 2 / 1 (1080 x 1920: 0.667 / 0.648 / 0.649): the loop is VALU-bound, the 16-byte broadcast
                                         // read hides behind 7 VALU operations, and 1200 small workgroups balance over 256 CUs where 300 do not
constexpr int STAT_CHUNK = 2048;         // pixels per statistics workgroup: its private sums stay below 2^21
constexpr int STAT_BINS = 8192;          // colours per statistics workgroup (blockIdx.y picks the range): 64 KiB of LDS

bool shape_ok(int h, int w, int K) {
    return h >= 1 && w >= 1 && h <= MAX_SIDE && w <= MAX_SIDE && (int64_t)h * w <= MAX_PIX && K >= 1 && K <= MAX_COL;
}

// grid: x = blocks of TPB * PPT pixels.  Dynamic LDS: kpad dwords, kpad = K rounded up to 4; the padding repeats colour K - 1 under an
// index >= K, which never beats colour K - 1 itself.
__global__ __launch_bounds__(TPB) void minmax_nearest_kernel(const uint8_t* __restrict__ pic, const float* __restrict__ pal,
                                                             uint16_t* __restrict__ label, uint16_t* __restrict__ dist, int64_t npix, int K,
                                                             int kpad) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_pal[];
    const int tid = threadIdx.x;
    for (int c = tid; c < kpad; c += TPB) s_pal[c] = pack_colour(pal, c < K ? c : K - 1);
    const int64_t base = (int64_t)blockIdx.x * (TPB * PPT) + tid;
    uint32_t px[PPT], best[PPT];
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int64_t p = base + j * TPB;
        px[j] = p < npix ? pack_pixel(pic, p) : 0u;
        best[j] = 0xFFFFFFFFu;
    }
    __syncthreads();
    for (int c = 0; c < kpad; c += 4) {
        const uint4 q = *(const uint4*)&s_pal[c];
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            const uint32_t k0 = __builtin_amdgcn_sad_hi_u8(px[j], q.x, (uint32_t)c), k1 = __builtin_amdgcn_sad_hi_u8(px[j], q.y, (uint32_t)c + 1u);
            const uint32_t k2 = __builtin_amdgcn_sad_hi_u8(px[j], q.z, (uint32_t)c + 2u), k3 = __builtin_amdgcn_sad_hi_u8(px[j], q.w, (uint32_t)c + 3u);
            best[j] = min(min(best[j], min(k0, k1)), min(k2, k3));
        }
    }
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int64_t p = base + j * TPB;
        if (p < npix) {
            label[p] = (uint16_t)(best[j] & 0xFFFFu);
            dist[p] = (uint16_t)(best[j] >> 16);
        }
    }
}

// grid: x = chunks of STAT_CHUNK pixels, y = ranges of STAT_BINS colours.
__global__ __launch_bounds__(TPB) void minmax_stats_kernel(const uint16_t* __restrict__ label, const uint16_t* __restrict__ dist,
                                                           uint32_t* __restrict__ cnt, u64* __restrict__ sum, int64_t npix, int K) {
    __shared__ uint32_t s_cnt[STAT_BINS];
    __shared__ uint32_t s_sum[STAT_BINS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int c0 = blockIdx.y * STAT_BINS, nb = K - c0 < STAT_BINS ? K - c0 : STAT_BINS;
    for (int i = tid; i < nb; i += TPB) {
        s_cnt[i] = 0u;
        s_sum[i] = 0u;
    }
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * STAT_CHUNK;
    for (int i = 0; i < STAT_CHUNK; i += TPB) {                 // (every lane of a wave takes part in the shuffles of every round)
        const int64_t p = base + i + tid;
        const uint32_t l = p < npix ? (uint32_t)label[p] : 0xFFFFFFFFu;
        const uint32_t d = p < npix ? (uint32_t)dist[p] : 0u;
        const uint32_t prev = __shfl_up(l, 1);
        const bool head = lane == 0 || prev != l;
        uint32_t pre = d;                                       // inclusive prefix sum of d over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = __shfl_up(pre, o);
            if (lane >= o) pre += t;
        }
        const u64 heads = __ballot(head);
        const u64 above = lane == 63 ? 0ull : heads >> (lane + 1);
        const int next = above ? lane + __ffsll((long long)above) : 64;          // the lane at which the next run starts
        const uint32_t end = __shfl(pre, next - 1);
        const uint32_t bin = l - (uint32_t)c0;                  // (wraps for a label below the range and for the sentinel)
        if (head && bin < (uint32_t)nb) {
            atomicAdd(&s_cnt[bin], (uint32_t)(next - lane));
            atomicAdd(&s_sum[bin], end - (pre - d));
        }
    }
    __syncthreads();
    for (int i = tid; i < nb; i += TPB) {
        const uint32_t n = s_cnt[i];
        if (n) {
            atomicAdd(&cnt[c0 + i], n);
            atomicAdd(&sum[c0 + i], (u64)s_sum[i]);
        }
    }
}

DEVI float neg_of(u64 s, uint32_t n) { return (float)((double)s / (double)n); }

// One workgroup.  A thread owns the colours [tid * per, tid * per + per).
__global__ __launch_bounds__(TPB) void minmax_compact_kernel(const uint32_t* __restrict__ cnt, const u64* __restrict__ sum,
                                                             int* __restrict__ count, pa_minmax_record* __restrict__ rec,
                                                             int* __restrict__ slot, int K) {
    __shared__ int s_scan[TPB];
    __shared__ uint32_t s_max;
    const int tid = threadIdx.x, per = (K + TPB - 1) / TPB;
    const int lo = min(tid * per, K), hi = min(lo + per, K);
    if (tid == 0) s_max = 0u;
    __syncthreads();
    int mine = 0;
    uint32_t top = 0u;                                          // neg >= 0: the order of the floats is the order of their bits
    for (int c = lo; c < hi; ++c) {
        const uint32_t n = cnt[c];
        if (n) {
            ++mine;
            top = max(top, __float_as_uint(neg_of(sum[c], n)));
        }
    }
    s_scan[tid] = mine;
    if (top) atomicMax(&s_max, top);
    __syncthreads();
    for (int o = 1; o < TPB; o <<= 1) {                         // inclusive scan
        const int t = tid >= o ? s_scan[tid - o] : 0;
        __syncthreads();
        s_scan[tid] += t;
        __syncthreads();
    }
    if (tid == TPB - 1) count[0] = s_scan[tid];
    const float m = fmaxf(__uint_as_float(s_max), 1.0f);
    int at = s_scan[tid] - mine;
    for (int c = lo; c < hi; ++c) {
        const uint32_t n = cnt[c];
        if (!n) {
            slot[c] = -1;
            continue;
        }
        const u64 s = sum[c];
        const float neg = neg_of(s, n);
        const float ratio = neg / m;
        pa_minmax_record r;
        r.colour = c;
        r.cls = c == K - 1 ? 0 : 1;
        r.n = n;
        r.reserved = 0u;
        r.S = s;
        r.neg = neg;
        r.score = 1.0f - ratio;
        rec[at] = r;
        slot[c] = at++;
    }
}

// One thread per 32-pixel word of the picture.
__global__ __launch_bounds__(TPB) void minmax_masks_kernel(const uint16_t* __restrict__ label, const int* __restrict__ slot,
                                                           uint32_t* __restrict__ bits, uint8_t* __restrict__ bytes, int64_t npix, int words,
                                                           int K, int first, int n_cap) {
    const int64_t wi = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (wi >= words) return;
    const int64_t p0 = wi * 32;
    const int valid = (int)(npix - p0 < 32 ? npix - p0 : 32);
    int cur = -1;
    uint32_t acc = 0u;
    for (int j = 0; j < valid; ++j) {
        const uint32_t l = label[p0 + j];
        int s = l < (uint32_t)K ? slot[l] : -1;
        s = s >= first && s - first < n_cap ? s - first : -1;
        if (s != cur) {
            if (cur >= 0) bits[(int64_t)cur * words + wi] |= acc;           // (this thread owns word wi of every row)
            cur = s;
            acc = 0u;
        }
        acc |= 1u << j;
        if (bytes && s >= 0) bytes[(int64_t)s * npix + p0 + j] = 1;
    }
    if (cur >= 0) bits[(int64_t)cur * words + wi] |= acc;
}

int launch_nearest(const void* image, const void* palette, int h, int w, int K, void* out_label, void* out_dist, hipStream_t stream) {
    const int64_t npix = (int64_t)h * w;
    const int kpad = (K + 3) & ~3;
    const unsigned blocks = (unsigned)((npix + TPB * PPT - 1) / (TPB * PPT));
    PA_LAUNCH(minmax_nearest_kernel, dim3(blocks), dim3(TPB), 4 * (size_t)kpad, stream, (const uint8_t*)image, (const float*)palette,
              (uint16_t*)out_label, (uint16_t*)out_dist, npix, K, kpad);
    LAUNCH_CHECK();
}

}  // namespace

extern "C" {

int pa_minmax_nearest(const void* image, const void* palette, int h, int w, int n_colours, void* out_label, void* out_dist,
                      hipStream_t stream) {
    if (!image || !palette || !out_label || !out_dist || !shape_ok(h, w, n_colours) || ((uintptr_t)palette & 3) || ((uintptr_t)out_label & 1) ||
        ((uintptr_t)out_dist & 1))
        return (int)hipErrorInvalidValue;
    return launch_nearest(image, palette, h, w, n_colours, out_label, out_dist, stream);
}

int64_t pa_minmax_workspace_bytes(int h, int w, int n_colours) {
    if (!shape_ok(h, w, n_colours)) return -1;
    return up16(8 * (int64_t)n_colours) + up16(4 * (int64_t)n_colours);
}

int pa_minmax_decode(const void* image, const void* palette, int h, int w, int n_colours, void* workspace, void* out_label, void* out_dist,
                     void* out_count, void* out_records, void* out_slot, hipStream_t stream) {
    if (!image || !palette || !workspace || !out_label || !out_dist || !out_count || !out_records || !out_slot || !shape_ok(h, w, n_colours) ||
        ((uintptr_t)palette & 3) || ((uintptr_t)workspace & 15) || ((uintptr_t)out_label & 1) || ((uintptr_t)out_dist & 1) ||
        ((uintptr_t)out_count & 3) || ((uintptr_t)out_records & 7) || ((uintptr_t)out_slot & 3))
        return (int)hipErrorInvalidValue;
    const int K = n_colours;
    const int64_t npix = (int64_t)h * w;
    u64* sum = (u64*)workspace;
    uint32_t* cnt = (uint32_t*)((char*)workspace + up16(8 * (int64_t)K));
    PA_TRY(hipMemsetAsync(workspace, 0, (size_t)(up16(8 * (int64_t)K) + up16(4 * (int64_t)K)), stream));
    PA_TRY(launch_nearest(image, palette, h, w, K, out_label, out_dist, stream));
    const dim3 grid((unsigned)((npix + STAT_CHUNK - 1) / STAT_CHUNK), (unsigned)((K + STAT_BINS - 1) / STAT_BINS));
    PA_LAUNCH_TRY(minmax_stats_kernel, grid, dim3(TPB), 0, stream, (const uint16_t*)out_label, (const uint16_t*)out_dist, cnt, sum, npix, K);
    PA_LAUNCH(minmax_compact_kernel, dim3(1), dim3(TPB), 0, stream, (const uint32_t*)cnt, (const u64*)sum, (int*)out_count,
              (pa_minmax_record*)out_records, (int*)out_slot, K);
    LAUNCH_CHECK();
}

int pa_minmax_masks(const void* label, const void* slot, int h, int w, int n_colours, int first, int n_cap, void* out_bits, void* out_bytes,
                    hipStream_t stream) {
    if (!label || !slot || !out_bits || !shape_ok(h, w, n_colours) || first < 0 || n_cap < 1 || n_cap > MAX_COL || ((uintptr_t)label & 1) ||
        ((uintptr_t)slot & 3) || ((uintptr_t)out_bits & 3))
        return (int)hipErrorInvalidValue;
    const int64_t npix = (int64_t)h * w;
    const int words = (int)((npix + 31) / 32);
    PA_TRY(hipMemsetAsync(out_bits, 0, 4 * (size_t)n_cap * words, stream));
    if (out_bytes) PA_TRY(hipMemsetAsync(out_bytes, 0, (size_t)n_cap * npix, stream));
    PA_LAUNCH(minmax_masks_kernel, dim3((unsigned)((words + TPB - 1) / TPB)), dim3(TPB), 0, stream, (const uint16_t*)label, (const int*)slot,
              (uint32_t*)out_bits, (uint8_t*)out_bytes, npix, words, n_colours, first, n_cap);
    LAUNCH_CHECK();
}

}  // extern "C"
