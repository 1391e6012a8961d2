// Panoptic merge of a painted `coco_pano_semseg` picture with class-agnostic instances on the device: what the evaluators do on the host
// with a float32 [H][W][133] distance tensor copied to numpy and back, a dense einsum("nhw,hwk->nk") over float masks and a Python loop
// with two .item() synchronisations per instance (Painter/eval/coco_panoptic/COCOPanoEvaluatorCustom.py:47-134, 203-276;
// COCOInstSegEvaluatorCustom.py:169-194; COCOPanoSemSegEvaluatorCustom.py:108-136), restated on integers and bit masks:
//
//   vote    : S[i][k] = sum over the pixels p of mask i of d2(p, k), k < n_things, uint64; class_i = first minimum.  The reference's
//             argmax_k sum (1 - d / D) is this argmin because D > 0 is one constant.  A workgroup packs the 2048 pixels of its chunk into
//             LDS; a wave takes an instance, each lane loads one of the chunk's 64 mask words, and the wave walks only the set bits
//             (wave-uniform bit scans): lane = thing class, the pixel is a broadcast LDS read, v_sad_u8 is the whole abs distance.  One
//             integer atomic per (instance, class) and chunk with a non-zero partial -- exact and order-independent.
//   paste   : ONE workgroup walks the instances in stable descending score order (counting rank in LDS).  Thread t owns the words
//             t, t + 1024, ... of the union U, so U needs no barrier; per instance one block reduction of (area, intersection) packed in
//             a uint64, double-buffered so that one barrier per instance is enough.  The two comparisons are the reference's own double
//             arithmetic.  Writes the list of accepted instances (position = id - 1); leaves at the score threshold.
//   hist    : LDS histogram of the semantic labels >= n_things of the pixels outside U, integer atomics to memory.
//   ids     : one wave hands out the stuff ids in label order (ballot prefix) and writes the segment table.
//   paint   : thread = pixel; a pixel inside U belongs to the first accepted instance, in order, whose mask holds its bit; writes the
//             panoptic map, the optional id2rgb picture and the things' final areas (LDS counts, then integer atomics).
//
// Everything is stream-ordered, allocates nothing, never returns to the host; the instance count is read on the device and every launch
// is sized by the capacities.  The padding bits of a mask's last word are masked wherever a mask is read.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "../../include/painter_hip.h"
#include "painter_post.h"

#pragma clang fp contract(off)

namespace {

constexpr int64_t MAX_PIX = 1 << 24;  // h * w: S <= 2^24 * (765 + 195075) < 2^42
constexpr int MAX_COL = 1024;         // n_colours
constexpr int MAX_INST = 1024;        // max_inst = threads of the paste workgroup
constexpr int PIX_CHUNK = 2048;       // pixels per vote / histogram workgroup = 64 mask words, one per lane
constexpr int PASTE_THREADS = 1024;

struct Layout {
    int64_t S, hist, meta, U, zero_end, semmap, list, stuff_id, total;
};

Layout layout(int h, int w, int K, int T, int max_inst) {
    Layout L;
    const int64_t npix = (int64_t)h * w, words = (npix + 31) / 32;
    int64_t o = 0;
    L.S = o;        o = up256(o + 8 * (int64_t)max_inst * T);
    L.hist = o;     o = up256(o + 4 * (int64_t)K);
    L.meta = o;     o = up256(o + 64);
    L.U = o;        o = up256(o + 4 * words);
    L.zero_end = o;                                  // [0, zero_end) is cleared at the start of a merge
    L.semmap = o;   o = up256(o + 4 * npix);
    L.list = o;     o = up256(o + 4 * (int64_t)max_inst);
    L.stuff_id = o; o = up256(o + 4 * (int64_t)K);
    L.total = o;
    return L;
}

bool shape_ok(int h, int w, int K, int T, int max_inst) {
    return h >= 1 && w >= 1 && (int64_t)h * w <= MAX_PIX && K >= 2 && K <= MAX_COL && T >= 2 && T <= K && max_inst >= 1 && max_inst <= MAX_INST;
}

// The bits of word w that are pixels: all of them except in a last word that the picture does not fill.
DEVI uint32_t pixel_bits(int w, int words, int64_t npix) {
    const int rest = (int)(npix & 31);
    return (w == words - 1 && rest) ? (1u << rest) - 1u : ~0u;
}
DEVI int count_of(const int* __restrict__ n_dev, int max_inst) {
    const int n = *n_dev;
    return n < 0 ? 0 : (n > max_inst ? max_inst : n);
}
// d2 of the definition: 0 sum |d|, 1 sum d^2, 2 sum (|d| + d^2) = twice the reference's mean distance.
template <int DIST>
DEVI uint32_t dist2(uint32_t px, uint32_t col) {
    if (DIST == 0) return __builtin_amdgcn_sad_u8(px, col, 0u);
    uint32_t s = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int d = (int)((px >> (8 * c)) & 255u) - (int)((col >> (8 * c)) & 255u);
        const uint32_t a = (uint32_t)(d < 0 ? -d : d);
        s += DIST == 1 ? a * a : a + a * a;
    }
    return s;
}

// grid: x = blocks of 256 words, y = mask row.  Any non-zero byte is a set bit.
__global__ __launch_bounds__(256) void pano_pack_kernel(const uint8_t* __restrict__ src, uint32_t* __restrict__ out, int64_t npix, int words) {
    const int w = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (w >= words) return;
    const int64_t p0 = (int64_t)w * 32;
    const int nb = npix - p0 < 32 ? (int)(npix - p0) : 32;
    const uint8_t* s = src + (int64_t)r * npix + p0;
    uint32_t word = 0;
    for (int b = 0; b < nb; ++b) word |= (s[b] != 0 ? 1u : 0u) << b;
    out[(int64_t)r * words + w] = word;
}

// grid: x = chunks of PIX_CHUNK pixels.  4 waves; wave v takes the instances v, v + 4, ...; lane = mask word of the chunk while loading,
// lane = thing class (in groups of 64) while summing.  A partial stays below 2048 * 195840 < 2^32.
template <int DIST>
__global__ __launch_bounds__(256) void pano_vote_kernel(const uint8_t* __restrict__ pic, const float* __restrict__ pal,
                                                        const uint32_t* __restrict__ masks, const int* __restrict__ n_dev, u64* __restrict__ S,
                                                        int64_t npix, int words, int T, int max_inst) {
    __shared__ uint32_t px[PIX_CHUNK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t base = (int64_t)blockIdx.x * PIX_CHUNK;
    const int valid = (int)(npix - base < PIX_CHUNK ? npix - base : PIX_CHUNK);
    for (int i = tid; i < PIX_CHUNK; i += 256) px[i] = i < valid ? pack_pixel(pic, base + i) : 0u;
    __syncthreads();
    const int n = count_of(n_dev, max_inst);
    const int w = blockIdx.x * (PIX_CHUNK / 32) + lane;
    const uint32_t ok = w < words ? pixel_bits(w, words, npix) : 0u;
    const int groups = (T + 63) / 64;
    for (int i = wave; i < n; i += 4) {
        const uint32_t m = ok ? masks[(int64_t)i * words + w] & ok : 0u;
        const u64 any = __ballot(m != 0u);
        if (!any) continue;                                       // wave-uniform: the instance has no pixel in this chunk
        for (int g = 0; g < groups; ++g) {
            const int k = g * 64 + lane;
            const uint32_t col = k < T ? pack_colour(pal, k) : 0u;
            uint32_t acc = 0;
            u64 rest = any;
            while (rest) {
                const int l = __builtin_ctzll(rest);
                rest &= rest - 1;
                uint32_t bits = (uint32_t)__builtin_amdgcn_readlane((int)m, l);
                const uint32_t* row = &px[l * 32];
                while (bits) {
                    const int b = __builtin_ctz(bits);
                    bits &= bits - 1;
                    acc += dist2<DIST>(row[b], col);
                }
            }
            if (k < T && acc) atomicAdd(&S[(int64_t)i * T + k], (u64)acc);
        }
    }
}

// One thread per instance slot: first minimum of its row of S; empty masks (a row of zeros) and slots past the count get class 0.
__global__ __launch_bounds__(256) void pano_classes_kernel(const u64* __restrict__ S, const int* __restrict__ n_dev, int* __restrict__ classes,
                                                           int T, int max_inst) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= max_inst) return;
    int best = 0;
    if (i < count_of(n_dev, max_inst)) {
        u64 bs = S[(int64_t)i * T];
        for (int k = 1; k < T; ++k) {
            const u64 s = S[(int64_t)i * T + k];
            if (s < bs) {
                bs = s;
                best = k;
            }
        }
    }
    classes[i] = best;
}

// ONE workgroup of 1024 threads.  list[id - 1] = instance that got segment id; meta[0] = accepted instances.
// U (cleared by the caller) ends as the union of the VISITED-and-accepted masks.  A NaN score sorts last, as torch.argsort(-scores) places it.
__global__ __launch_bounds__(PASTE_THREADS) void pano_paste_kernel(const uint32_t* __restrict__ masks, const float* __restrict__ scores,
                                                                   const int* __restrict__ n_dev, uint32_t* __restrict__ U,
                                                                   int* __restrict__ list, int* __restrict__ meta,
                                                                   int words, int64_t npix, int max_inst, double overlap_thr, double score_thr) {
    __shared__ float s_score[MAX_INST];
    __shared__ int s_order[MAX_INST];
    __shared__ u64 s_part[2][PASTE_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = count_of(n_dev, max_inst);
    s_score[tid] = tid < n ? scores[tid] : 0.f;
    __syncthreads();
    if (tid < n) {
        const float si = s_score[tid], ki = si != si ? -INFINITY : si;
        int r = 0;
        for (int j = 0; j < n; ++j) {
            const float sj = s_score[j], kj = sj != sj ? -INFINITY : sj;
            r += (kj > ki || (kj == ki && j < tid)) ? 1 : 0;
        }
        s_order[r] = tid;
    }
    __syncthreads();
    const uint32_t tail = pixel_bits(words - 1, words, npix);
    int id = 0, par = 0;
    for (int r = 0; r < n; ++r) {                                 // every branch below is uniform over the workgroup
        const int i = s_order[r];
        if ((double)s_score[i] < score_thr) break;
        const uint32_t* row = masks + (int64_t)i * words;
        uint32_t a = 0, it = 0;
        for (int w = tid; w < words; w += PASTE_THREADS) {
            uint32_t m = row[w];
            if (w == words - 1) m &= tail;
            if (m) {
                a += __popc(m);
                it += __popc(m & U[w]);
            }
        }
        u64 v = ((u64)a << 32) | (u64)it;                         // both halves stay below 2^25: no carry between them
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) s_part[par][wave] = v;
        __syncthreads();       // the only barrier of an instance: s_part[par] is next written two instances on, behind the next barrier
        u64 tot = 0;
#pragma unroll
        for (int k = 0; k < PASTE_THREADS / 64; ++k) tot += s_part[par][k];
        par ^= 1;
        const uint32_t area = (uint32_t)(tot >> 32), inter = (uint32_t)tot;
        if (area == 0) continue;
        if ((double)inter / (double)area > overlap_thr) continue;
        ++id;
        if (tid == 0) list[id - 1] = i;
        for (int w = tid; w < words; w += PASTE_THREADS) {        // the words this thread alone reads and writes
            uint32_t m = row[w];
            if (w == words - 1) m &= tail;
            if (m) U[w] |= m;
        }
    }
    if (tid == 0) meta[0] = id;
}

// grid: x = chunks of PIX_CHUNK pixels.  hist[l] += pixels of the chunk with semantic label l >= T outside U.
__global__ __launch_bounds__(256) void pano_hist_kernel(const int* __restrict__ semmap, const uint32_t* __restrict__ U,
                                                        uint32_t* __restrict__ hist, int64_t npix, int T, int K) {
    __shared__ uint32_t h[MAX_COL];
    const int tid = threadIdx.x;
    for (int i = tid; i < K; i += 256) h[i] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * PIX_CHUNK;
    for (int i = tid; i < PIX_CHUNK; i += 256) {
        const int64_t p = base + i;
        if (p >= npix) break;
        const int l = semmap[p];
        if (l >= T && l < K && !((U[p >> 5] >> (p & 31)) & 1u)) atomicAdd(&h[l], 1u);
    }
    __syncthreads();
    for (int i = T + tid; i < K; i += 256)
        if (h[i]) atomicAdd(&hist[i], h[i]);
}

// One wave.  Things: segment id of the paste, area 0 for the paint pass to fill.  Stuff: labels in ascending order, kept unless
// (double)count < stuff_thr, ids continue after the things'.
__global__ __launch_bounds__(64) void pano_ids_kernel(const uint32_t* __restrict__ hist, const int* __restrict__ list,
                                                      const int* __restrict__ classes, const float* __restrict__ scores, const int* __restrict__ meta,
                                                      int* __restrict__ stuff_id, pa_pano_segment* __restrict__ seg, int* __restrict__ out_count,
                                                      int T, int K, double stuff_thr) {
    const int lane = threadIdx.x;
    const int n_acc = meta[0];
    for (int id = 1 + lane; id <= n_acc; id += 64) {
        const int i = list[id - 1];
        pa_pano_segment s;
        s.id = id; s.isthing = 1; s.category_id = classes[i]; s.instance_id = i; s.area = 0; s.score = scores[i];
        seg[id - 1] = s;
    }
    for (int l = lane; l < T; l += 64) stuff_id[l] = 0;
    int next = n_acc;
    for (int l0 = T; l0 < K; l0 += 64) {
        const int l = l0 + lane;
        const uint32_t c = l < K ? hist[l] : 0u;
        const bool keep = l < K && !((double)c < stuff_thr);
        const u64 b = __ballot(keep);
        if (l < K) {
            const int id = keep ? next + __popcll(b & ((1ull << lane) - 1ull)) + 1 : 0;
            stuff_id[l] = id;
            if (keep) {
                pa_pano_segment s;
                s.id = id; s.isthing = 0; s.category_id = l; s.instance_id = -1; s.area = (int)c; s.score = 0.f;
                seg[id - 1] = s;
            }
        }
        next += __popcll(b);
    }
    if (lane == 0) *out_count = next;
}

// grid: x = blocks of 256 pixels.
__global__ __launch_bounds__(256) void pano_paint_kernel(const int* __restrict__ semmap, const uint32_t* __restrict__ masks,
                                                         const uint32_t* __restrict__ U, const int* __restrict__ list,
                                                         const int* __restrict__ meta, const int* __restrict__ stuff_id,
                                                         int* __restrict__ panoptic, uint8_t* __restrict__ rgb, pa_pano_segment* __restrict__ seg,
                                                         int64_t npix, int words, int T, int K) {
    __shared__ int s_area[MAX_INST];
    __shared__ int s_list[MAX_INST];
    const int tid = threadIdx.x;
    const int n_acc = meta[0] < MAX_INST ? meta[0] : MAX_INST;
    for (int i = tid; i < n_acc; i += 256) {
        s_area[i] = 0;
        s_list[i] = list[i];
    }
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * 256 + tid;
    if (p < npix) {
        const int w = (int)(p >> 5), b = (int)(p & 31);
        int id = 0;
        if ((U[w] >> b) & 1u) {
            for (int k = 0; k < n_acc; ++k)
                if ((masks[(int64_t)s_list[k] * words + w] >> b) & 1u) {
                    id = k + 1;
                    break;
                }
            if (id) atomicAdd(&s_area[id - 1], 1);
        } else {
            const int l = semmap[p];
            if (l >= T && l < K) id = stuff_id[l];
        }
        panoptic[p] = id;
        if (rgb) {                                                // panopticapi's id2rgb
            rgb[3 * p] = (uint8_t)(id & 255);
            rgb[3 * p + 1] = (uint8_t)((id >> 8) & 255);
            rgb[3 * p + 2] = (uint8_t)(id >> 16);
        }
    }
    __syncthreads();
    for (int i = tid; i < n_acc; i += 256)
        if (s_area[i]) atomicAdd(&seg[i].area, s_area[i]);
}

int launch_vote(const uint8_t* pic, const float* pal, const uint32_t* masks, const int* n_dev, u64* S, int* classes, int h, int w, int T,
                int dist_type, int max_inst, hipStream_t stream) {
    const int64_t npix = (int64_t)h * w;
    const int words = (int)((npix + 31) / 32);
    const dim3 grid((unsigned)((npix + PIX_CHUNK - 1) / PIX_CHUNK));
    PA_TRY(hipMemsetAsync(S, 0, 8 * (size_t)max_inst * T, stream));
    if (dist_type == 0) PA_LAUNCH_TRY(pano_vote_kernel<0>, grid, dim3(256), 0, stream, pic, pal, masks, n_dev, S, npix, words, T, max_inst);
    else if (dist_type == 1) PA_LAUNCH_TRY(pano_vote_kernel<1>, grid, dim3(256), 0, stream, pic, pal, masks, n_dev, S, npix, words, T, max_inst);
    else PA_LAUNCH_TRY(pano_vote_kernel<2>, grid, dim3(256), 0, stream, pic, pal, masks, n_dev, S, npix, words, T, max_inst);
    PA_LAUNCH(pano_classes_kernel, dim3((unsigned)((max_inst + 255) / 256)), dim3(256), 0, stream, S, n_dev, classes, T, max_inst);
    return (int)hipGetLastError();
}

bool thresholds_ok(double a, double b, double c) { return a == a && b == b && c == c; }

// S of the layout is not touched here: [hist, zero_end) is cleared.
int launch_merge(const int* semmap, const uint32_t* masks, const float* scores, const int* classes, const int* n_dev, int h, int w, int K, int T,
                 int max_inst, double overlap_thr, double stuff_thr, double score_thr, char* ws, const Layout& L, int* panoptic, uint8_t* rgb,
                 int* out_count, pa_pano_segment* seg, hipStream_t stream) {
    const int64_t npix = (int64_t)h * w;
    const int words = (int)((npix + 31) / 32);
    uint32_t* hist = (uint32_t*)(ws + L.hist);
    int* meta = (int*)(ws + L.meta);
    uint32_t* U = (uint32_t*)(ws + L.U);
    int* list = (int*)(ws + L.list);
    int* stuff_id = (int*)(ws + L.stuff_id);
    PA_TRY(hipMemsetAsync(ws + L.hist, 0, (size_t)(L.zero_end - L.hist), stream));
    PA_TRY(hipMemsetAsync(seg, 0, sizeof(pa_pano_segment) * (size_t)(max_inst + K - T), stream));
    PA_LAUNCH_TRY(pano_paste_kernel, dim3(1), dim3(PASTE_THREADS), 0, stream, masks, scores, n_dev, U, list, meta, words, npix, max_inst,
                  overlap_thr, score_thr);
    PA_LAUNCH_TRY(pano_hist_kernel, dim3((unsigned)((npix + PIX_CHUNK - 1) / PIX_CHUNK)), dim3(256), 0, stream, semmap, U, hist, npix, T, K);
    PA_LAUNCH_TRY(pano_ids_kernel, dim3(1), dim3(64), 0, stream, hist, list, classes, scores, meta, stuff_id, seg, out_count, T, K, stuff_thr);
    PA_LAUNCH(pano_paint_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, semmap, masks, U, list, meta, stuff_id, panoptic,
              rgb, seg, npix, words, T, K);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int64_t pa_pano_workspace_bytes(int h, int w, int n_colours, int n_things, int max_inst) {
    if (!shape_ok(h, w, n_colours, n_things, max_inst)) return -1;
    return layout(h, w, n_colours, n_things, max_inst).total;
}

int pa_pack_mask_bits(const void* masks_u8, int n_rows, int h, int w, void* out_u32, hipStream_t stream) {
    if (!masks_u8 || !out_u32 || n_rows < 1 || n_rows > MAX_INST || h < 1 || w < 1 || (int64_t)h * w > MAX_PIX) return (int)hipErrorInvalidValue;
    const int64_t npix = (int64_t)h * w;
    const int words = (int)((npix + 31) / 32);
    PA_LAUNCH(pano_pack_kernel, dim3((unsigned)((words + 255) / 256), (unsigned)n_rows), dim3(256), 0, stream, (const uint8_t*)masks_u8,
              (uint32_t*)out_u32, npix, words);
    LAUNCH_CHECK();
}

int pa_pano_vote(const void* image, const float* palette, const void* masks_u32, const void* n_dev, int h, int w, int n_colours, int n_things,
                 int dist_type, int max_inst, void* out_s_u64, void* out_classes, hipStream_t stream) {
    if (!image || !palette || !masks_u32 || !n_dev || !out_s_u64 || !out_classes || !shape_ok(h, w, n_colours, n_things, max_inst) ||
        dist_type < 0 || dist_type > 2)
        return (int)hipErrorInvalidValue;
    return launch_vote((const uint8_t*)image, palette, (const uint32_t*)masks_u32, (const int*)n_dev, (u64*)out_s_u64, (int*)out_classes, h, w,
                       n_things, dist_type, max_inst, stream);
}

int pa_pano_merge(const void* semmap_i32, const void* masks_u32, const float* scores, const void* classes_i32, const void* n_dev, int h, int w,
                  int n_colours, int n_things, int max_inst, double overlap_threshold, double stuff_area_thresh, double instances_score_thresh,
                  void* workspace, void* out_panoptic, void* out_rgb, void* out_count, void* out_segments, hipStream_t stream) {
    if (!semmap_i32 || !masks_u32 || !scores || !classes_i32 || !n_dev || !workspace || !out_panoptic || !out_count || !out_segments ||
        !shape_ok(h, w, n_colours, n_things, max_inst) || !thresholds_ok(overlap_threshold, stuff_area_thresh, instances_score_thresh) ||
        ((uintptr_t)workspace & 255) != 0)
        return (int)hipErrorInvalidValue;
    const Layout L = layout(h, w, n_colours, n_things, max_inst);
    return launch_merge((const int*)semmap_i32, (const uint32_t*)masks_u32, scores, (const int*)classes_i32, (const int*)n_dev, h, w, n_colours,
                        n_things, max_inst, overlap_threshold, stuff_area_thresh, instances_score_thresh, (char*)workspace, L,
                        (int*)out_panoptic, (uint8_t*)out_rgb, (int*)out_count, (pa_pano_segment*)out_segments, stream);
}

int pa_pano_decode(const void* image, const float* palette, const void* masks_u32, const float* scores, const void* n_dev,
                   const void* classes_i32, int h, int w, int n_colours, int n_things, int dist_type, int max_inst, double overlap_threshold,
                   double stuff_area_thresh, double instances_score_thresh, void* workspace, void* out_panoptic, void* out_rgb, void* out_count,
                   void* out_segments, void* out_classes, hipStream_t stream) {
    if (!image || !palette || !masks_u32 || !scores || !n_dev || !workspace || !out_panoptic || !out_count || !out_segments || !out_classes ||
        !shape_ok(h, w, n_colours, n_things, max_inst) || dist_type < 0 || dist_type > 2 ||
        !thresholds_ok(overlap_threshold, stuff_area_thresh, instances_score_thresh) || ((uintptr_t)workspace & 255) != 0)
        return (int)hipErrorInvalidValue;
    const Layout L = layout(h, w, n_colours, n_things, max_inst);
    char* ws = (char*)workspace;
    int* semmap = (int*)(ws + L.semmap);
    PA_TRY(pa_palette_argmin(image, palette, semmap, h, w, n_colours, dist_type, stream));
    if (classes_i32)
        PA_TRY(hipMemcpyAsync(out_classes, classes_i32, 4 * (size_t)max_inst, hipMemcpyDeviceToDevice, stream));
    else
        PA_TRY(launch_vote((const uint8_t*)image, palette, (const uint32_t*)masks_u32, (const int*)n_dev, (u64*)(ws + L.S), (int*)out_classes, h,
                           w, n_things, dist_type, max_inst, stream));
    return launch_merge(semmap, (const uint32_t*)masks_u32, scores, (const int*)out_classes, (const int*)n_dev, h, w, n_colours, n_things,
                        max_inst, overlap_threshold, stuff_area_thresh, instances_score_thresh, ws, L, (int*)out_panoptic, (uint8_t*)out_rgb,
                        (int*)out_count, (pa_pano_segment*)out_segments, stream);
}

}  // extern "C"
