// Panoptic quality of panoptic maps against ground-truth annotations on the device: what panopticapi's pq_compute_single_core does per
// picture with two np.unique passes over the picture and Python dict loops, and what PQStat accumulates over a data set -- restated
// from panopticapi's published source (tests/painter_pq_host.py is the definition), unverified against panopticapi.  The map and its
// segment table are where pa_pano_decode left them; only tp, fp, fn and the IoU sum per category leave the device.
//
//   count  : C[g][p] += 1 over the pixels of a whole job table in ONE launch, grid = (parts, jobs).  A workgroup of 1024 threads builds the
//            job's two id -> index maps in LDS (open addressing, 512 slots each, tables of at most 255 entries) and strides over the
//            job's chunks of 2048 pixels.  Lanes are consecutive pixels and segments are coherent, so a wave folds runs of equal
//            (gt id, predicted id) neighbours with a ballot: the head of a run looks the two ids up and adds the run's length -- two
//            look-ups and one atomic per run.  The workgroup counts into (G_cap + 2) x (P_cap + 1) private 32-bit bins in LDS and adds
//            its non-zero bins to the job's uint32 matrix at the end; where maps and bins exceed 160 KB of LDS the run heads add to the
//            matrix directly (the same kernel, BINS_IN_LDS = false).  Integer atomics only.
//   match  : one workgroup per job.  Column and row sums, one thread per (g, p) for the pair test with its two IEEE divisions, matched
//            bits and the duplicate check, the crowd segment per category, false negatives and false positives through LDS histograms.
//   finish : one thread per category walks the jobs in order and the g slots in order and adds into the accumulators sequentially:
//            two runs, and the host statement, give the same bits.  No floating-point atomics anywhere.
//
// Everything is stream-ordered, allocates nothing and never returns to the host.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/painter_hip.h"
#include "painter_post.h"

#pragma clang fp contract(off)

namespace {

constexpr int PQ_THREADS = 1024;
constexpr int PQ_CHUNK = 2048;                    // pixels of a chunk: two passes of the workgroup
constexpr int PQ_CHUNKS_PER_PART = 4;             // a workgroup zeroes and flushes its bins once: give it several chunks
constexpr int PQ_MAX_PARTS = 256;
constexpr int PQ_SLOTS = 512;                     // of an id -> index map; a table has at most 255 entries, so a probe always ends
constexpr int PQ_MAP_BYTES = 2 * 2 * 4 * PQ_SLOTS;          // keys and values of both maps
constexpr int PQ_LDS_BYTES = 160 * 1024;
constexpr int PQ_MAX_G = 254, PQ_MAX_P = 255, PQ_MAX_K = 1024;
constexpr int64_t PQ_MAX_PIXELS = (int64_t)1 << 31;          // of a job: no 32-bit count wraps

enum : uint32_t { FLAG_UNLISTED = 1u, FLAG_EMPTY = 2u, FLAG_CATEGORY = 4u, FLAG_UNION = 8u, FLAG_TWICE = 16u, FLAG_ORDER = 32u };

inline int64_t n_bins(int g_cap, int p_cap) { return (int64_t)(g_cap + 2) * (p_cap + 1); }
inline bool caps_ok(int g_cap, int p_cap) { return g_cap >= 1 && g_cap <= PQ_MAX_G && p_cap >= 1 && p_cap <= PQ_MAX_P; }

// Workspace: the count matrices, then per job and g slot the match (IoU, category or -1), then per job fn and fp per category.
struct Layout {
    int64_t counts, iou, cat, fnfp, end;
};
inline Layout layout(int n_jobs, int g_cap, int p_cap, int K) {
    Layout l;
    l.counts = 0;
    l.iou = up16(4 * (int64_t)n_jobs * n_bins(g_cap, p_cap));
    l.cat = l.iou + 8 * (int64_t)n_jobs * g_cap;
    l.fnfp = up16(l.cat + 4 * (int64_t)n_jobs * g_cap);
    l.end = l.fnfp + 4 * (int64_t)n_jobs * 2 * K;
    return l;
}

DEVI int slot_of(int id) { return (int)(((uint32_t)id * 2654435761u) >> 23); }          // 9 bits

// Entry `index` (1-based) of a table under its id.  Ids <= 0 are never listed (0 is the empty slot); of a repeated id one entry stays.
DEVI void map_insert(int* keys, int* vals, int id, int index) {
    if (id <= 0) return;
    int s = slot_of(id);
    for (int probe = 0; probe < PQ_SLOTS; ++probe) {
        const int old = atomicCAS(&keys[s], 0, id);
        if (old == 0) { vals[s] = index; return; }
        if (old == id) return;
        s = (s + 1) & (PQ_SLOTS - 1);
    }
}

// -> index of `id`, 0 when it is not listed.
DEVI int map_find(const int* keys, const int* vals, int id) {
    int s = slot_of(id);
    for (int probe = 0; probe < PQ_SLOTS; ++probe) {
        const int k = keys[s];
        if (k == id) return vals[s];
        if (k == 0) return 0;
        s = (s + 1) & (PQ_SLOTS - 1);
    }
    return 0;
}

// The table sizes of a job as every kernel reads them: G from the host, P from the device, both within the call's capacities.
DEVI int job_g(const pa_pq_job& job, int g_cap) { return clampi(job.n_gt, 0, job.g_cap < g_cap ? job.g_cap : g_cap); }
DEVI int job_p(const pa_pq_job& job, int p_cap) {
    return clampi(*static_cast<const int32_t*>(job.pred_count), 0, job.p_cap < p_cap ? job.p_cap : p_cap);
}

// grid: x = part of the job, y = job.  counts: uint32 [jobs][(g_cap + 2) * (p_cap + 1)], cleared.
template <bool BINS_IN_LDS>
__global__ __launch_bounds__(PQ_THREADS) void pq_count_kernel(const pa_pq_job* __restrict__ jobs, int g_cap, int p_cap,
                                                              uint32_t* __restrict__ counts, uint32_t* __restrict__ flags) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* gkeys = reinterpret_cast<int*>(smem);
    int* gvals = gkeys + PQ_SLOTS;
    int* pkeys = gvals + PQ_SLOTS;
    int* pvals = pkeys + PQ_SLOTS;
    uint32_t* bins = reinterpret_cast<uint32_t*>(smem + PQ_MAP_BYTES);
    const int tid = threadIdx.x, lane = tid & 63, j = blockIdx.y;
    const pa_pq_job job = jobs[j];
    const int h = job.h, w = job.w;
    if (h < 1 || w < 1) return;                                   // uniform over the workgroup
    const int64_t npix = (int64_t)h * w;
    if (npix > PQ_MAX_PIXELS) return;
    const int64_t n_chunks = (npix + PQ_CHUNK - 1) / PQ_CHUNK;
    if ((int64_t)blockIdx.x >= n_chunks) return;
    const int G = job_g(job, g_cap), P = job_p(job, p_cap), ld = p_cap + 1, total_bins = (g_cap + 2) * ld;
    for (int i = tid; i < 4 * PQ_SLOTS; i += PQ_THREADS) gkeys[i] = 0;
    if (BINS_IN_LDS)
        for (int i = tid; i < total_bins; i += PQ_THREADS) bins[i] = 0u;
    __syncthreads();
    const pa_pq_gt_segment* __restrict__ gseg = static_cast<const pa_pq_gt_segment*>(job.gt_segments);
    const pa_pano_segment* __restrict__ pseg = static_cast<const pa_pano_segment*>(job.pred_segments);
    if (tid < G) map_insert(gkeys, gvals, gseg[tid].id, tid + 1);
    if (tid >= 512 && tid - 512 < P) map_insert(pkeys, pvals, pseg[tid - 512].id, tid - 512 + 1);
    __syncthreads();
    const int32_t* __restrict__ pred = static_cast<const int32_t*>(job.pred);
    const int32_t* __restrict__ gt32 = static_cast<const int32_t*>(job.gt);
    const uint8_t* __restrict__ gt8 = static_cast<const uint8_t*>(job.gt);
    uint32_t* __restrict__ mine = counts + (int64_t)j * total_bins;
    bool unlisted = false;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
#pragma unroll
        for (int half = 0; half < PQ_CHUNK / PQ_THREADS; ++half) {
            const int64_t at = c * PQ_CHUNK + half * PQ_THREADS + tid;
            const bool live = at < npix;
            int gid = 0, pid = 0;
            if (live) {
                pid = pred[at];
                gid = job.gt_rgb ? (int)gt8[3 * at] + 256 * (int)gt8[3 * at + 1] + 65536 * (int)gt8[3 * at + 2] : gt32[at];
            }
            // runs of equal (gid, pid, live) among the wave's lanes: the head of a run looks up and adds its length
            const int gbefore = __shfl_up(gid, 1, 64), pbefore = __shfl_up(pid, 1, 64);
            const int lbefore = __shfl_up((int)live, 1, 64);
            const bool head = lane == 0 || gbefore != gid || pbefore != pid || lbefore != (int)live;
            const u64 heads = __ballot(head);
            if (head && live) {
                const u64 later = lane == 63 ? 0ull : heads >> (lane + 1);
                const uint32_t len = later ? (uint32_t)__builtin_ctzll(later) + 1u : (uint32_t)(64 - lane);
                int g = 0, p = 0;
                if (gid != 0) {
                    g = map_find(gkeys, gvals, gid);
                    g = g ? g : G + 1;                            // a non-zero id that is not in the table
                }
                if (pid != 0) p = map_find(pkeys, pvals, pid);
                if (pid != 0 && p == 0) unlisted = true;          // refused, not counted
                else if (BINS_IN_LDS) atomicAdd(&bins[g * ld + p], len);
                else atomicAdd(&mine[g * ld + p], len);
            }
        }
    }
    if (__ballot(unlisted) != 0ull && lane == 0) atomicOr(&flags[j], FLAG_UNLISTED);
    if (BINS_IN_LDS) {
        __syncthreads();
        for (int i = tid; i < total_bins; i += PQ_THREADS) {
            const uint32_t v = bins[i];
            if (v) atomicAdd(&mine[i], v);
        }
    }
}

// One workgroup per job.  out_iou double [jobs][g_cap], out_cat int32 [jobs][g_cap] (the category of a matched g, else -1), out_fnfp
// uint32 [jobs][2][K].
__global__ __launch_bounds__(PQ_THREADS) void pq_match_kernel(const pa_pq_job* __restrict__ jobs, int g_cap, int p_cap, int K,
                                                              const uint32_t* __restrict__ counts, double* __restrict__ out_iou,
                                                              int32_t* __restrict__ out_cat, uint32_t* __restrict__ out_fnfp,
                                                              uint32_t* __restrict__ flags) {
    __shared__ uint32_t parea[256];                       // column sums, p = 0 .. P
    __shared__ long long garea[256];                      // g = 1 .. G: the annotation's area, or the row sum
    __shared__ int gcat[256], gcrowd[256], pcat[256];
    __shared__ int gmatch[256], pmatch[256];              // how often a row / a column was matched
    __shared__ double giou[256];
    __shared__ int crowd[PQ_MAX_K];                       // per category its crowd segment g, or 0
    __shared__ uint32_t fn_hist[PQ_MAX_K], fp_hist[PQ_MAX_K];
    __shared__ uint32_t s_flags;
    const int tid = threadIdx.x, j = blockIdx.x;
    const pa_pq_job job = jobs[j];
    const int G = job_g(job, g_cap), P = job_p(job, p_cap), ld = p_cap + 1;
    const uint32_t* __restrict__ C = counts + (int64_t)j * (g_cap + 2) * ld;
    const pa_pq_gt_segment* __restrict__ gseg = static_cast<const pa_pq_gt_segment*>(job.gt_segments);
    const pa_pano_segment* __restrict__ pseg = static_cast<const pa_pano_segment*>(job.pred_segments);
    if (tid == 0) s_flags = 0u;
    for (int i = tid; i < K; i += PQ_THREADS) { crowd[i] = 0; fn_hist[i] = 0u; fp_hist[i] = 0u; }
    if (tid < 256) { gmatch[tid] = 0; pmatch[tid] = 0; giou[tid] = 0.0; }
    __syncthreads();
    // the tables: ids ascending from above 0, categories within [0, K)
    uint32_t bits = 0u;
    if (tid >= 1 && tid <= G) {
        const int g = tid, id = gseg[g - 1].id, cat = gseg[g - 1].category;
        if (id <= (g > 1 ? gseg[g - 2].id : 0)) bits |= FLAG_ORDER;
        if (cat < 0 || cat >= K) bits |= FLAG_CATEGORY;
        gcat[g] = cat;
        gcrowd[g] = gseg[g - 1].iscrowd != 0;
        long long area = gseg[g - 1].area;
        if (area < 0) {                                   // count it from the map
            area = 0;
            for (int p = 0; p <= P; ++p) area += C[g * ld + p];
        }
        garea[g] = area;
    }
    if (tid >= 256 && tid - 256 <= P) {
        const int p = tid - 256;
        uint32_t sum = 0u;
        for (int g = 0; g <= G + 1; ++g) sum += C[g * ld + p];
        parea[p] = sum;
        if (p >= 1) {
            const int id = pseg[p - 1].id, cat = pseg[p - 1].category_id;
            if (id <= (p > 1 ? pseg[p - 2].id : 0)) bits |= FLAG_ORDER;
            if (cat < 0 || cat >= K) bits |= FLAG_CATEGORY;
            if (sum == 0u) bits |= FLAG_EMPTY;
            pcat[p] = cat;
        }
    }
    if (bits) atomicOr(&s_flags, bits);
    __syncthreads();
    const bool tables_ok = (s_flags & (FLAG_ORDER | FLAG_CATEGORY)) == 0u;          // uniform; nothing is matched otherwise
    if (tables_ok) {
        for (int i = tid; i < G * P; i += PQ_THREADS) {
            const int g = i / P + 1, p = i % P + 1;
            const uint32_t c = C[g * ld + p];
            if (c == 0u || gcrowd[g] || gcat[g] != pcat[p]) continue;
            const long long uni = (long long)parea[p] + garea[g] - (long long)c - (long long)C[p];
            if (uni <= 0) { atomicOr(&s_flags, FLAG_UNION); continue; }
            const double iou = (double)c / (double)uni;
            if (iou > 0.5) {
                const int gn = atomicAdd(&gmatch[g], 1), pn = atomicAdd(&pmatch[p], 1);
                if (gn > 0 || pn > 0) atomicOr(&s_flags, FLAG_TWICE);
                giou[g] = iou;
            }
        }
        // the crowd segment of a category: the one listed last (the largest rank; of equal ranks the later entry)
        if (tid == 0) {
            for (int g = 1; g <= G; ++g) {
                if (!gcrowd[g]) continue;
                const int have = crowd[gcat[g]];
                if (have == 0 || gseg[g - 1].rank >= gseg[have - 1].rank) crowd[gcat[g]] = g;
            }
        }
    }
    __syncthreads();
    if (tables_ok) {
        if (tid >= 1 && tid <= G && !gcrowd[tid] && gmatch[tid] == 0) atomicAdd(&fn_hist[gcat[tid]], 1u);
        if (tid >= 256 && tid - 256 >= 1 && tid - 256 <= P && pmatch[tid - 256] == 0) {
            const int p = tid - 256, gc = crowd[pcat[p]];
            const long long inter = (long long)C[p] + (gc ? (long long)C[gc * ld + p] : 0ll);
            if (!((double)inter / (double)parea[p] > 0.5)) atomicAdd(&fp_hist[pcat[p]], 1u);
        }
    }
    __syncthreads();
    if (tid < g_cap) {
        const int g = tid + 1;
        const bool matched = tables_ok && g <= G && gmatch[g] > 0;
        out_cat[(int64_t)j * g_cap + tid] = matched ? gcat[g] : -1;
        out_iou[(int64_t)j * g_cap + tid] = matched ? giou[g] : 0.0;
    }
    for (int i = tid; i < K; i += PQ_THREADS) {
        out_fnfp[((int64_t)j * 2 + 0) * K + i] = fn_hist[i];
        out_fnfp[((int64_t)j * 2 + 1) * K + i] = fp_hist[i];
    }
    if (tid == 0 && s_flags) atomicOr(&flags[j], s_flags);
}

// One thread per category: jobs in order, g slots in order.
__global__ __launch_bounds__(256) void pq_finish_kernel(int n_jobs, int g_cap, int K, const double* __restrict__ iou,
                                                        const int32_t* __restrict__ cat, const uint32_t* __restrict__ fnfp,
                                                        const uint32_t* __restrict__ flags, long long* __restrict__ acc_tp,
                                                        long long* __restrict__ acc_fp, long long* __restrict__ acc_fn,
                                                        double* __restrict__ acc_iou) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= K) return;
    long long tp = acc_tp[c], fp = acc_fp[c], fn = acc_fn[c];
    double sum = acc_iou[c];
    for (int j = 0; j < n_jobs; ++j) {
        if (flags[j]) continue;                           // a refused picture adds nothing
        for (int g = 0; g < g_cap; ++g)
            if (cat[(int64_t)j * g_cap + g] == c) {
                tp += 1;
                sum += iou[(int64_t)j * g_cap + g];
            }
        fn += fnfp[((int64_t)j * 2 + 0) * K + c];
        fp += fnfp[((int64_t)j * 2 + 1) * K + c];
    }
    acc_tp[c] = tp; acc_fp[c] = fp; acc_fn[c] = fn;
    acc_iou[c] = sum;
}

}  // namespace

extern "C" {

int pa_pq_lds_bins(int g_cap, int p_cap) { return caps_ok(g_cap, p_cap) && PQ_MAP_BYTES + 4 * n_bins(g_cap, p_cap) <= PQ_LDS_BYTES ? 1 : 0; }

int64_t pa_pq_workspace_bytes(int n_jobs, int g_cap, int p_cap, int n_classes) {
    if (n_jobs < 1 || n_jobs > 65535 || !caps_ok(g_cap, p_cap) || n_classes < 1 || n_classes > PQ_MAX_K) return -1;
    return layout(n_jobs, g_cap, p_cap, n_classes).end;
}

int pa_pq_add(const pa_pq_job* jobs, int n_jobs, int64_t max_pixels, int g_cap, int p_cap, int n_classes, int bins, void* acc_tp_i64,
              void* acc_fp_i64, void* acc_fn_i64, void* acc_iou_f64, void* flags_u32, void* workspace, hipStream_t stream) {
    if (!jobs || !acc_tp_i64 || !acc_fp_i64 || !acc_fn_i64 || !acc_iou_f64 || !flags_u32 || !workspace || n_jobs < 1 || n_jobs > 65535 ||
        max_pixels < 1 || max_pixels > PQ_MAX_PIXELS || !caps_ok(g_cap, p_cap) || n_classes < 1 || n_classes > PQ_MAX_K || bins < 0 ||
        bins > 1 || (((uintptr_t)acc_tp_i64 | (uintptr_t)acc_fp_i64 | (uintptr_t)acc_fn_i64 | (uintptr_t)acc_iou_f64) & 7) != 0 ||
        ((uintptr_t)flags_u32 & 3) != 0 || ((uintptr_t)workspace & 15) != 0)
        return (int)hipErrorInvalidValue;
    const Layout l = layout(n_jobs, g_cap, p_cap, n_classes);
    char* ws = static_cast<char*>(workspace);
    uint32_t* counts = reinterpret_cast<uint32_t*>(ws + l.counts);
    double* iou = reinterpret_cast<double*>(ws + l.iou);
    int32_t* cat = reinterpret_cast<int32_t*>(ws + l.cat);
    uint32_t* fnfp = reinterpret_cast<uint32_t*>(ws + l.fnfp);
    uint32_t* flags = static_cast<uint32_t*>(flags_u32);
    const bool lds_bins = bins == 0 && pa_pq_lds_bins(g_cap, p_cap);
    const size_t lds = (size_t)PQ_MAP_BYTES + (lds_bins ? (size_t)(4 * n_bins(g_cap, p_cap)) : 0);
    if (lds_bins) {
        static bool attr_done = false;
        if (!attr_done) {
            PA_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(pq_count_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       PQ_LDS_BYTES));
            attr_done = true;
        }
    }
    PA_TRY(hipMemsetAsync(counts, 0, (size_t)(4 * (int64_t)n_jobs * n_bins(g_cap, p_cap)), stream));
    PA_TRY(hipMemsetAsync(flags, 0, 4 * (size_t)n_jobs, stream));
    const int64_t chunks = (max_pixels + PQ_CHUNK - 1) / PQ_CHUNK, want = (chunks + PQ_CHUNKS_PER_PART - 1) / PQ_CHUNKS_PER_PART;
    const dim3 grid((unsigned)(want < PQ_MAX_PARTS ? want : PQ_MAX_PARTS), (unsigned)n_jobs);
    if (lds_bins) PA_LAUNCH_TRY((pq_count_kernel<true>), grid, dim3(PQ_THREADS), lds, stream, jobs, g_cap, p_cap, counts, flags);
    else PA_LAUNCH_TRY((pq_count_kernel<false>), grid, dim3(PQ_THREADS), lds, stream, jobs, g_cap, p_cap, counts, flags);
    PA_LAUNCH_TRY(pq_match_kernel, dim3((unsigned)n_jobs), dim3(PQ_THREADS), 0, stream, jobs, g_cap, p_cap, n_classes,
                  (const uint32_t*)counts, iou, cat, fnfp, flags);
    PA_LAUNCH(pq_finish_kernel, dim3((unsigned)((n_classes + 255) / 256)), dim3(256), 0, stream, n_jobs, g_cap, n_classes, (const double*)iou,
              (const int32_t*)cat, (const uint32_t*)fnfp, (const uint32_t*)flags, (long long*)acc_tp_i64, (long long*)acc_fp_i64,
              (long long*)acc_fn_i64, (double*)acc_iou_f64);
    LAUNCH_CHECK();
}

}  // extern "C"
