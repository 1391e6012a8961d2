// COCO instance mask AP up to the per-detection match flags on the device: what COCOeval.computeIoU and COCOeval.evaluateImg do per
// picture on RLE masks with Python loops (iouType "segm", useCats 0 or 1) -- restated from pycocotools' published source
// (tests/painter_ap_host.py is the definition), unverified against pycocotools.  The detections' bit masks, scores and count are where
// pa_inst_decode left them, their classes where pa_pano_decode left them; one 48-byte record per detection leaves the device.
//
//   intersect : I[d][g] = popc(det[d] & gt[g]) summed over the words of the masks, for a whole job table in ONE launch, grid = (word parts,
//               pair tiles, jobs).  A thread holds its word of 8 detections and 8 ground truths in registers (16 loads, 64 and + popc) and
//               strides over the part's 2048 words; the tiles of the first ground-truth column also count the detections' pixels, those
//               of the first detection row the ground truths'.  The workgroup reduces across lanes (shuffles) and waves (LDS) once at the
//               end and adds its non-zero sums with 32-bit integer atomics.  The padding bits of a last word are masked, whoever packed it.
//   match     : one workgroup per job.  Stable rank of the detections by descending score (O(D^2) counting, ties to the lower index), the
//               IoU doubles -- one IEEE division each -- staged in LDS (D_cap x G_cap x 8 bytes, 128 KB at the caps, of the 160 KB of a
//               CU), per area range the ignore flags as bits in LDS, then ONE THREAD per (mode, range, threshold) runs evaluateImg's
//               sequential greedy loop with the matched, crowd and ignored ground truths as bits in registers.  The walk over the
//               ground truths "ignored ones last, stop at the first ignored one once a non-ignored one is held" is ONE pass in table
//               order with two running bests (non-ignored, ignored; >= keeps the later of equals, as the walk does) and the ignored
//               best counts only when there is no other: no order table, and the row of IoUs is read four at a time, every lane
//               the same address.  That walk, the rank, the threshold cap and the ignore words are coco_match.h's, shared with
//               painter_kpt.hip; the class filter of mode "per_class" goes in as the walk's skip predicate.
//   emit      : per detection in sorted order one pa_ap_record, and the number of records per job.  A job with a flag word emits nothing.
//
// Caps: AP_MAX_D = AP_MAX_G = 128 detections / ground truths per picture (COCO val has at most 93 annotations per picture, the decode keeps
// 100), n_ranges * n_thrs <= 64 (the bits of a record's words), n_classes <= 1024, h * w < 2^31.
// Everything is stream-ordered, allocates nothing and never returns to the host.  Integer atomics only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/painter_hip.h"
#include "common.h"
#include "coco_match.h"

#pragma clang fp contract(off)

namespace {

constexpr int AP_THREADS = 256;
constexpr int AP_TILE = 8;                         // detections x ground truths a thread holds
constexpr int AP_SHARE = 2048;                     // words of a part: eight passes of the workgroup
constexpr int AP_MAX_PARTS = 64;
constexpr int AP_MAX_D = 128, AP_MAX_G = 128, AP_MAX_K = 1024, AP_MAX_BITS = 64;
constexpr int64_t AP_MAX_WORDS = (int64_t)1 << 26;           // h * w < 2^31

enum : uint32_t { FLAG_NAN = 1u, FLAG_DET_CLASS = 2u, FLAG_GT_CLASS = 4u };

inline bool caps_ok(int n_jobs, int d_cap, int g_cap) {
    return n_jobs >= 1 && n_jobs <= 65535 && d_cap >= 1 && d_cap <= AP_MAX_D && g_cap >= 1 && g_cap <= AP_MAX_G;
}

// Workspace: I, the detections' pixel counts and the ground truths' (cleared together), then per job the sorted order and the four
// bit words per rank (matched agnostic, matched per class, ignored agnostic, ignored per class).
struct Layout {
    int64_t inter, darea, gpix, order, bits, end;
};
inline Layout layout(int n_jobs, int d_cap, int g_cap) {
    Layout l;
    l.inter = 0;
    l.darea = up16(4 * (int64_t)n_jobs * d_cap * g_cap);
    l.gpix = up16(l.darea + 4 * (int64_t)n_jobs * d_cap);
    l.order = up16(l.gpix + 4 * (int64_t)n_jobs * g_cap);
    l.bits = up16(l.order + 4 * (int64_t)n_jobs * d_cap);
    l.end = l.bits + 8 * (int64_t)n_jobs * 4 * d_cap;
    return l;
}

// Pixels of a job, 0 for one that counts nothing.
DEVI int64_t job_pixels(const pa_ap_job& job) {
    if (job.h < 1 || job.w < 1) return 0;
    const int64_t npix = (int64_t)job.h * job.w;
    return npix < ((int64_t)1 << 31) ? npix : 0;
}
// The table sizes of a job as every kernel reads them: D from the device, G from the host, both within the call's capacities.
DEVI int job_d(const pa_ap_job& job, int d_cap) {
    if (!job.det_masks || !job.det_scores || !job.det_count || job_pixels(job) == 0) return 0;
    return clampi(*static_cast<const int32_t*>(job.det_count), 0, job.d_cap < d_cap ? job.d_cap : d_cap);
}
DEVI int job_g(const pa_ap_job& job, int g_cap) {
    if (!job.gt_masks || !job.gt_table || job_pixels(job) == 0) return 0;
    return clampi(job.n_gt, 0, g_cap);
}
DEVI uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += (uint32_t)__shfl_xor((int)v, s, 64);
    return v;
}

// grid: x = part of the job's words, y = pair tile (detection tile major), z = job.  inter uint32 [jobs][d_cap][g_cap], darea uint32
// [jobs][d_cap], gpix uint32 [jobs][g_cap], all cleared.
__global__ __launch_bounds__(AP_THREADS) void ap_intersect_kernel(const pa_ap_job* __restrict__ jobs, int d_cap, int g_cap,
                                                                  uint32_t* __restrict__ inter, uint32_t* __restrict__ darea,
                                                                  uint32_t* __restrict__ gpix) {
    __shared__ uint32_t sums[AP_TILE * AP_TILE + 2 * AP_TILE];
    const int tid = threadIdx.x, lane = tid & 63, j = blockIdx.z;
    const pa_ap_job job = jobs[j];
    const int64_t npix = job_pixels(job);
    if (npix == 0) return;                                        // uniform over the workgroup, as every return below
    const int words = (int)((npix + 31) / 32), rest = (int)(npix & 31);
    const int D = job_d(job, d_cap), G = job_g(job, g_cap);
    if (D == 0 && G == 0) return;
    const int tiles_g = (g_cap + AP_TILE - 1) / AP_TILE;
    const int d0 = (int)(blockIdx.y / tiles_g) * AP_TILE, g0 = (int)(blockIdx.y % tiles_g) * AP_TILE;
    if (d0 >= (D > 0 ? D : 1) || g0 >= (G > 0 ? G : 1)) return;
    const int n_parts = (words + AP_SHARE - 1) / AP_SHARE;
    if ((int)blockIdx.x >= n_parts) return;
    if (tid < AP_TILE * AP_TILE + 2 * AP_TILE) sums[tid] = 0u;
    __syncthreads();
    const uint32_t* __restrict__ dm = static_cast<const uint32_t*>(job.det_masks);
    const uint32_t* __restrict__ gm = static_cast<const uint32_t*>(job.gt_masks);
    uint32_t acc[AP_TILE][AP_TILE], da[AP_TILE], ga[AP_TILE];
#pragma unroll
    for (int i = 0; i < AP_TILE; ++i) {
        da[i] = 0u;
        ga[i] = 0u;
#pragma unroll
        for (int k = 0; k < AP_TILE; ++k) acc[i][k] = 0u;
    }
    for (int part = blockIdx.x; part < n_parts; part += gridDim.x) {
        const int end = (part + 1) * AP_SHARE < words ? (part + 1) * AP_SHARE : words;
        for (int w = part * AP_SHARE + tid; w < end; w += AP_THREADS) {
            const uint32_t keep = (w == words - 1 && rest) ? (1u << rest) - 1u : ~0u;          // the bits of the word that are pixels
            uint32_t a[AP_TILE], b[AP_TILE];
#pragma unroll
            for (int i = 0; i < AP_TILE; ++i) {
                a[i] = d0 + i < D ? dm[(int64_t)(d0 + i) * words + w] & keep : 0u;
                b[i] = g0 + i < G ? gm[(int64_t)(g0 + i) * words + w] & keep : 0u;
            }
#pragma unroll
            for (int i = 0; i < AP_TILE; ++i) {
                da[i] += (uint32_t)__popc(a[i]);
                ga[i] += (uint32_t)__popc(b[i]);
#pragma unroll
                for (int k = 0; k < AP_TILE; ++k) acc[i][k] += (uint32_t)__popc(a[i] & b[k]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < AP_TILE; ++i) {
#pragma unroll
        for (int k = 0; k < AP_TILE; ++k) {
            const uint32_t v = wave_sum(acc[i][k]);
            if (lane == 0 && v) atomicAdd(&sums[i * AP_TILE + k], v);
        }
        const uint32_t vd = wave_sum(da[i]), vg = wave_sum(ga[i]);
        if (lane == 0 && vd) atomicAdd(&sums[AP_TILE * AP_TILE + i], vd);
        if (lane == 0 && vg) atomicAdd(&sums[AP_TILE * AP_TILE + AP_TILE + i], vg);
    }
    __syncthreads();
    if (tid < AP_TILE * AP_TILE) {
        const int d = d0 + tid / AP_TILE, g = g0 + tid % AP_TILE;
        if (d < D && g < G && sums[tid]) atomicAdd(&inter[((int64_t)j * d_cap + d) * g_cap + g], sums[tid]);
    } else if (tid < AP_TILE * AP_TILE + AP_TILE) {
        const int d = d0 + tid - AP_TILE * AP_TILE;
        if (g0 == 0 && d < D && sums[tid]) atomicAdd(&darea[(int64_t)j * d_cap + d], sums[tid]);
    } else if (tid < AP_TILE * AP_TILE + 2 * AP_TILE) {
        const int g = g0 + tid - AP_TILE * AP_TILE - AP_TILE;
        if (d0 == 0 && g < G && sums[tid]) atomicAdd(&gpix[(int64_t)j * g_cap + g], sums[tid]);
    }
}

// One workgroup per job; dynamic LDS: double [d_cap][g_cap].  order int32 [jobs][d_cap] (rank -> detection), bits u64 [jobs][4][d_cap].
__global__ __launch_bounds__(AP_THREADS) void ap_match_kernel(const pa_ap_job* __restrict__ jobs, int d_cap, int g_cap, int K, int modes,
                                                              const double* __restrict__ thrs, int T, const double* __restrict__ ranges,
                                                              int A, const uint32_t* __restrict__ inter, const uint32_t* __restrict__ darea,
                                                              const uint32_t* __restrict__ gpix, int32_t* __restrict__ order_out,
                                                              u64* __restrict__ bits_out, uint32_t* __restrict__ flags) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* ious = reinterpret_cast<double*>(smem);
    __shared__ double s_garea[AP_MAX_G];
    __shared__ u64 s_bits[4][AP_MAX_D];
    __shared__ float s_score[AP_MAX_D];
    __shared__ int s_darea[AP_MAX_D], s_dcls[AP_MAX_D], s_order[AP_MAX_D], s_gcls[AP_MAX_G];
    __shared__ uint32_t s_gpix[AP_MAX_G];
    __shared__ uint8_t s_gcrowd[AP_MAX_G];
    __shared__ u64 s_ign[AP_MAX_BITS][2], s_crowd[2];            // per range the ignored ground truths as bits; the crowd ones
    __shared__ uint32_t s_flags;
    const int tid = threadIdx.x, j = blockIdx.x;
    const pa_ap_job job = jobs[j];
    const int D = job_d(job, d_cap), G = job_g(job, g_cap);
    const bool lone = D == 0 && job.empty_as_one != 0;            // the reference's single empty detection
    const int Dn = lone ? 1 : D;
    const float* __restrict__ scores = static_cast<const float*>(job.det_scores);
    const int32_t* __restrict__ classes = static_cast<const int32_t*>(job.det_classes);
    const pa_ap_gt* __restrict__ gt = static_cast<const pa_ap_gt*>(job.gt_table);
    if (tid == 0) s_flags = 0u;
    __syncthreads();
    uint32_t bad = 0u;
    bool crowd = false;
    if (tid < AP_MAX_D) {
        s_bits[0][tid] = s_bits[1][tid] = s_bits[2][tid] = s_bits[3][tid] = 0ull;
        if (tid < Dn) {
            const float s = lone ? 0.f : scores[tid];
            const int c = lone || !classes ? 0 : classes[tid];
            if (s != s) bad |= FLAG_NAN;
            if ((modes & 2) && (c < 0 || c >= K)) bad |= FLAG_DET_CLASS;
            s_score[tid] = s;
            s_dcls[tid] = c;
            s_darea[tid] = lone ? 0 : (int)darea[(int64_t)j * d_cap + tid];
        }
    } else if (tid - AP_MAX_D < G) {
        const int g = tid - AP_MAX_D;
        const pa_ap_gt e = gt[g];
        if (e.category < 0 || e.category >= K) bad |= FLAG_GT_CLASS;
        const uint32_t pix = gpix[(int64_t)j * g_cap + g];
        s_gcls[g] = e.category;
        crowd = e.iscrowd != 0;
        s_gcrowd[g] = crowd;
        s_gpix[g] = pix;
        s_garea[g] = e.area < 0.0 ? (double)pix : e.area;
    }
    if (tid >= AP_MAX_D) {                                        // waves 2 and 3 hold ground truths 0 .. 63 and 64 .. 127
        const u64 b = __ballot(crowd);
        if ((tid & 63) == 0) s_crowd[(tid - AP_MAX_D) >> 6] = b;
    }
    if (bad) atomicOr(&s_flags, bad);
    __syncthreads();
    if (s_flags) {                                                // uniform: a refused picture is not matched
        if (tid == 0) flags[j] = s_flags;
        return;
    }
    // stable rank by descending score, ties to the lower index
    if (tid < Dn) s_order[coco::rank_by_score(s_score, Dn, tid, false)] = tid;
    for (int i = tid; i < Dn * G; i += AP_THREADS) {
        const int d = i / G, g = i % G;
        const uint32_t c = lone ? 0u : inter[((int64_t)j * d_cap + d) * g_cap + g];
        double v = 0.0;
        if (c) {
            const long long uni = s_gcrowd[g] ? (long long)s_darea[d] : (long long)s_darea[d] + (long long)s_gpix[g] - (long long)c;
            v = (double)c / (double)uni;
        }
        ious[d * g_cap + g] = v;
    }
    // per range: the ignored ground truths
    if (tid < A) coco::ignore_words(s_garea, G, ranges[2 * tid], ranges[2 * tid + 1], s_crowd[0], s_crowd[1], s_ign[tid]);
    __syncthreads();
    if (tid < 2 * A * T && ((modes >> (tid / (A * T))) & 1)) {
        const int mode = tid / (A * T), a = tid % (A * T) / T, t = tid % T;
        const double thr0 = coco::cap_threshold(thrs[t]), lo = ranges[2 * a], hi = ranges[2 * a + 1];
        const u64 bit = 1ull << (a * T + t);
        const u64 ign0 = s_ign[a][0], ign1 = s_ign[a][1], crowd0 = s_crowd[0], crowd1 = s_crowd[1];
        u64 taken0 = 0ull, taken1 = 0ull;                         // the ground truths matched at this threshold
        for (int r = 0; r < Dn; ++r) {
            const int d = s_order[r], dc = s_dcls[d];
            const int m = coco::match_one(ious + d * g_cap, G, thr0, ign0, ign1, crowd0, crowd1, taken0, taken1,
                                          [&](int g) { return mode == 1 && s_gcls[g] != dc; });
            bool ign;
            if (m > -1) {
                atomicOr(&s_bits[mode][r], bit);
                ign = coco::bit_of(ign0, ign1, m);
            } else {
                ign = (double)s_darea[d] < lo || (double)s_darea[d] > hi;
            }
            if (ign) atomicOr(&s_bits[2 + mode][r], bit);
        }
    }
    __syncthreads();
    if (tid < Dn) {
        order_out[(int64_t)j * d_cap + tid] = s_order[tid];
#pragma unroll
        for (int s = 0; s < 4; ++s) bits_out[((int64_t)j * 4 + s) * d_cap + tid] = s_bits[s][tid];
    }
    if (tid == 0) flags[j] = 0u;
}

// One workgroup per job, one thread per rank.
__global__ __launch_bounds__(AP_MAX_D) void ap_emit_kernel(const pa_ap_job* __restrict__ jobs, int d_cap, const uint32_t* __restrict__ darea,
                                                           const int32_t* __restrict__ order, const u64* __restrict__ bits,
                                                           const uint32_t* __restrict__ flags, pa_ap_record* __restrict__ records,
                                                           int32_t* __restrict__ record_counts) {
    const int r = threadIdx.x, j = blockIdx.x;
    const pa_ap_job job = jobs[j];
    const int D = job_d(job, d_cap);
    const bool lone = D == 0 && job.empty_as_one != 0;
    const int Dn = flags[j] ? 0 : (lone ? 1 : D);
    if (r == 0) record_counts[j] = Dn;
    if (r >= Dn) return;
    const int d = order[(int64_t)j * d_cap + r];
    const int32_t* __restrict__ classes = static_cast<const int32_t*>(job.det_classes);
    pa_ap_record rec;
    rec.score = lone ? 0.f : static_cast<const float*>(job.det_scores)[d];
    rec.area = lone ? 0 : (int32_t)darea[(int64_t)j * d_cap + d];
    rec.category = lone || !classes ? 0 : classes[d];
    rec.index = d;
    rec.matched[0] = bits[((int64_t)j * 4 + 0) * d_cap + r];
    rec.matched[1] = bits[((int64_t)j * 4 + 1) * d_cap + r];
    rec.ignored[0] = bits[((int64_t)j * 4 + 2) * d_cap + r];
    rec.ignored[1] = bits[((int64_t)j * 4 + 3) * d_cap + r];
    records[(int64_t)j * d_cap + r] = rec;
}

}  // namespace

extern "C" {

int64_t pa_ap_workspace_bytes(int n_jobs, int d_cap, int g_cap) {
    if (!caps_ok(n_jobs, d_cap, g_cap)) return -1;
    return layout(n_jobs, d_cap, g_cap).end;
}

int64_t pa_ap_workspace_offset(int n_jobs, int d_cap, int g_cap, int which) {
    if (!caps_ok(n_jobs, d_cap, g_cap) || which < 0 || which > 4) return -1;
    const Layout l = layout(n_jobs, d_cap, g_cap);
    const int64_t at[5] = {l.inter, l.darea, l.gpix, l.order, l.bits};
    return at[which];
}

int pa_ap_add(const pa_ap_job* jobs, int n_jobs, int64_t max_words, int d_cap, int g_cap, int n_classes, int modes, const double* iou_thrs_f64,
              int n_thrs, const double* area_ranges_f64, int n_ranges, pa_ap_record* records, void* record_counts, void* flags_u32,
              void* workspace, hipStream_t stream) {
    if (!jobs || !iou_thrs_f64 || !area_ranges_f64 || !records || !record_counts || !flags_u32 || !workspace || !caps_ok(n_jobs, d_cap, g_cap) ||
        max_words < 1 || max_words > AP_MAX_WORDS || n_classes < 1 || n_classes > AP_MAX_K || modes < 1 || modes > 3 || n_thrs < 1 ||
        n_ranges < 1 || n_thrs > AP_MAX_BITS || n_ranges > AP_MAX_BITS || n_thrs * n_ranges > AP_MAX_BITS ||
        (((uintptr_t)jobs | (uintptr_t)iou_thrs_f64 | (uintptr_t)area_ranges_f64 | (uintptr_t)records) & 7) != 0 ||
        (((uintptr_t)record_counts | (uintptr_t)flags_u32) & 3) != 0 || ((uintptr_t)workspace & 15) != 0)
        return (int)hipErrorInvalidValue;
    const Layout l = layout(n_jobs, d_cap, g_cap);
    char* ws = static_cast<char*>(workspace);
    uint32_t* inter = reinterpret_cast<uint32_t*>(ws + l.inter);
    uint32_t* darea = reinterpret_cast<uint32_t*>(ws + l.darea);
    uint32_t* gpix = reinterpret_cast<uint32_t*>(ws + l.gpix);
    int32_t* order = reinterpret_cast<int32_t*>(ws + l.order);
    u64* bits = reinterpret_cast<u64*>(ws + l.bits);
    uint32_t* flags = static_cast<uint32_t*>(flags_u32);
    const size_t lds = sizeof(double) * (size_t)d_cap * (size_t)g_cap;
    static bool attr_done = false;
    if (!attr_done) {
        PA_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(ap_match_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)(sizeof(double) * AP_MAX_D * AP_MAX_G)));
        attr_done = true;
    }
    PA_TRY(hipMemsetAsync(inter, 0, (size_t)l.order, stream));
    const int64_t parts = (max_words + AP_SHARE - 1) / AP_SHARE;
    const unsigned tiles = (unsigned)(((d_cap + AP_TILE - 1) / AP_TILE) * ((g_cap + AP_TILE - 1) / AP_TILE));
    const dim3 grid((unsigned)(parts < AP_MAX_PARTS ? parts : AP_MAX_PARTS), tiles, (unsigned)n_jobs);
    PA_LAUNCH_TRY(ap_intersect_kernel, grid, dim3(AP_THREADS), 0, stream, jobs, d_cap, g_cap, inter, darea, gpix);
    PA_LAUNCH_TRY(ap_match_kernel, dim3((unsigned)n_jobs), dim3(AP_THREADS), lds, stream, jobs, d_cap, g_cap, n_classes, modes, iou_thrs_f64,
                  n_thrs, area_ranges_f64, n_ranges, (const uint32_t*)inter, (const uint32_t*)darea, (const uint32_t*)gpix, order, bits, flags);
    PA_LAUNCH(ap_emit_kernel, dim3((unsigned)n_jobs), dim3(AP_MAX_D), 0, stream, jobs, d_cap, (const uint32_t*)darea, (const int32_t*)order,
              (const u64*)bits, (const uint32_t*)flags, records, (int32_t*)record_counts);
    LAUNCH_CHECK();
}

}  // extern "C"
