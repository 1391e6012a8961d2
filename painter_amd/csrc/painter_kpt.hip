// COCO keypoint AP up to the per-detection match flags on the device: what TopDownCocoDatasetCustom.evaluate
// (mmpose_custom/data/topdown_coco_dataset.py:194-315) does after the decode -- photo coordinates, rescoring, OKS NMS over a photo's person
// boxes -- and what COCOeval(..., "keypoints", sigmas) does per photo (computeOks, evaluateImg).  mmpose's oks_iou / oks_nms and
// xtcocotools' COCOeval are restated from their published source (tests/painter_kpt_host.py is the definition), unverified against mmpose /
// xtcocotools.  preds and maxvals are read where pa_pose_keypoints left them; one 32-byte record per evaluated detection leaves the device.
//
//   poses    : one WAVE per box, lane k = keypoint k: the float2 of preds and the maxval are read coalesced, the photo coordinates are
//              painter_engine.to_image's float64 expression rounded to float32, the rescoring's float32 running sum walks the lanes in
//              joint order (shuffles, every lane the same sum).
//   evaluate : one workgroup per photo, one thread per box.
//              rank    stable rank by score (O(D^2) counting on the scores in LDS): descending, equal scores to the HIGHER row as
//                      argsort(kind="stable")[::-1] leaves them; without NMS to the lower row, as COCOeval's stable sort by -score does.
//              nms     thread t holds the pose of the box of rank t in registers.  Per surviving pivot: every wave's first live lane
//                      behind the pivot has put its pose into the wave's slot in LDS; ONE barrier; the first slot that is filled is the
//                      next pivot, every live thread behind it computes its OKS against the slot (every lane the same address: a
//                      broadcast) and drops out above the threshold.  Slots are double-buffered, so the next round's writes need no
//                      second barrier.  No D x D matrix exists anywhere.
//              oks     the OKS doubles of the first max_det survivors against the ground truths, staged in LDS (max_det x g_cap x 8
//                      bytes, 64 KB at the caps, of the 160 KB of a CU) and copied to the workspace for the tests.
//              match   ONE THREAD per (range, threshold) runs evaluateImg's sequential greedy loop with the matched, crowd and ignored
//                      ground truths as bits in registers: one pass in table order with two running bests (non-ignored, ignored; >=
//                      keeps the later of equals, as the walk does) and the ignored best counts only when there is no other -- the walk
//                      painter_ap.hip's ap_match_kernel runs, coco_match.h's match_one, with no class filter.  The
//                      rank, the threshold cap and the per-range ignore words come from that header too.
//              emit    one pa_kpt_record per evaluated survivor.  A photo with a flag word emits nothing.
//
// exp is HIP's double exp; everything that feeds it is stated operation by operation, no fused multiply-add.
// Everything is stream-ordered, allocates nothing and never returns to the host.  LDS atomics on integers only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/painter_hip.h"
#include "common.h"
#include "coco_match.h"

#pragma clang fp contract(off)

namespace {

constexpr int KP_MAX_D = 1024, KP_MAX_G = 128, KP_MAX_K = 32, KP_MAX_BITS = 64, KP_MAX_E = 64;
constexpr int KP_MAX_WAVES = KP_MAX_D / 64;
constexpr int KP_MAX_BOXES = 1 << 24;
constexpr double KP_EPS = 2.220446049250313e-16;              // np.spacing(1) = 2^-52
constexpr int KP_NONE = 0x7fffffff;

enum : uint32_t { FLAG_NAN = 1u, FLAG_GT_AREA = 2u, FLAG_ROW = 4u };

inline bool caps_ok(int n_jobs, int d_cap, int g_cap, int max_det) {
    return n_jobs >= 1 && n_jobs <= 65535 && d_cap >= 1 && d_cap <= KP_MAX_D && g_cap >= 1 && g_cap <= KP_MAX_G && max_det >= 1 &&
           max_det <= KP_MAX_E;
}

// Workspace: per job the NMS order (rank -> position in the job's rows), the survivor flags by rank, the evaluation OKS doubles.
struct Layout {
    int64_t order, alive, oks, end;
};
inline Layout layout(int n_jobs, int d_cap, int g_cap, int max_det) {
    Layout l;
    l.order = 0;
    l.alive = up16(4 * (int64_t)n_jobs * d_cap);
    l.oks = up16(l.alive + 4 * (int64_t)n_jobs * d_cap);
    l.end = l.oks + 8 * (int64_t)n_jobs * max_det * g_cap;
    return l;
}

// One wave per box; boxes float32 [n][5] = center x, y, scale x, y, box score.
__global__ __launch_bounds__(256) void kpt_poses_kernel(const float* __restrict__ preds, const float* __restrict__ maxvals,
                                                        const float* __restrict__ boxes, int n, int K, double heat_w, double heat_h,
                                                        float vis_thr, float* __restrict__ poses, float* __restrict__ scores,
                                                        float* __restrict__ areas) {
    const int lane = threadIdx.x & 63;
    const int64_t box = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (box >= n) return;                                         // uniform over the wave
    const float cx = boxes[box * 5 + 0], cy = boxes[box * 5 + 1], sx = boxes[box * 5 + 2], sy = boxes[box * 5 + 3];
    float m = 0.f;
    if (lane < K) {
        const float2 p = reinterpret_cast<const float2*>(preds)[box * K + lane];
        m = maxvals[box * K + lane];
        const double fx = (double)sx * 200.0, fy = (double)sy * 200.0;
        const double x = (((double)p.x * (fx / heat_w)) + (double)cx) - fx * 0.5;
        const double y = (((double)p.y * (fy / heat_h)) + (double)cy) - fy * 0.5;
        float* out = poses + (box * K + lane) * 3;
        out[0] = (float)x;
        out[1] = (float)y;
        out[2] = m;
    }
    float total = 0.f;
    int count = 0;
    for (int k = 0; k < K; ++k) {                                 // joint order; every lane adds the same values
        const float v = __shfl(m, k, 64);
        if (v > vis_thr) {
            total = total + v;
            ++count;
        }
    }
    if (lane == 0) {
        if (count) total = total / (float)count;
        scores[box] = total * boxes[box * 5 + 4];
        areas[box] = (sx * 200.f) * (sy * 200.f);
    }
}

// One workgroup per photo, blockDim.x = d_cap rounded up to whole waves, at least two; dynamic LDS: double [max_det][g_cap].
__global__ __launch_bounds__(KP_MAX_D) void kpt_evaluate_kernel(const pa_kpt_job* __restrict__ jobs, const float* __restrict__ poses,
                                                                const float* __restrict__ scores, const float* __restrict__ areas,
                                                                int n_rows, int d_cap, int g_cap, int K, const double* __restrict__ sigmas,
                                                                float oks_thr, int max_det, const double* __restrict__ thrs, int T,
                                                                const double* __restrict__ ranges, int A, pa_kpt_record* __restrict__ records,
                                                                int32_t* __restrict__ record_counts, int32_t* __restrict__ survivor_counts,
                                                                uint32_t* __restrict__ flags, int32_t* __restrict__ order_out,
                                                                int32_t* __restrict__ alive_out, double* __restrict__ oks_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* s_oks = reinterpret_cast<double*>(smem);
    __shared__ double s_var[KP_MAX_K], s_garea[KP_MAX_G], s_darea[KP_MAX_E];
    __shared__ u64 s_matched[KP_MAX_E], s_ignored[KP_MAX_E], s_ign[KP_MAX_BITS][2], s_crowd[2], s_skip[2];
    __shared__ float s_score[KP_MAX_D];
    __shared__ float s_slot[2][KP_MAX_WAVES][2 * KP_MAX_K + 1];   // x[K], y[K], the box area
    __shared__ int s_order[KP_MAX_D], s_cand[2][KP_MAX_WAVES], s_keep[KP_MAX_E];
    __shared__ uint32_t s_flags;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_waves = (int)blockDim.x >> 6, j = blockIdx.x;
    const pa_kpt_job job = jobs[j];
    const int32_t* __restrict__ rows = static_cast<const int32_t*>(job.rows);
    const double* __restrict__ gkp = static_cast<const double*>(job.gt_keypoints);
    const pa_kpt_gt* __restrict__ gt = static_cast<const pa_kpt_gt*>(job.gt_table);
    const int D = rows ? clampi(job.n_box, 0, d_cap) : 0;
    const int G = gkp && gt ? clampi(job.n_gt, 0, g_cap) : 0;
    const bool nms = oks_thr >= 0.f;
    if (tid == 0) s_flags = 0u;
    if (tid < KP_MAX_E) s_matched[tid] = s_ignored[tid] = 0ull;
    if (tid < K) {
        const double s2 = sigmas[tid] * 2.0;
        s_var[tid] = s2 * s2;
    }
    __syncthreads();
    // the job's tables: scores and box areas of its rows, the ground truths' flags
    uint32_t bad = 0u;
    int row = 0;
    float area = 0.f;
    if (tid < D) {
        row = rows[tid];
        if (row < 0 || row >= n_rows) {
            bad |= FLAG_ROW;
            row = 0;
        } else {
            const float s = scores[row];
            area = areas[row];
            if (s != s || area != area) bad |= FLAG_NAN;
            s_score[tid] = s;
        }
    }
    if (tid < KP_MAX_G) {                                         // waves 0 and 1 hold ground truths 0 .. 63 and 64 .. 127
        bool crowd = false, skip = false;
        if (tid < G) {
            const pa_kpt_gt e = gt[tid];
            const double a = e.area + KP_EPS;
            if (!(a > 0.0 && a < INFINITY)) bad |= FLAG_GT_AREA;
            s_garea[tid] = e.area;
            crowd = e.iscrowd != 0;
            skip = crowd || e.num_keypoints == 0;
        }
        const u64 bc = __ballot(crowd), bs = __ballot(skip);
        if (lane == 0) {
            s_crowd[wave] = bc;
            s_skip[wave] = bs;
        }
    }
    if (bad) atomicOr(&s_flags, bad);
    __syncthreads();
    if (s_flags) {                                                // uniform: a refused photo is neither ranked nor matched
        if (tid == 0) {
            flags[j] = s_flags;
            record_counts[j] = 0;
            survivor_counts[j] = 0;
        }
        return;
    }
    if (tid < D) s_order[coco::rank_by_score(s_score, D, tid, nms)] = tid;
    __syncthreads();
    // thread t takes the box of rank t
    float px[KP_MAX_K], py[KP_MAX_K];
    bool alive = tid < D;
    bad = 0u;
    if (alive) {
        row = rows[s_order[tid]];                                 // in range: checked above
        area = areas[row];
        const float* __restrict__ p = poses + (int64_t)row * K * 3;
#pragma unroll
        for (int k = 0; k < KP_MAX_K; ++k) {
            px[k] = py[k] = 0.f;
            if (k < K) {
                px[k] = p[3 * k];
                py[k] = p[3 * k + 1];
                const float v = p[3 * k + 2];
                if (px[k] != px[k] || py[k] != py[k] || v != v) bad |= FLAG_NAN;
            }
        }
    }
    if (bad) atomicOr(&s_flags, bad);
    __syncthreads();
    if (s_flags) {
        if (tid == 0) {
            flags[j] = s_flags;
            record_counts[j] = 0;
            survivor_counts[j] = 0;
        }
        return;
    }
    int n_surv = 0;
    if (nms) {
        int cur = -1, b = 0;
        for (int round = 0; round <= D; ++round) {               // at most D pivots and the round that finds none
            const u64 live = __ballot(alive && tid > cur);
            const int first = live ? __ffsll((long long)live) - 1 : -1;
            if (lane == 0) s_cand[b][wave] = live ? wave * 64 + first : KP_NONE;
            if (lane == first) {
                float* slot = s_slot[b][wave];
#pragma unroll
                for (int k = 0; k < KP_MAX_K; ++k)
                    if (k < K) {
                        slot[k] = px[k];
                        slot[K + k] = py[k];
                    }
                slot[2 * K] = area;
            }
            __syncthreads();
            int next = KP_NONE, pw = 0;
            for (int w = 0; w < n_waves; ++w) {
                const int c = s_cand[b][w];
                if (c != KP_NONE) {
                    next = c;
                    pw = w;
                    break;
                }
            }
            if (next == KP_NONE) break;                           // uniform
            cur = next;
            if (tid == 0 && n_surv < max_det) s_keep[n_surv] = cur;
            ++n_surv;
            if (alive && tid > cur) {
                const float* slot = s_slot[b][pw];
                const double den = (double)((slot[2 * K] + area) / 2.f) + KP_EPS;
                double sum = 0.0;
#pragma unroll
                for (int k = 0; k < KP_MAX_K; ++k)
                    if (k < K) {
                        const float dx = px[k] - slot[k], dy = py[k] - slot[K + k];
                        const float d2 = dx * dx + dy * dy;
                        const double e = (double)d2 / s_var[k] / den / 2.0;
                        sum = sum + exp(-e);
                    }
                const float oks = (float)(sum / (double)K);
                if (oks > oks_thr) alive = false;
            }
            b ^= 1;
        }
    } else {
        n_surv = D;
        if (tid < D && tid < max_det) s_keep[tid] = tid;
    }
    const int E = n_surv < max_det ? n_surv : max_det;
    if (tid < D) {
        order_out[(int64_t)j * d_cap + tid] = s_order[tid];
        alive_out[(int64_t)j * d_cap + tid] = alive ? 1 : 0;
    }
    __syncthreads();
    // the evaluated survivors: loadRes' area, computeOks against every ground truth
    if (tid < E) {
        const float* __restrict__ p = poses + (int64_t)rows[s_order[s_keep[tid]]] * K * 3;
        double x0 = (double)p[0], x1 = x0, y0 = (double)p[1], y1 = y0;
        for (int k = 1; k < K; ++k) {
            const double x = (double)p[3 * k], y = (double)p[3 * k + 1];
            x0 = x < x0 ? x : x0;
            x1 = x > x1 ? x : x1;
            y0 = y < y0 ? y : y0;
            y1 = y > y1 ? y : y1;
        }
        s_darea[tid] = (x1 - x0) * (y1 - y0);
    }
    for (int i = tid; i < E * G; i += (int)blockDim.x) {
        const int e = i / G, g = i % G;
        const float* __restrict__ p = poses + (int64_t)rows[s_order[s_keep[e]]] * K * 3;
        const double* __restrict__ q = gkp + (int64_t)g * K * 3;
        const double den = s_garea[g] + KP_EPS;
        int k1 = 0;
        for (int k = 0; k < K; ++k) k1 += q[3 * k + 2] > 0.0 ? 1 : 0;
        double sum = 0.0;
        if (k1 > 0) {
            for (int k = 0; k < K; ++k) {
                if (!(q[3 * k + 2] > 0.0)) continue;
                const double dx = (double)p[3 * k] - q[3 * k], dy = (double)p[3 * k + 1] - q[3 * k + 1];
                const double ev = (dx * dx + dy * dy) / s_var[k] / den / 2.0;
                sum = sum + exp(-ev);
            }
            sum = sum / (double)k1;
        } else {
            const pa_kpt_gt t = gt[g];
            const double bx0 = t.bbox[0] - t.bbox[2], bx1 = t.bbox[0] + t.bbox[2] * 2.0;
            const double by0 = t.bbox[1] - t.bbox[3], by1 = t.bbox[1] + t.bbox[3] * 2.0;
            for (int k = 0; k < K; ++k) {
                const double xd = (double)p[3 * k], yd = (double)p[3 * k + 1];
                const double ax = bx0 - xd, cx = xd - bx1, ay = by0 - yd, cy = yd - by1;
                const double dx = (ax > 0.0 ? ax : 0.0) + (cx > 0.0 ? cx : 0.0), dy = (ay > 0.0 ? ay : 0.0) + (cy > 0.0 ? cy : 0.0);
                const double ev = (dx * dx + dy * dy) / s_var[k] / den / 2.0;
                sum = sum + exp(-ev);
            }
            sum = sum / (double)K;
        }
        s_oks[e * g_cap + g] = sum;
        oks_out[((int64_t)j * max_det + e) * g_cap + g] = sum;
    }
    // per range: the ignored ground truths
    if (tid < A) coco::ignore_words(s_garea, G, ranges[2 * tid], ranges[2 * tid + 1], s_skip[0], s_skip[1], s_ign[tid]);
    __syncthreads();
    if (tid < A * T) {
        const int a = tid / T, t = tid % T;
        const double thr0 = coco::cap_threshold(thrs[t]), lo = ranges[2 * a], hi = ranges[2 * a + 1];
        const u64 bit = 1ull << (a * T + t);
        const u64 ign0 = s_ign[a][0], ign1 = s_ign[a][1], crowd0 = s_crowd[0], crowd1 = s_crowd[1];
        u64 taken0 = 0ull, taken1 = 0ull;                         // the ground truths matched at this threshold
        for (int r = 0; r < E; ++r) {
            const int m = coco::match_one(s_oks + r * g_cap, G, thr0, ign0, ign1, crowd0, crowd1, taken0, taken1, [](int) { return false; });
            bool ign;
            if (m > -1) {
                atomicOr(&s_matched[r], bit);
                ign = coco::bit_of(ign0, ign1, m);
            } else {
                ign = s_darea[r] < lo || s_darea[r] > hi;
            }
            if (ign) atomicOr(&s_ignored[r], bit);
        }
    }
    __syncthreads();
    if (tid < E) {
        const int r = rows[s_order[s_keep[tid]]];
        pa_kpt_record rec;
        rec.score = scores[r];
        rec.row = r;
        rec.area = s_darea[tid];
        rec.matched = s_matched[tid];
        rec.ignored = s_ignored[tid];
        records[(int64_t)j * max_det + tid] = rec;
    }
    if (tid == 0) {
        flags[j] = 0u;
        record_counts[j] = E;
        survivor_counts[j] = n_surv;
    }
}

}  // namespace

extern "C" {

int64_t pa_kpt_workspace_bytes(int n_jobs, int d_cap, int g_cap, int max_det) {
    if (!caps_ok(n_jobs, d_cap, g_cap, max_det)) return -1;
    return layout(n_jobs, d_cap, g_cap, max_det).end;
}

int64_t pa_kpt_workspace_offset(int n_jobs, int d_cap, int g_cap, int max_det, int which) {
    if (!caps_ok(n_jobs, d_cap, g_cap, max_det) || which < 0 || which > 2) return -1;
    const Layout l = layout(n_jobs, d_cap, g_cap, max_det);
    const int64_t at[3] = {l.order, l.alive, l.oks};
    return at[which];
}

int pa_kpt_poses(const float* preds, const float* maxvals, const float* boxes_f32, int n, int n_keypoints, int heat_w, int heat_h,
                 float vis_thr, float* out_poses, float* out_scores, float* out_areas, hipStream_t stream) {
    if (!preds || !maxvals || !boxes_f32 || !out_poses || !out_scores || !out_areas || n < 1 || n > KP_MAX_BOXES || n_keypoints < 1 ||
        n_keypoints > KP_MAX_K || heat_w < 1 || heat_h < 1 || vis_thr != vis_thr || ((uintptr_t)preds & 7) != 0 ||
        (((uintptr_t)maxvals | (uintptr_t)boxes_f32 | (uintptr_t)out_poses | (uintptr_t)out_scores | (uintptr_t)out_areas) & 3) != 0)
        return (int)hipErrorInvalidValue;
    PA_LAUNCH(kpt_poses_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, preds, maxvals, boxes_f32, n, n_keypoints, (double)heat_w,
              (double)heat_h, vis_thr, out_poses, out_scores, out_areas);
    LAUNCH_CHECK();
}

int pa_kpt_evaluate(const pa_kpt_job* jobs, int n_jobs, const float* poses, const float* scores, const float* areas, int n_rows, int d_cap,
                    int g_cap, int n_keypoints, const double* sigmas_f64, float oks_thr, int max_det, const double* iou_thrs_f64, int n_thrs,
                    const double* area_ranges_f64, int n_ranges, pa_kpt_record* records, void* record_counts, void* survivor_counts,
                    void* flags_u32, void* workspace, hipStream_t stream) {
    if (!jobs || !poses || !scores || !areas || !sigmas_f64 || !iou_thrs_f64 || !area_ranges_f64 || !records || !record_counts ||
        !survivor_counts || !flags_u32 || !workspace || !caps_ok(n_jobs, d_cap, g_cap, max_det) || n_rows < 1 || n_rows > KP_MAX_BOXES ||
        n_keypoints < 1 || n_keypoints > KP_MAX_K || oks_thr != oks_thr || n_thrs < 1 || n_ranges < 1 || n_thrs > KP_MAX_BITS ||
        n_ranges > KP_MAX_BITS || n_thrs * n_ranges > KP_MAX_BITS ||
        (((uintptr_t)jobs | (uintptr_t)sigmas_f64 | (uintptr_t)iou_thrs_f64 | (uintptr_t)area_ranges_f64 | (uintptr_t)records) & 7) != 0 ||
        (((uintptr_t)poses | (uintptr_t)scores | (uintptr_t)areas | (uintptr_t)record_counts | (uintptr_t)survivor_counts |
          (uintptr_t)flags_u32) & 3) != 0 || ((uintptr_t)workspace & 15) != 0)
        return (int)hipErrorInvalidValue;
    const Layout l = layout(n_jobs, d_cap, g_cap, max_det);
    char* ws = static_cast<char*>(workspace);
    const size_t lds = sizeof(double) * (size_t)max_det * (size_t)g_cap;
    static bool attr_done = false;
    if (!attr_done) {
        PA_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kpt_evaluate_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)(sizeof(double) * KP_MAX_E * KP_MAX_G)));
        attr_done = true;
    }
    const unsigned threads = (unsigned)(d_cap <= 128 ? 128 : (d_cap + 63) / 64 * 64);          // two waves hold the ground truths' flags
    PA_LAUNCH(kpt_evaluate_kernel, dim3((unsigned)n_jobs), dim3(threads), lds, stream, jobs, poses, scores, areas, n_rows, d_cap, g_cap,
              n_keypoints, sigmas_f64, oks_thr, max_det, iou_thrs_f64, n_thrs, area_ranges_f64, n_ranges, records, (int32_t*)record_counts,
              (int32_t*)survivor_counts, (uint32_t*)flags_u32, reinterpret_cast<int32_t*>(ws + l.order), reinterpret_cast<int32_t*>(ws + l.alive),
              reinterpret_cast<double*>(ws + l.oks));
    LAUNCH_CHECK();
}

}  // extern "C"
