// Class-agnostic instance decode of a painted picture and Matrix NMS on the device: what the evaluator's default route does with ATen
// ops on [800][H][W][3] float32 difference tensors, float32 masks and a dense fp32 torch.mm
// (Painter/eval/coco_panoptic/COCOCAInstSegEvaluatorCustom.py:252-354, post_process_segm_output_by_threshold; Painter/util/matrix_nms.py:5-121,
// mask_matrix_nms), restated on integers:
//
//   stats         : per (threshold t, colour c): n = #pixels with float(L1) / 3.0f < thr_t, S = sum of L1 over them; L1 = byte-wise
//                   |pixel - colour| summed over the channels = ONE v_sad_u8 on packed bytes.  Lane = colour, the pixel is wave-uniform
//                   (broadcast LDS read), so n and S live in registers and need no cross-lane reduction; integer atomics finish.
//   rank / select : exact rank of every live candidate under  S1 * n2 < S2 * n1  (int64; ties -> lower index t * K + c) by counting,
//                   the first nms_pre are the survivors; score = 1 - maskness / max(largest kept maskness, 1) in float64.  Scores are
//                   non-increasing along the rank, so the stable descending sort before the NMS is the identity.
//   bitmasks      : the survivors' masks recomputed from the picture, [nms_pre][words] uint32, bit b of word w = pixel 32 w + b.
//   intersections : inter[i][j] = sum_w popcount(m_i[w] & m_j[w]), upper triangle, tiled like a GEMM (64 x 64 tile, 4 x 4 accumulators
//                   per lane, 32-word panels in LDS, v_and + v_bcnt = 32 pixel pairs per two VALU ops), split over the words with
//                   integer atomics (order-independent, so deterministic); a wave skips the words at which its rows or the columns are all zero.
//   nms epilogue  : iou, column maximum, decay, column minimum, updated scores -- float64.
//   final         : rank by updated score (descending, ties -> earlier position), first max_num; gather bit masks and indices.
//
// Everything is stream-ordered, allocates nothing and never returns to the host between stages: the survivor count stays on the device
// and every launch is sized by the capacities (T * K candidates, nms_pre survivors).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "../../include/painter_hip.h"
#include "painter_post.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAX_THR = 8;            // thresholds per decode
constexpr int MAX_CAND = 65536;       // T * K
constexpr int MAX_PRE = 4096;         // nms_pre
constexpr int MAX_SIDE = 16384;       // h, w
constexpr int64_t MAX_PIX = 1 << 24;  // h * w: S <= 765 * 2^24 < 2^34, S * n < 2^58
constexpr int PIX_CHUNK = 2048;       // pixels per stats workgroup
constexpr int RANK_SPLIT = 1024;      // candidates per rank workgroup (the j side)
constexpr int MASK_GROUP = 64;        // survivors per bitmask workgroup
constexpr int TILE = 64;              // intersection tile (rows and columns)
constexpr int PANEL = 32;             // words per LDS panel
constexpr int WORD_SPLIT = 1024;      // words per intersection workgroup

struct Layout {
    int64_t cnt, sum, rank, meta, inter, zero_end, surv_idx, surv_col, surv_cut, area, mness, score, ecomp, score2, src, masks, total;
    int ws;                           // mask row stride in words (multiple of 4: 16-byte panel loads)
};

Layout layout(int h, int w, int K, int T, int nms_pre) {
    Layout L;
    const int64_t M = (int64_t)T * K, words = ((int64_t)h * w + 31) / 32;
    L.ws = (int)((words + 3) & ~(int64_t)3);
    int64_t o = 0;
    L.cnt = o;      o = up256(o + 4 * M);
    L.sum = o;      o = up256(o + 8 * M);
    L.rank = o;     o = up256(o + 4 * M);
    L.meta = o;     o = up256(o + 64);
    L.inter = o;    o = up256(o + 4 * (int64_t)nms_pre * nms_pre);
    L.zero_end = o;                                  // [0, zero_end) is cleared at the start of a decode
    L.surv_idx = o; o = up256(o + 4 * (int64_t)nms_pre);
    L.surv_col = o; o = up256(o + 4 * (int64_t)nms_pre);
    L.surv_cut = o; o = up256(o + 4 * (int64_t)nms_pre);
    L.area = o;     o = up256(o + 4 * (int64_t)nms_pre);
    L.mness = o;    o = up256(o + 8 * (int64_t)nms_pre);
    L.score = o;    o = up256(o + 8 * (int64_t)nms_pre);
    L.ecomp = o;    o = up256(o + 8 * (int64_t)nms_pre);
    L.score2 = o;   o = up256(o + 8 * (int64_t)nms_pre);
    L.src = o;      o = up256(o + 4 * (int64_t)nms_pre);
    L.masks = o;    o = up256(o + 4 * (int64_t)nms_pre * L.ws);
    L.total = o;
    return L;
}

bool shape_ok(int h, int w, int K, int T) {
    return h >= 1 && w >= 1 && h <= MAX_SIDE && w <= MAX_SIDE && (int64_t)h * w <= MAX_PIX && K >= 1 && T >= 1 && T <= MAX_THR &&
           (int64_t)T * K <= MAX_CAND;
}

// The mask test  float(L1) / 3.0f < thr  is monotone in the integer L1 in [0, 765]: the number of L1 values that pass is the cut-off,
// mask <=> L1 < cut.  All 256 threads of the workgroup call this; *s_cut must be visible as 0 before (the caller synchronises after).
DEVI void count_cut(int* s_cut, float thr) {
    int c = 0;
    for (int l1 = threadIdx.x; l1 <= 765; l1 += 256) c += ((float)l1 / 3.0f < thr) ? 1 : 0;
    if (c) atomicAdd(s_cut, c);
}

// grid: x = blocks of 256 colours, y = chunks of PIX_CHUNK pixels, z = threshold.
__global__ __launch_bounds__(256) void inst_stats_kernel(const uint8_t* __restrict__ pic, const float* __restrict__ pal,
                                                         const float* __restrict__ thr, uint32_t* __restrict__ cnt, u64* __restrict__ sum,
                                                         int64_t npix, int K) {
    __shared__ __attribute__((aligned(16))) uint32_t px[PIX_CHUNK];
    __shared__ int s_cut;
    const int tid = threadIdx.x, t = blockIdx.z;
    const int64_t base = (int64_t)blockIdx.y * PIX_CHUNK;
    const int valid = (int)(npix - base < PIX_CHUNK ? npix - base : PIX_CHUNK);
    if (tid == 0) s_cut = 0;
    for (int i = tid; i < valid; i += 256) px[i] = pack_pixel(pic, base + i);
    __syncthreads();
    count_cut(&s_cut, thr[t]);
    __syncthreads();
    const uint32_t cut = (uint32_t)s_cut;
    const int c = blockIdx.x * 256 + tid;
    const uint32_t col = c < K ? pack_colour(pal, c) : 0u;
    uint32_t n = 0, s = 0;
    int i = 0;
    for (; i + 4 <= valid; i += 4) {
        const uint4 q = *(const uint4*)&px[i];
        const uint32_t d0 = __builtin_amdgcn_sad_u8(q.x, col, 0u), d1 = __builtin_amdgcn_sad_u8(q.y, col, 0u);
        const uint32_t d2 = __builtin_amdgcn_sad_u8(q.z, col, 0u), d3 = __builtin_amdgcn_sad_u8(q.w, col, 0u);
        n += (d0 < cut) + (d1 < cut) + (d2 < cut) + (d3 < cut);
        s += (d0 < cut ? d0 : 0u) + (d1 < cut ? d1 : 0u) + (d2 < cut ? d2 : 0u) + (d3 < cut ? d3 : 0u);
    }
    for (; i < valid; ++i) {
        const uint32_t d = __builtin_amdgcn_sad_u8(px[i], col, 0u);
        n += d < cut;
        s += d < cut ? d : 0u;
    }
    if (c < K && n) {
        atomicAdd(&cnt[(int64_t)t * K + c], n);
        atomicAdd(&sum[(int64_t)t * K + c], (u64)s);
    }
}

// grid: x = blocks of 256 candidates (the i side), y = splits of RANK_SPLIT candidates (the j side).  rank[i] += #{ live j in the
// split : key_j < key_i, or equal and j < i }, key = S / n compared as S_j * n_i against S_i * n_j; meta[0] += live candidates.
__global__ __launch_bounds__(256) void inst_rank_kernel(const uint32_t* __restrict__ cnt, const u64* __restrict__ sum,
                                                        uint32_t* __restrict__ rank, int* __restrict__ meta, int M) {
    __shared__ uint32_t sn[RANK_SPLIT];
    __shared__ u64 ss[RANK_SPLIT];
    const int tid = threadIdx.x, i = blockIdx.x * 256 + tid;
    const int j0 = blockIdx.y * RANK_SPLIT, nj = M - j0 < RANK_SPLIT ? M - j0 : RANK_SPLIT;
    for (int k = tid; k < nj; k += 256) {
        sn[k] = cnt[j0 + k];
        ss[k] = sum[j0 + k];
    }
    const u64 ni = i < M ? cnt[i] : 0u, si = i < M ? sum[i] : 0u;
    const int live = __syncthreads_count(ni != 0);
    if (blockIdx.y == 0 && tid == 0 && live) atomicAdd(&meta[0], live);
    if (ni == 0) return;
    uint32_t r = 0;
    for (int k = 0; k < nj; ++k) {
        const u64 nk = sn[k];
        const u64 a = ss[k] * ni, b = si * nk;       // key_k < key_i  <=>  S_k * n_i < S_i * n_k
        r += (nk != 0 && (a < b || (a == b && j0 + k < i))) ? 1u : 0u;
    }
    if (r) atomicAdd(&rank[i], r);
}

// One thread per candidate: the first nms_pre of the rank order become the survivors, in rank order.
__global__ __launch_bounds__(256) void inst_select_kernel(const uint32_t* __restrict__ cnt, const u64* __restrict__ sum,
                                                          const uint32_t* __restrict__ rank, const float* __restrict__ pal,
                                                          const float* __restrict__ thr, int* __restrict__ surv_idx,
                                                          uint32_t* __restrict__ surv_col, int* __restrict__ surv_cut, int* __restrict__ area,
                                                          double* __restrict__ mness, int M, int K, int T, int nms_pre) {
    __shared__ int s_cut[MAX_THR];
    if (threadIdx.x < MAX_THR) s_cut[threadIdx.x] = 0;
    __syncthreads();
    for (int t = 0; t < T; ++t) count_cut(&s_cut[t], thr[t]);
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const uint32_t n = cnt[i];
    if (n == 0) return;
    const uint32_t r = rank[i];
    if (r >= (uint32_t)nms_pre) return;
    surv_idx[r] = i;
    surv_col[r] = pack_colour(pal, i % K);
    surv_cut[r] = s_cut[i / K];
    area[r] = (int)n;
    mness[r] = (double)sum[i] / (3.0 * (double)n);
}

// meta[1] = number of survivors; score = 1 - maskness / max(largest kept maskness, 1).  The division is monotone, so the largest kept
// maskness is the last survivor's.
__global__ __launch_bounds__(256) void inst_score_kernel(const double* __restrict__ mness, double* __restrict__ score, int* __restrict__ meta,
                                                         int nms_pre) {
    const int N = meta[0] < nms_pre ? meta[0] : nms_pre;
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r == 0) meta[1] = N;
    if (r >= N) return;
    const double top = mness[N - 1];
    score[r] = 1.0 - mness[r] / (top > 1.0 ? top : 1.0);
}

// grid: x = blocks of 256 words, y = groups of MASK_GROUP survivors.  A thread keeps the 32 pixels of its word in registers and walks
// the survivors of its group (colour and cut-off are wave-uniform loads); consecutive lanes store consecutive words.
__global__ __launch_bounds__(256) void inst_bitmask_kernel(const uint8_t* __restrict__ pic, const uint32_t* __restrict__ surv_col,
                                                           const int* __restrict__ surv_cut, const int* __restrict__ meta,
                                                           uint32_t* __restrict__ masks, int64_t npix, int ws, int nms_pre) {
    const int N = meta[0] < nms_pre ? meta[0] : nms_pre;
    const int w = blockIdx.x * 256 + threadIdx.x;
    const int r0 = blockIdx.y * MASK_GROUP, r1 = r0 + MASK_GROUP < N ? r0 + MASK_GROUP : N;
    if (w >= ws || r0 >= N) return;
    uint32_t px[32];
    uint32_t ok = 0;
#pragma unroll
    for (int b = 0; b < 32; ++b) {
        const int64_t p = (int64_t)w * 32 + b;
        px[b] = p < npix ? pack_pixel(pic, p) : 0u;
        ok |= (p < npix ? 1u : 0u) << b;
    }
    for (int r = r0; r < r1; ++r) {
        const uint32_t col = surv_col[r], cut = (uint32_t)surv_cut[r];
        uint32_t word = 0;
#pragma unroll
        for (int b = 0; b < 32; ++b) word |= (__builtin_amdgcn_sad_u8(px[b], col, 0u) < cut ? 1u : 0u) << b;
        masks[(int64_t)r * ws + w] = word & ok;
    }
}

// grid: x = column tile, y = row tile (x >= y: upper triangle), z = split of WORD_SPLIT words.  256 threads, thread (tx, ty) = (tid & 15,
// tid >> 4) owns rows 4 ty .. 4 ty + 3 and columns 4 tx .. 4 tx + 3 of the tile.  Panels sit in LDS as [word][row], so the four rows
// (columns) of a thread are one 16-byte read: per word 2 reads feed 16 v_and + 16 v_bcnt.  A mask covers a few per cent of the picture, so
// most words of most rows are zero: while staging, the threads record per panel WHICH words hold a bit in the 16 rows of each wave
// (flag[.][wave]) and in any of the 64 columns (flag[.][4]); a wave walks only the words set in both -- a wave-uniform bit scan, the
// skipped terms are exact zeros.  The flags alternate between two sets, the idle one is cleared while the other is in use.
// n_dev (if not NULL) overrides n_rows.
__global__ __launch_bounds__(256) void inst_inter_kernel(const uint32_t* __restrict__ masks, const int* __restrict__ n_dev, int n_rows,
                                                         int ws, int* __restrict__ inter, int ld) {
    __shared__ __attribute__((aligned(16))) uint32_t A[PANEL][TILE];
    __shared__ __attribute__((aligned(16))) uint32_t B[PANEL][TILE];
    __shared__ uint32_t flag[2][8];
    static_assert(PANEL == 32 && TILE == 64, "one flag bit per panel word, one flag word per wave");
    const int N = n_dev ? (*n_dev < n_rows ? *n_dev : n_rows) : n_rows;
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (tj < ti || tj * TILE >= N) return;                       // uniform over the workgroup
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int kbeg = blockIdx.z * WORD_SPLIT, kend = kbeg + WORD_SPLIT < ws ? kbeg + WORD_SPLIT : ws;
    uint32_t acc[4][4] = {};
    if (tid < 16) flag[tid >> 3][tid & 7] = 0;
    __syncthreads();
    int p = 0;
    for (int k0 = kbeg; k0 < kend; k0 += PANEL, p ^= 1) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int idx = tid + 256 * e, row = idx >> 3, kk = 4 * (idx & 7), k = k0 + kk;
            const int gi = ti * TILE + row, gj = tj * TILE + row;
            uint4 a = make_uint4(0, 0, 0, 0), b = make_uint4(0, 0, 0, 0);
            if (k < kend) {                                      // ws and the split are multiples of 4: the 16 bytes are inside the row
                if (gi < N) a = *(const uint4*)&masks[(int64_t)gi * ws + k];
                if (gj < N) b = *(const uint4*)&masks[(int64_t)gj * ws + k];
            }
            A[kk][row] = a.x; A[kk + 1][row] = a.y; A[kk + 2][row] = a.z; A[kk + 3][row] = a.w;
            B[kk][row] = b.x; B[kk + 1][row] = b.y; B[kk + 2][row] = b.z; B[kk + 3][row] = b.w;
            const uint32_t bits_a = ((a.x ? 1u : 0u) | (a.y ? 2u : 0u) | (a.z ? 4u : 0u) | (a.w ? 8u : 0u)) << kk;
            const uint32_t bits_b = ((b.x ? 1u : 0u) | (b.y ? 2u : 0u) | (b.z ? 4u : 0u) | (b.w ? 8u : 0u)) << kk;
            if (bits_a) atomicOr(&flag[p][row >> 4], bits_a);
            if (bits_b) atomicOr(&flag[p][4], bits_b);
        }
        __syncthreads();
        if (tid < 8) flag[p ^ 1][tid] = 0;                       // last read before the barrier that ended the previous panel
        uint32_t ks = __builtin_amdgcn_readfirstlane(flag[p][tid >> 6] & flag[p][4]);
        while (ks) {
            const int k = __builtin_ctz(ks);
            ks &= ks - 1;
            const uint4 a = *(const uint4*)&A[k][4 * ty];
            const uint4 b = *(const uint4*)&B[k][4 * tx];
            const uint32_t av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int ii = 0; ii < 4; ++ii)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) acc[ii][jj] += __popc(av[ii] & bv[jj]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int ii = 0; ii < 4; ++ii)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int gi = ti * TILE + 4 * ty + ii, gj = tj * TILE + 4 * tx + jj;
            if (gi < N && gj < N && acc[ii][jj]) atomicAdd(&inter[(int64_t)gi * ld + gj], (int)acc[ii][jj]);
        }
}

DEVI double iou_of(int v, int ai, int aj) { return (double)v / (double)(ai + aj - v); }

// Column passes of the NMS, block (64 columns, 16 row lanes).  Only i < j enters: the reference's matrices are zero on and below the
// diagonal, where iou = 0 gives decay = 1 / e_i >= 1, while row 0 (compensation 0, e_0 = 1) gives decay <= 1 in every column j >= 1 --
// so entries with inter = 0 never lower a column minimum below what row 0 leaves, and the minimum starts from 1.
// PASS 0: ecomp[j] = exp(-sigma * comp_j^2) (gaussian) or 1 - comp_j (linear), comp_j = max_i iou[i][j].
// PASS 1: score2[j] = score[j] * min_i decay[i][j], decay = exp(-sigma * iou^2) / ecomp[i] or (1 - iou) / ecomp[i]; NaN (0 / 0 of
// the linear kernel on identical masks) propagates as it does in the reference.
template <int PASS>
__global__ __launch_bounds__(1024) void inst_nms_kernel(const int* __restrict__ inter, int ld, const int* __restrict__ area,
                                                        const int* __restrict__ meta, const double* __restrict__ score,
                                                        double* __restrict__ ecomp, double* __restrict__ score2, double sigma, int linear) {
    __shared__ double red[16][64];
    const int N = meta[1];
    const int tx = threadIdx.x, ty = threadIdx.y, j = blockIdx.x * 64 + tx;
    if (blockIdx.x * 64 >= N) return;
    double m = PASS == 0 ? 0.0 : 1.0;
    if (j < N) {
        const int aj = area[j];
        for (int i = ty; i < j; i += 16) {
            const int v = inter[(int64_t)i * ld + j];
            if (v == 0) continue;
            const double iou = iou_of(v, area[i], aj);
            if (PASS == 0) {
                m = iou > m ? iou : m;
            } else {
                const double d = (linear ? 1.0 - iou : exp(-1.0 * sigma * (iou * iou))) / ecomp[i];
                m = (d < m || d != d) ? d : m;
            }
        }
    }
    red[ty][tx] = m;
    __syncthreads();
    if (ty == 0 && j < N) {
        for (int k = 1; k < 16; ++k) {
            const double d = red[k][tx];
            if (PASS == 0) m = d > m ? d : m;
            else m = (d < m || d != d) ? d : m;
        }
        if (PASS == 0) ecomp[j] = linear ? 1.0 - m : exp(-1.0 * sigma * (m * m));
        else score2[j] = score[j] * m;
    }
}

// One thread per survivor: its position in the descending order of the updated scores (NaN first, as torch.sort places it; ties ->
// earlier position); the first max_num go out.
__global__ __launch_bounds__(256) void inst_final_kernel(const double* __restrict__ score2, const int* __restrict__ surv_idx,
                                                         const int* __restrict__ meta, int* __restrict__ src, int* __restrict__ out_count,
                                                         float* __restrict__ out_scores, double* __restrict__ out_scores64,
                                                         int* __restrict__ out_idx, int max_num) {
    const int N = meta[1];
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j == 0) *out_count = N < max_num ? N : max_num;
    if (j >= N) return;
    const double sj = score2[j], kj = sj != sj ? INFINITY : sj;
    int r = 0;
    for (int k = 0; k < N; ++k) {
        const double sk = score2[k], kk = sk != sk ? INFINITY : sk;
        r += (kk > kj || (kk == kj && k < j)) ? 1 : 0;
    }
    if (r < max_num) {
        src[r] = j;
        out_scores[r] = (float)sj;
        if (out_scores64) out_scores64[r] = sj;
        out_idx[r] = surv_idx[j];
    }
}

// grid: x = blocks of 256 words, y = output row.  Rows past the count are cleared.  out_bytes (optional): the same masks with one byte
// per pixel, [max_num][npix] -- what a caller hands on as a bool array without unpacking 100 x H x W bits on the host.
__global__ __launch_bounds__(256) void inst_gather_kernel(const uint32_t* __restrict__ masks, const int* __restrict__ src,
                                                          const int* __restrict__ out_count, uint32_t* __restrict__ out_masks,
                                                          uint8_t* __restrict__ out_bytes, int words, int ws, int64_t npix) {
    const int w = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (w >= words) return;
    const uint32_t word = r < *out_count ? masks[(int64_t)src[r] * ws + w] : 0u;
    out_masks[(int64_t)r * words + w] = word;
    if (out_bytes) {
        const int64_t p0 = (int64_t)w * 32;
        const int nb = npix - p0 < 32 ? (int)(npix - p0) : 32;
        uint8_t* o = out_bytes + (int64_t)r * npix + p0;
        for (int b = 0; b < nb; ++b) o[b] = (uint8_t)((word >> b) & 1u);
    }
}

int launch_stats(const uint8_t* pic, const float* pal, const float* thr, uint32_t* cnt, u64* sum, int h, int w, int K, int T,
                 hipStream_t stream) {
    const int64_t npix = (int64_t)h * w;
    const dim3 grid((unsigned)((K + 255) / 256), (unsigned)((npix + PIX_CHUNK - 1) / PIX_CHUNK), (unsigned)T);
    PA_LAUNCH(inst_stats_kernel, grid, dim3(256), 0, stream, pic, pal, thr, cnt, sum, npix, K);
    return (int)hipGetLastError();
}

int launch_inter(const uint32_t* masks, const int* n_dev, int n_rows, int ws, int* inter, int ld, hipStream_t stream) {
    const unsigned tiles = (unsigned)((n_rows + TILE - 1) / TILE);
    const dim3 grid(tiles, tiles, (unsigned)((ws + WORD_SPLIT - 1) / WORD_SPLIT));
    PA_LAUNCH(inst_inter_kernel, grid, dim3(256), 0, stream, masks, n_dev, n_rows, ws, inter, ld);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int64_t pa_inst_workspace_bytes(int h, int w, int n_colours, int n_thr, int nms_pre) {
    if (!shape_ok(h, w, n_colours, n_thr) || nms_pre < 1 || nms_pre > MAX_PRE) return -1;
    return layout(h, w, n_colours, n_thr, nms_pre).total;
}

int64_t pa_inst_workspace_offset(int h, int w, int n_colours, int n_thr, int nms_pre, int section) {
    if (!shape_ok(h, w, n_colours, n_thr) || nms_pre < 1 || nms_pre > MAX_PRE) return -1;
    const Layout L = layout(h, w, n_colours, n_thr, nms_pre);
    switch (section) {
        case 0: return L.cnt;
        case 1: return L.sum;
        case 2: return L.meta;
        case 3: return L.surv_idx;
        case 4: return L.area;
        case 5: return L.score;
        case 6: return L.masks;
        case 7: return L.inter;
        case 8: return L.score2;
        case 9: return L.ws;
        default: return -1;
    }
}

int pa_inst_stats(const void* picture, const float* palette, const float* thresholds, void* n_u32, void* s_u64, int h, int w,
                  int n_colours, int n_thr, hipStream_t stream) {
    if (!picture || !palette || !thresholds || !n_u32 || !s_u64 || !shape_ok(h, w, n_colours, n_thr)) return (int)hipErrorInvalidValue;
    const int64_t M = (int64_t)n_thr * n_colours;
    PA_TRY(hipMemsetAsync(n_u32, 0, 4 * M, stream));
    PA_TRY(hipMemsetAsync(s_u64, 0, 8 * M, stream));
    return launch_stats((const uint8_t*)picture, palette, thresholds, (uint32_t*)n_u32, (u64*)s_u64, h, w, n_colours, n_thr, stream);
}

int pa_inst_intersections(const void* masks_u32, int n_rows, int words, void* inter_i32, int ld, hipStream_t stream) {
    if (!masks_u32 || !inter_i32 || n_rows < 1 || n_rows > MAX_PRE || words < 4 || words % 4 != 0 || ld < n_rows ||
        ((uintptr_t)masks_u32 & 15) != 0)
        return (int)hipErrorInvalidValue;
    PA_TRY(hipMemsetAsync(inter_i32, 0, 4 * (int64_t)n_rows * ld, stream));
    return launch_inter((const uint32_t*)masks_u32, nullptr, n_rows, words, (int*)inter_i32, ld, stream);
}

int pa_inst_decode(const void* picture, const float* palette, const float* thresholds, int h, int w, int n_colours, int n_thr, int nms_pre,
                   int max_num, float sigma, int kernel, void* workspace, void* out_count, float* out_scores, void* out_scores_f64,
                   void* out_candidates, void* out_masks, void* out_masks_u8, hipStream_t stream) {
    if (!picture || !palette || !thresholds || !workspace || !out_count || !out_scores || !out_candidates || !out_masks ||
        !shape_ok(h, w, n_colours, n_thr) || nms_pre < 1 || nms_pre > MAX_PRE || max_num < 1 || max_num > nms_pre || kernel < 0 ||
        kernel > 1 || !(sigma == sigma) || ((uintptr_t)workspace & 255) != 0)
        return (int)hipErrorInvalidValue;
    const Layout L = layout(h, w, n_colours, n_thr, nms_pre);
    char* ws = (char*)workspace;
    uint32_t* cnt = (uint32_t*)(ws + L.cnt);
    u64* sum = (u64*)(ws + L.sum);
    uint32_t* rank = (uint32_t*)(ws + L.rank);
    int* meta = (int*)(ws + L.meta);
    int* inter = (int*)(ws + L.inter);
    int* surv_idx = (int*)(ws + L.surv_idx);
    uint32_t* surv_col = (uint32_t*)(ws + L.surv_col);
    int* surv_cut = (int*)(ws + L.surv_cut);
    int* area = (int*)(ws + L.area);
    double* mness = (double*)(ws + L.mness);
    double* score = (double*)(ws + L.score);
    double* ecomp = (double*)(ws + L.ecomp);
    double* score2 = (double*)(ws + L.score2);
    int* src = (int*)(ws + L.src);
    uint32_t* masks = (uint32_t*)(ws + L.masks);
    const uint8_t* pic = (const uint8_t*)picture;
    const int M = n_thr * n_colours;
    const int64_t npix = (int64_t)h * w;
    const int words = (int)((npix + 31) / 32);

    PA_TRY(hipMemsetAsync(ws, 0, (size_t)L.zero_end, stream));
    PA_TRY(hipMemsetAsync(out_scores, 0, 4 * (size_t)max_num, stream));
    PA_TRY(hipMemsetAsync(out_candidates, 0, 4 * (size_t)max_num, stream));
    if (out_scores_f64) PA_TRY(hipMemsetAsync(out_scores_f64, 0, 8 * (size_t)max_num, stream));
    PA_TRY(launch_stats(pic, palette, thresholds, cnt, sum, h, w, n_colours, n_thr, stream));
    PA_LAUNCH_TRY(inst_rank_kernel, dim3((unsigned)((M + 255) / 256), (unsigned)((M + RANK_SPLIT - 1) / RANK_SPLIT)), dim3(256), 0, stream, cnt,
                  sum, rank, meta, M);
    PA_LAUNCH_TRY(inst_select_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, stream, cnt, sum, rank, palette, thresholds, surv_idx,
                  surv_col, surv_cut, area, mness, M, n_colours, n_thr, nms_pre);
    const unsigned pre_blocks = (unsigned)((nms_pre + 255) / 256);
    PA_LAUNCH_TRY(inst_score_kernel, dim3(pre_blocks), dim3(256), 0, stream, mness, score, meta, nms_pre);
    PA_LAUNCH_TRY(inst_bitmask_kernel, dim3((unsigned)((L.ws + 255) / 256), (unsigned)((nms_pre + MASK_GROUP - 1) / MASK_GROUP)), dim3(256), 0,
                  stream, pic, surv_col, surv_cut, meta, masks, npix, L.ws, nms_pre);
    PA_TRY(launch_inter(masks, meta + 1, nms_pre, L.ws, inter, nms_pre, stream));
    const dim3 nms_grid((unsigned)((nms_pre + 63) / 64)), nms_block(64, 16);
    PA_LAUNCH_TRY(inst_nms_kernel<0>, nms_grid, nms_block, 0, stream, inter, nms_pre, area, meta, score, ecomp, score2, (double)sigma, kernel);
    PA_LAUNCH_TRY(inst_nms_kernel<1>, nms_grid, nms_block, 0, stream, inter, nms_pre, area, meta, score, ecomp, score2, (double)sigma, kernel);
    PA_LAUNCH_TRY(inst_final_kernel, dim3(pre_blocks), dim3(256), 0, stream, score2, surv_idx, meta, src, (int*)out_count, out_scores,
                  (double*)out_scores_f64, (int*)out_candidates, max_num);
    PA_LAUNCH(inst_gather_kernel, dim3((unsigned)((words + 255) / 256), (unsigned)max_num), dim3(256), 0, stream, masks, src,
              (const int*)out_count, (uint32_t*)out_masks, (uint8_t*)out_masks_u8, words, L.ws, npix);
    LAUNCH_CHECK();
}

}  // extern "C"
