// Keypoints of painted `coco_pose` pictures on the device: what TopDownCustom.forward_pseudo_test does with a float32 [n][18][H][W] distance
// tensor, 18 masks, 17 masked copies of R, a 107 MB copy to the host, a numpy shift / average and a Python loop over n x 17 heat maps
// (Painter/eval/mmpose_custom/model/top_down.py:163-258, then mmpose's keypoints_from_heatmaps), restated on the bytes of the two
// pictures.  tests/painter_pose_host.py is the definition.
//
//   A pixel of the picture P belongs to ONE class cls_P (first minimum of |G - g_c| + |B - b_c| over the K + 1 palette rows, the last row
//   background); the pixel of the flipped picture Q that flip_back and the one-column shift move onto (y, x) is (y, W - x), and (y, W - 1)
//   for x = 0, and belongs to one class too.  So at a pixel at most two channels of the output are non-zero: cls_P with T[R_P] and
//   pair[cls_Q] with T[R_Q], T[i] = float32(i) / 255.  out = (heat_P + shifted) / 2 in float32: one table look-up each, ONE float32 add,
//   an exact halving -- the reference's own operations, because its argmax and the sign of its neighbour differences depend on how
//   float32 rounds T[a] + T[b] (T[0] + T[3] != T[1] + T[2]).  No heat map and no mask is ever stored.
//
//   peaks  : a workgroup owns 2048 pixels of one box.  Every contribution is a 64-bit key (float bits << 32) | (0xFFFFFFFF - pixel):
//            positive floats order as unsigned integers, so the largest key is the largest value and among equals the first pixel in
//            row-major order -- numpy's argmax.  Keys are maximised in the wave (one butterfly per channel present in the wave), then with
//            LDS atomics, then with one 64-bit vector atomic max per (workgroup, channel) into a zeroed [n][K] table.  max is order-free:
//            the result is deterministic.  Zero values are never candidates: a channel without a positive value keeps key 0.
//   finish : one lane per (box, channel) unpacks the key and evaluates the output at the four neighbours of the peak straight from the
//            two pictures: 0.25 * sign(float32 difference) where 1 < px < W - 1 and 1 < py < H - 1; (-1, -1) and 0 for key 0.
//   heat   : the elementwise statement of the output, for `return_heatmap=True` and for the tests.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/painter_hip.h"
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAX_K = 32;             // keypoint channels
constexpr int PIX_CHUNK = 2048;       // pixels per workgroup of the peak search
constexpr int THREADS = 256;

struct Pose {
    const uint8_t* P;      // [n][H][W][3]
    const uint8_t* Q;      // flipped pictures or NULL
    const int* pal;        // [K + 1][2]
    const int* pair;       // [K]
    int H, W, K, shift;
};

// float32(i) / 255 as the reference computes it: the double quotient rounds to the same float32 for every i in 0..255
// (tests/test_painter_pose_cpu.py), and double division does not depend on how float32 division is compiled.
DEVI float unit(int r) { return (float)((double)r / 255.0); }

// First minimum over the K + 1 rows; pal = the palette in LDS.
DEVI int classify(const int* __restrict__ pal, int K, int g, int b) {
    int best = 0, bd = abs(g - pal[0]) + abs(b - pal[1]);
    for (int c = 1; c <= K; ++c) {
        const int d = abs(g - pal[2 * c]) + abs(b - pal[2 * c + 1]);
        if (d < bd) { bd = d; best = c; }
    }
    return best;
}

// The column of Q that lands on column x after flip_back and the shift.
DEVI int source_column(int x, int W, int shift) { return shift ? (x == 0 ? W - 1 : W - x) : W - 1 - x; }

// The (at most two) channels that are non-zero at pixel (y, x) of box `box`: (c0, v0) from P, (c1, v1) from Q, a channel of -1 = none.
// When c0 == c1 the output of that channel is (v0 + v1) / 2, otherwise v0 / 2 and v1 / 2; without Q it is v0.
DEVI void contributions(const Pose& a, const int* __restrict__ pal, const int* __restrict__ pair, const float* __restrict__ T, int64_t box,
                        int y, int x, int& c0, float& v0, int& c1, float& v1) {
    const int64_t row = (box * a.H + y) * (int64_t)a.W;
    const uint8_t* p = a.P + 3 * (row + x);
    c0 = classify(pal, a.K, p[1], p[2]);
    v0 = T[p[0]];
    if (c0 >= a.K || v0 == 0.0f) c0 = -1;
    c1 = -1;
    v1 = 0.0f;
    if (a.Q) {
        const uint8_t* q = a.Q + 3 * (row + source_column(x, a.W, a.shift));
        const int cq = classify(pal, a.K, q[1], q[2]);
        v1 = T[q[0]];
        if (cq < a.K && v1 != 0.0f) c1 = pair[cq];
    }
}

// out_k(y, x) of the definition.
DEVI float value_of(const Pose& a, const int* __restrict__ pal, const int* __restrict__ pair, const float* __restrict__ T, int64_t box, int y,
                    int x, int k) {
    int c0, c1;
    float v0, v1;
    contributions(a, pal, pair, T, box, y, x, c0, v0, c1, v1);
    const float hp = c0 == k ? v0 : 0.0f;
    if (!a.Q) return hp;
    const float hq = c1 == k ? v1 : 0.0f;
    return (hp + hq) / 2.0f;
}

// Palette, pairs and the table T into LDS; THREADS = 256 threads.
DEVI void stage(const Pose& a, int* pal, int* pair, float* T) {
    const int t = threadIdx.x;
    T[t] = unit(t);
    if (t < 2 * (a.K + 1)) pal[t] = a.pal[t];
    if (t < a.K) {
        const int p = a.pair[t];
        pair[t] = p < 0 ? 0 : (p >= a.K ? a.K - 1 : p);          // a bad table must not index out of bounds
    }
    __syncthreads();
}

DEVI u64 shfl_xor_u64(u64 v, int m) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m);
    return ((u64)hi << 32) | lo;
}

// Every lane brings (channel or -1, key).  Per channel present in the wave: butterfly maximum, then ONE LDS atomic by its first lane.
DEVI void wave_merge(u64* best, int ch, u64 key) {
    const int lane = threadIdx.x & 63;
    u64 pending = __ballot(ch >= 0);
    while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const int c = __shfl(ch, leader);
        const bool mine = ch == c;
        u64 k = mine ? key : 0ull;
#pragma unroll
        for (int m = 32; m; m >>= 1) {
            const u64 o = shfl_xor_u64(k, m);
            k = o > k ? o : k;
        }
        if (lane == leader) atomicMax(&best[c], k);
        pending &= ~__ballot(mine);
    }
}

DEVI u64 make_key(float v, uint32_t pixel) { return ((u64)__float_as_uint(v) << 32) | (u64)(0xFFFFFFFFu - pixel); }

// grid: x = box * chunks + chunk.  keys: u64 [n][K], zeroed.
__global__ __launch_bounds__(THREADS) void pose_peak_kernel(Pose a, u64* __restrict__ keys, int chunks) {
    __shared__ int pal[2 * (MAX_K + 1)];
    __shared__ int pair[MAX_K];
    __shared__ float T[256];
    __shared__ u64 best[MAX_K];
    const int tid = threadIdx.x;
    if (tid < MAX_K) best[tid] = 0ull;
    stage(a, pal, pair, T);
    const int64_t box = blockIdx.x / chunks;
    const int64_t npix = (int64_t)a.H * a.W;
    const int64_t base = (int64_t)(blockIdx.x % chunks) * PIX_CHUNK;
    for (int i = tid; i < PIX_CHUNK; i += THREADS) {          // the trip count is uniform: wave_merge is entered by whole waves
        const int64_t p = base + i;
        int c0 = -1, c1 = -1;
        float v0 = 0.0f, v1 = 0.0f;
        if (p < npix) contributions(a, pal, pair, T, box, (int)(p / a.W), (int)(p % a.W), c0, v0, c1, v1);
        if (a.Q) {
            if (c0 >= 0 && c0 == c1) {
                v0 = (v0 + v1) / 2.0f;
                c1 = -1;
            } else {
                v0 = v0 / 2.0f;
                v1 = v1 / 2.0f;
            }
        }
        wave_merge(best, c0, make_key(v0, (uint32_t)p));
        if (a.Q) wave_merge(best, c1, make_key(v1, (uint32_t)p));
    }
    __syncthreads();
    if (tid < a.K && best[tid] != 0ull) atomicMax(&keys[box * a.K + tid], best[tid]);
}

// thread = (box, channel).
__global__ __launch_bounds__(THREADS) void pose_finish_kernel(Pose a, const u64* __restrict__ keys, float* __restrict__ preds,
                                                              float* __restrict__ maxvals, int64_t total) {
    __shared__ int pal[2 * (MAX_K + 1)];
    __shared__ int pair[MAX_K];
    __shared__ float T[256];
    stage(a, pal, pair, T);
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= total) return;
    const u64 key = keys[i];
    const int64_t pixel = (int64_t)(0xFFFFFFFFu - (uint32_t)key);
    float x = -1.0f, y = -1.0f, m = 0.0f;
    if (key != 0ull && pixel < (int64_t)a.H * a.W) {
        const int64_t box = i / a.K;
        const int k = (int)(i % a.K), px = (int)(pixel % a.W), py = (int)(pixel / a.W);
        m = __uint_as_float((uint32_t)(key >> 32));
        x = (float)px;
        y = (float)py;
        if (1 < px && px < a.W - 1 && 1 < py && py < a.H - 1) {
            const float dx = value_of(a, pal, pair, T, box, py, px + 1, k) - value_of(a, pal, pair, T, box, py, px - 1, k);
            const float dy = value_of(a, pal, pair, T, box, py + 1, px, k) - value_of(a, pal, pair, T, box, py - 1, px, k);
            x += dx > 0.0f ? 0.25f : (dx < 0.0f ? -0.25f : 0.0f);
            y += dy > 0.0f ? 0.25f : (dy < 0.0f ? -0.25f : 0.0f);
        }
    }
    preds[2 * i] = x;
    preds[2 * i + 1] = y;
    maxvals[i] = m;
}

// thread = pixel of a box; writes its K channel values (coalesced along x for every channel).
__global__ __launch_bounds__(THREADS) void pose_heat_kernel(Pose a, float* __restrict__ out, int chunks) {
    __shared__ int pal[2 * (MAX_K + 1)];
    __shared__ int pair[MAX_K];
    __shared__ float T[256];
    stage(a, pal, pair, T);
    const int64_t box = blockIdx.x / chunks;
    const int64_t npix = (int64_t)a.H * a.W;
    const int64_t p = (int64_t)(blockIdx.x % chunks) * THREADS + threadIdx.x;
    if (p >= npix) return;
    int c0, c1;
    float v0, v1;
    contributions(a, pal, pair, T, box, (int)(p / a.W), (int)(p % a.W), c0, v0, c1, v1);
    float* o = out + box * a.K * npix + p;
    for (int k = 0; k < a.K; ++k) {
        const float hp = c0 == k ? v0 : 0.0f;
        o[(int64_t)k * npix] = a.Q ? (hp + (c1 == k ? v1 : 0.0f)) / 2.0f : hp;
    }
}

bool shape_ok(int n, int H, int W, int K, int64_t per_box) {
    if (K < 1 || K > MAX_K || H < 1 || W < 1 || n < 1 || (int64_t)H * W >= ((int64_t)1 << 31)) return false;
    const int64_t chunks = ((int64_t)H * W + per_box - 1) / per_box;
    return chunks * n < ((int64_t)1 << 31);          // one grid dimension
}

}  // namespace

extern "C" {

int64_t pa_pose_workspace_bytes(int n, int n_keypoints) {
    if (n < 1 || n_keypoints < 1 || n_keypoints > MAX_K) return -1;
    return 8 * (int64_t)n * n_keypoints;
}

int pa_pose_keypoints(const void* pictures, const void* flipped, const void* palette_i32, const void* pair_i32, int n, int h, int w,
                      int n_keypoints, int shift, void* workspace, float* out_preds, float* out_maxvals, hipStream_t stream) {
    if (!pictures || !palette_i32 || !pair_i32 || !workspace || !out_preds || !out_maxvals || ((uintptr_t)workspace & 7) != 0 ||
        !shape_ok(n, h, w, n_keypoints, PIX_CHUNK))
        return (int)hipErrorInvalidValue;
    const Pose a = {(const uint8_t*)pictures, (const uint8_t*)flipped, (const int*)palette_i32, (const int*)pair_i32, h, w, n_keypoints,
                    shift ? 1 : 0};
    const int chunks = (int)(((int64_t)h * w + PIX_CHUNK - 1) / PIX_CHUNK);
    const int64_t total = (int64_t)n * n_keypoints;
    PA_TRY(hipMemsetAsync(workspace, 0, 8 * (size_t)total, stream));
    PA_LAUNCH_TRY(pose_peak_kernel, dim3((unsigned)((int64_t)chunks * n)), dim3(THREADS), 0, stream, a, (u64*)workspace, chunks);
    PA_LAUNCH(pose_finish_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream, a, (const u64*)workspace,
              out_preds, out_maxvals, total);
    LAUNCH_CHECK();
}

int pa_pose_heatmaps(const void* pictures, const void* flipped, const void* palette_i32, const void* pair_i32, int n, int h, int w,
                     int n_keypoints, int shift, float* out_heatmaps, hipStream_t stream) {
    if (!pictures || !palette_i32 || !pair_i32 || !out_heatmaps || !shape_ok(n, h, w, n_keypoints, THREADS)) return (int)hipErrorInvalidValue;
    const Pose a = {(const uint8_t*)pictures, (const uint8_t*)flipped, (const int*)palette_i32, (const int*)pair_i32, h, w, n_keypoints,
                    shift ? 1 : 0};
    const int chunks = (int)(((int64_t)h * w + THREADS - 1) / THREADS);
    PA_LAUNCH(pose_heat_kernel, dim3((unsigned)((int64_t)chunks * n)), dim3(THREADS), 0, stream, a, out_heatmaps, chunks);
    LAUNCH_CHECK();
}

}  // extern "C"
