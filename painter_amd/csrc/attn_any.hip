// Attention forward for ANY token grid, and the resize of the rel-pos tables that goes with it (include/painter_anysize.h): the forward at
// a run-time input size other than the constructed one (the reference's get_rel_pos / get_abs_pos make its model size-agnostic;
// Painter/eval/coco_panoptic runs at 1120 x 560 = 70 x 35 tokens on the 896 x 448 checkpoint).
//
// The kernel is the generation-1 forward of attn_fwd.hip -- same work split, same MFMA products, same bias tables, same arithmetic per
// logit -- without its three shape assumptions (L % 32 == 0, Hp % 4 == 0, Wp % 4 == 0):
//   1. a lane's run of 4 keys may cross a key row (or several: Wp < 4): per run two row entries of the bias table and a select per key, the
//      four column entries from a table that repeats its first three behind its end (Wp < 4: (kh, kw) step per key);
//   2. the last 32-key tile may be partial: keys >= L get the logit -inf (weight exactly 0), and their K and V rows are zeros in the LDS
//      images -- they are never read from memory, where they are the next sample's first tokens or nobody's (0 * NaN would be NaN);
//   3. rows >= L of the last query tile run on a copy of row L - 1 (a load that stays inside the sample) and are not stored.
#include "attn_common.h"
#include "attn_any.h"
#include "../../include/painter_hip.h"
#include "../../include/painter_anysize.h"

template <typename T, int NW, int HD>
__global__ __launch_bounds__(NW * 64) void attn_any_kernel(const T* __restrict__ qkv, size_t ldq, const T* __restrict__ rcat,
                                                           T* __restrict__ out, size_t ldo, float* __restrict__ lse, int L, int H,
                                                           int Hp, int Wp, int NRP, float scale, int tab_stride, int TS) {
    typedef KvTile<T, HD> KV;
    constexpr int NT = NW * 64;
    constexpr int KB = KV::KB, VB = KV::VB, KS = KV::KS, DB = KV::DB;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 5;
    const int bh = blockIdx.y, b = bh / H, h = bh % H;
    const int D = H * HD;                            // (TS floats per query: Hp row entries, Wp column entries, the first 3 columns again)
    const T* base = qkv + (size_t)b * L * ldq + h * HD;
    const T* kbase = base + D;
    const T* vbase = base + 2 * D;
    const int qt = blockIdx.x * NW + wave;
    const bool valid = qt * 32 < L;
    const int q = qt * 32 + (lane & 31);
    const int qc = q < L ? q : L - 1;                   // rows >= L of the last tile: a copy of row L - 1, never stored
    unsigned char* const kimg = smem;
    unsigned char* const vimg = smem + 2 * KB;
    unsigned char* const wreg = smem + 2 * KB + 2 * VB + (size_t)wave * tab_stride;
    float* tab = reinterpret_cast<float*>(wreg) + (lane & 31) * TS;
    KV::zero_pad(vimg, tid, NT);
    KV::zero_pad(vimg + VB, tid, NT);

    Frag<T> qf[KS];
    if (valid) {
#pragma unroll
        for (int s = 0; s < KS; ++s) load_gfrag<T>(qf[s], base + (size_t)qc * ldq, s, g);
        build_bias_table<T, HD>(tab, rcat, NRP, qf, qc / Wp, qc % Wp, Hp, Wp, lane);
        if (g == 0 && Wp >= 4) {                        // (same-wave LDS operations are ordered: no barrier)
#pragma unroll
            for (int t = 0; t < 3; ++t) tab[Hp + Wp + t] = tab[Hp + t];
        }
    }

    RowStageB<T, NT, HD> ks;
    TrStageB<T, HD> vs;
    const int ntile = (L + 31) / 32;
    ks.load(kbase, ldq, tid, L);
    vs.load(vbase, ldq, tid, L);
    ks.store(kimg, tid);
    vs.store(vimg, tid);
    __syncthreads();

    f32x16 oacc[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[db][r] = 0.f;
    float m = -INFINITY, l = 0.f;
    const float sl = scale * LOG2E_F;
    // running (key row, key col) of the FIRST key of the four 4-key runs this lane owns in the current tile
    int kh[4], kw[4];
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
        const int ks0 = 8 * rg + 4 * g;
        kh[rg] = ks0 / Wp;
        kw[rg] = ks0 % Wp;
    }
    const int dq_ = 32 / Wp, dr_ = 32 % Wp;

    for (int j = 0; j < ntile; ++j) {
        if (j + 1 < ntile) {
            ks.load(kbase + (size_t)(j + 1) * 32 * ldq, ldq, tid, L - (j + 1) * 32);
            vs.load(vbase + (size_t)(j + 1) * 32 * ldq, ldq, tid, L - (j + 1) * 32);
        }
        const unsigned char* kt = kimg + (j & 1) * KB;
        const unsigned char* vt = vimg + (j & 1) * VB;
        if (valid) {
            f32x16 sacc;
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                Frag<T> kf;
                load_rowfrag<T, HD>(kf, kt, lane & 31, s, g);
                mma(sacc, kf, qf[s]);
            }
            float p[16];
            const int nk = L - j * 32;                  // keys of this tile that exist (>= 1)
            if (Wp >= 4) {
                // a run of 4 keys crosses one key row at the most: keys t < c lie in row kh, the others in row kh + 1, and the column
                // part of the table repeats its first three entries behind its end, so the four columns are consecutive floats.
                // (kh of a key >= L may be Hp or more: clamped, that key's logit is overwritten below)
#pragma unroll
                for (int rg = 0; rg < 4; ++rg) {
                    const float b0 = tab[min(kh[rg], Hp - 1)], b1 = tab[min(kh[rg] + 1, Hp - 1)];
                    const float* tw = tab + Hp + kw[rg];
                    const int c = Wp - kw[rg];
#pragma unroll
                    for (int t = 0; t < 4; ++t) p[rg * 4 + t] = fmaf(sacc[rg * 4 + t], sl, (t < c ? b0 : b1) + tw[t]);
                }
            } else {
#pragma unroll
                for (int rg = 0; rg < 4; ++rg) {        // key rows of 1 - 3 tokens: (kh, kw) step per key
                    int hh = kh[rg], ww = kw[rg];
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        p[rg * 4 + t] = fmaf(sacc[rg * 4 + t], sl, tab[min(hh, Hp - 1)] + tab[Hp + ww]);
                        if (++ww == Wp) { ww = 0; ++hh; }
                    }
                }
            }
            if (nk < 32) {                              // the partial last tile: keys >= L get weight exactly 0
#pragma unroll
                for (int rg = 0; rg < 4; ++rg)
#pragma unroll
                    for (int t = 0; t < 4; ++t)
                        if (8 * rg + 4 * g + t >= nk) p[rg * 4 + t] = -INFINITY;
            }
            float tmax = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; r += 4) tmax = fmaxf(tmax, fmaxf(fmaxf(p[r], p[r + 1]), fmaxf(p[r + 2], p[r + 3])));
            tmax = fmaxf(tmax, lane_xor32(tmax));       // key 0 of the tile exists: finite
            const float mn = fmaxf(m, tmax);
            const float alpha = __builtin_amdgcn_exp2f(m - mn);
            float rs = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                p[r] = __builtin_amdgcn_exp2f(p[r] - mn);
                rs += p[r];
            }
            l = l * alpha + rs;
            m = mn;
#pragma unroll
            for (int db = 0; db < DB; ++db)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[db][r] *= alpha;
            Frag<T> pf[2];
            pack_frag<T>(pf[0], p);
            pack_frag<T>(pf[1], p + 8);
#pragma unroll
            for (int db = 0; db < DB; ++db)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    Frag<T> vf;
                    load_trfrag<T, HD>(vf, vt, db * 32 + (lane & 31), s, g);
                    mma(oacc[db], vf, pf[s]);
                }
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {            // dr_ < Wp: one wrap at the most, whatever Wp
                kh[rg] += dq_;
                kw[rg] += dr_;
                if (kw[rg] >= Wp) { kw[rg] -= Wp; kh[rg] += 1; }
            }
        }
        if (j + 1 < ntile) {
            ks.store(kimg + ((j + 1) & 1) * KB, tid);
            vs.store(vimg + ((j + 1) & 1) * VB, tid);
        }
        __syncthreads();
    }

    // epilogue: normalise, stage O^T through this wave's (now free) table region, store the rows that exist
    unsigned char* stg = wreg;
    constexpr int ROWB = HD * sizeof(T);
    if (valid) {
        const float lt = l + lane_xor32(l);
        const float inv = 1.f / lt;
        if (g == 0 && q < L) lse[(size_t)bh * L + q] = (m + __builtin_amdgcn_logf(lt)) * LN2_F;   // v_log_f32 = log2
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                const int d0 = db * 32 + 8 * rg + 4 * g;
                if (d0 < HD) {                                     // rows d >= HD of the last block are padding
                    T* dst = reinterpret_cast<T*>(stg + (lane & 31) * ROWB) + d0;
                    const float a = oacc[db][rg * 4] * inv, bb = oacc[db][rg * 4 + 1] * inv, c = oacc[db][rg * 4 + 2] * inv,
                                d = oacc[db][rg * 4 + 3] * inv;
                    *reinterpret_cast<typename TT<T>::Vec4*>(dst) = cvt4(a, bb, c, d, (T*)nullptr);
                }
            }
    }
    __syncthreads();
    if (valid) {
        constexpr int CPR = ROWB / 16;
#pragma unroll
        for (int i = 0; i < 32 * CPR / 64; ++i) {
            const int c = lane + 64 * i, row = c / CPR, ch = c % CPR;
            if (qt * 32 + row < L) {
                const uint4 v = *reinterpret_cast<const uint4*>(stg + row * ROWB + ch * 16);
                *reinterpret_cast<uint4*>(out + ((size_t)b * L + qt * 32 + row) * ldo + h * HD + ch * TT<T>::EPC) = v;
            }
        }
    }
}

// floats per query's table: Hp row entries, Wp column entries, the first 3 columns again; odd, so that the 32 tables of a wave start in 32
// different LDS banks (70 x 35, B = 8, 16 heads, bf16: 0.888 ms with the even 108, 0.873 with 109)
static int any_ts(int Hp, int Wp) { return (Hp + Wp + 3) | 1; }
static int any_tab_stride(int Hp, int Wp, int hd, int elem) {
    const int64_t a = (int64_t)32 * any_ts(Hp, Wp) * 4, b = 32 * hd * elem;
    const int64_t s = a > b ? a : b;
    return s > (1 << 20) ? -1 : (int)((s + 15) / 16 * 16);
}
template <typename T, int NW, int HD>
static int attn_any_launch(const T* qkv, int64_t ldq, const T* rcat, T* out, int64_t ldo, float* lse, int Bn, int L, int H, int Hp, int Wp,
                           float scale, hipStream_t st) {
    const int NRP = pa_relpos_rows_padded(Hp, Wp);
    const int ts = any_tab_stride(Hp, Wp, HD, sizeof(T));
    if (ts < 0) return (int)hipErrorInvalidValue;
    const size_t smem = 2 * KvTile<T, HD>::KB + 2 * KvTile<T, HD>::VB + (size_t)NW * ts;
    if (smem > 160 * 1024) return (int)hipErrorInvalidValue;
    auto kern = attn_any_kernel<T, NW, HD>;
    static bool done = false;
    if (!done) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return (int)e;
        done = true;
    }
    const int qtiles = (L + 31) / 32;
    dim3 grid((qtiles + NW - 1) / NW, Bn * H);
    PA_LAUNCH(kern, grid, dim3(NW * 64), smem, st, qkv, (size_t)ldq, rcat, out, (size_t)ldo, lse, L, H, Hp, Wp, NRP, scale, ts, any_ts(Hp, Wp));
    return (int)hipGetLastError();
}
template <typename T>
static int attn_any_t(const void* qkv, int64_t ldq, const void* rcat, void* out, int64_t ldo, float* lse, int Bn, int L, int H, int Hp,
                      int Wp, int hd, float scale, hipStream_t st) {
    const T *q = (const T*)qkv, *r = (const T*)rcat;
    T* o = (T*)out;
    // 4 waves whatever the grid: at 70 x 35 (77 query tiles = 7 * 11) 7 waves would leave no idle wave, but their tables fill the LDS of a CU
    // with ONE workgroup where two of 4 waves fit: 0.873 ms with 7 waves, 0.854 with 4
    if (hd == 80) return attn_any_launch<T, 4, 80>(q, ldq, r, o, ldo, lse, Bn, L, H, Hp, Wp, scale, st);
    return attn_any_launch<T, 4, 64>(q, ldq, r, o, ldo, lse, Bn, L, H, Hp, Wp, scale, st);
}

static long long g_attn_any_launches = 0;
extern "C" int64_t pa_attn_any_launches(void) { return g_attn_any_launches; }

extern "C" int pa_attn_any_fwd(int dtype, const void* qkv, int64_t ldq, const void* rcat, void* out, int64_t ldo, float* lse, int batch,
                               int L, int heads, int Hp, int Wp, int head_dim, float scale, hipStream_t st) {
    if (qkv == nullptr || rcat == nullptr || out == nullptr || lse == nullptr) return (int)hipErrorInvalidValue;
    if (dtype != PA_BF16 && dtype != PA_F32) return (int)hipErrorInvalidValue;
    if (batch < 1 || heads < 1 || Hp < 1 || Wp < 1 || (int64_t)Hp * Wp != L || L > (1 << 24)) return (int)hipErrorInvalidValue;
    if (head_dim != 64 && head_dim != 80) return (int)hipErrorInvalidValue;
    if ((int64_t)batch * heads > 65535) return (int)hipErrorInvalidValue;
    const int es = dtype == PA_BF16 ? 2 : 4;
    // 16-byte vector loads and stores of whole head rows
    if (ldq < (int64_t)3 * heads * head_dim || ldo < (int64_t)heads * head_dim || ldq * es % 16 || ldo * es % 16) return (int)hipErrorInvalidValue;
    if ((uintptr_t)qkv % 16 || (uintptr_t)rcat % 16 || (uintptr_t)out % 16) return (int)hipErrorInvalidValue;
    ++g_attn_any_launches;
    if (dtype == PA_BF16) return attn_any_t<bf16>(qkv, ldq, rcat, out, ldo, lse, batch, L, heads, Hp, Wp, head_dim, scale, st);
    return attn_any_t<float>(qkv, ldq, rcat, out, ldo, lse, batch, L, heads, Hp, Wp, head_dim, scale, st);
}

// ------------------------------------------------------------------------------------------------ rel-pos table resize
// F.interpolate(mode="linear", align_corners=False) along the table's length (util/vitdet_utils.py:79-85), every block, both tables, one launch
__global__ void relpos_resize_kernel(const float* const* __restrict__ tabs, float* __restrict__ dst, int nblocks, int sh, int sw, int dh,
                                     int dw, int hd) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (dh + dw) * hd) return;
    const int blk = blockIdx.y;
    const int r = i / hd, d = i % hd;
    const bool is_w = r >= dh;
    const int j = is_w ? r - dh : r, nin = is_w ? sw : sh, nout = is_w ? dw : dh;
    const float* t = tabs[is_w ? nblocks + blk : blk];
    float v;
    if (nin == nout) {
        v = t[(size_t)j * hd + d];
    } else {
        const float s = fmaxf((float)nin / (float)nout * ((float)j + 0.5f) - 0.5f, 0.f);
        int i0 = (int)s;
        if (i0 > nin - 1) i0 = nin - 1;
        const int i1 = i0 < nin - 1 ? i0 + 1 : i0;
        const float l1 = fminf(fmaxf(s - (float)i0, 0.f), 1.f);
        v = (1.f - l1) * t[(size_t)i0 * hd + d] + l1 * t[(size_t)i1 * hd + d];
    }
    dst[(size_t)blk * (dh + dw) * hd + i] = v;
}
extern "C" int pa_relpos_resize(const void* src_tabs, void* dst, int nblocks, int src_h, int src_w, int dst_h, int dst_w, int head_dim,
                                hipStream_t st) {
    if (src_tabs == nullptr || dst == nullptr || nblocks < 1 || nblocks > 65535 || head_dim < 1) return (int)hipErrorInvalidValue;
    if (src_h < 1 || src_w < 1 || dst_h < 1 || dst_w < 1 || ((int64_t)dst_h + dst_w) * head_dim > (1 << 30)) return (int)hipErrorInvalidValue;
    const int n = (dst_h + dst_w) * head_dim;
    PA_LAUNCH(relpos_resize_kernel, dim3((n + 255) / 256, nblocks), dim3(256), 0, st, reinterpret_cast<const float* const*>(src_tabs),
              (float*)dst, nblocks, src_h, src_w, dst_h, dst_w, head_dim);
    LAUNCH_CHECK();
}
