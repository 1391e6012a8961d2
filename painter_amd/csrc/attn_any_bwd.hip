// Attention backward for ANY token grid, and the adjoint of the rel-pos table resize (include/painter_anysize_grad.h): the backward at a
// run-time input size other than the constructed one.
//
// The kernels are the generation-1 backward of attn_bwd.hip -- same work split (Delta, kernel A: dQ + bias-gradient tables, kernel B: dK / dV,
// table contraction on the GEMM engine), same MFMA products, same arithmetic per logit -- without its three shape assumptions
// (L % 32 == 0, Hp % 4 == 0, Wp % 4 == 0), the way attn_any.hip restates the forward:
//   1. a run of keys may cross a key row (or several: Wp < 4): the bias read keeps a key's own (row, column) as the forward does, and the
//      scatter of dS into the per-query (kh | kw) gradient tables walks the 8 keys the two half-waves of a query hold for one register
//      group: half 0 adds the row sums, half 1 the column sums, each with plain in-order read-modify-writes of entries only it touches
//      (attn_bwd.hip uses LDS float atomics where the two halves meet; here the halves exchange their dS first: no atomics);
//   2. the last 32-key tile may be partial: keys >= L get P = 0 and dS = 0 exactly, and their K and V rows are zeros in the LDS images;
//   3. query rows >= L of the last query tile: kernel A runs them on zeros (Q = dO = 0, lse = Delta = 0: dS = 0) and stores nothing of them;
//      kernel B stages zeros for their Q and dO rows and forces their P and dS to 0.
#include "attn_common.h"
#include "attn_any.h"
#include "../../include/painter_hip.h"
#include "../../include/painter_anysize_grad.h"

template <typename T> DEVI void zero_frag(Frag<T>& f) {
    if constexpr (sizeof(T) == 2) f.set(zero4());
    else f.set(zero4(), zero4());
}

// floats per query: the bias table as attn_any.hip lays it out (Hp row entries, Wp column entries, the first 3 columns again; odd), and
// the gradient table (Hp row sums, Wp column sums; odd)
static int anyb_ts(int Hp, int Wp) { return (Hp + Wp + 3) | 1; }
static int anyb_tg(int Hp, int Wp) { return (Hp + Wp) | 1; }

// ------------------------------------------------------------------------------- kernel A: dQ + bias-gradient tables
template <typename T, int NW, int HD>
__global__ __launch_bounds__(NW * 64) void attn_any_bwd_dq_kernel(const T* __restrict__ qkv, size_t ldq, const T* __restrict__ rcat,
                                                                  const T* __restrict__ rcatT, const T* __restrict__ dout, size_t lddo,
                                                                  const float* __restrict__ lse, const float* __restrict__ delta,
                                                                  T* __restrict__ dqkv, T* __restrict__ dG, float* __restrict__ aux, int L,
                                                                  int H, int Hp, int Wp, int NRP, float scale, int tab_stride, int TS, int TG) {
    typedef KvTile<T, HD> KV;
    constexpr int NT = NW * 64;
    constexpr int KB = KV::KB, VB = KV::VB, KS = KV::KS, DB = KV::DB;
    constexpr int STG = 2 * KB + VB;           // one stage: K row image, V row image, K^T image
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 5;
    const int bh = blockIdx.y, b = bh / H, h = bh % H;
    const int D = H * HD, TA = Hp + Wp;
    const int ntile = (L + 31) / 32;
    const T* base = qkv + (size_t)b * L * ldq + h * HD;
    const T* kbase = base + D;
    const T* vbase = base + 2 * D;
    const int qt = blockIdx.x * NW + wave;
    const bool valid = qt * 32 < L;
    const int q = qt * 32 + (lane & 31);
    const bool qlive = q < L;
    const int qc = qlive ? q : L - 1;          // (table indices of a row >= L stay inside the table; nothing of such a row is loaded)
    const int qh = qc / Wp, qw = qc % Wp;
    unsigned char* wreg = smem + 2 * STG + (size_t)wave * tab_stride;
    KV::zero_pad(smem + 2 * KB, tid, NT);
    KV::zero_pad(smem + STG + 2 * KB, tid, NT);
    float* tab = reinterpret_cast<float*>(wreg) + (lane & 31) * TS;
    float* tabg = reinterpret_cast<float*>(wreg) + 32 * TS + (lane & 31) * TG;

    Frag<T> qf[KS], dof[KS];
    float lse2 = 0.f, dlt = 0.f;
    if (valid) {
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            if (qlive) {
                load_gfrag<T>(qf[s], base + (size_t)q * ldq, s, g);
                load_gfrag<T>(dof[s], dout + ((size_t)b * L + q) * lddo + h * HD, s, g);
            } else {
                zero_frag<T>(qf[s]);
                zero_frag<T>(dof[s]);
            }
        }
        if (qlive) {
            lse2 = lse[(size_t)bh * L + q] * LOG2E_F;
            dlt = delta[(size_t)bh * L + q];
        }
        build_bias_table<T, HD>(tab, rcat, NRP, qf, qh, qw, Hp, Wp, lane);      // (a row >= L: Q = 0, a table of zeros)
        if (g == 0 && Wp >= 4) {                        // (same-wave LDS operations are ordered: no barrier)
#pragma unroll
            for (int t = 0; t < 3; ++t) tab[Hp + Wp + t] = tab[Hp + t];
        }
        for (int c = g; c < TA; c += 2) tabg[c] = 0.f;
        // export the transposed table + per-row scalars for kernel B (rows >= L: zeros; kernel B does not use them)
        float* ax = aux + ((size_t)bh * ntile + qt) * (TA + 2) * 32 + (lane & 31);
        for (int c = g; c < TA; c += 2) ax[(size_t)c * 32] = tab[c];
        if (g == 0) ax[(size_t)TA * 32] = lse2;
        else ax[(size_t)(TA + 1) * 32] = dlt;
    }

    RowStageB<T, NT, HD> ks, vs;
    TrStageB<T, HD> kts;
    ks.load(kbase, ldq, tid, L);
    kts.load(kbase, ldq, tid, L);
    vs.load(vbase, ldq, tid, L);
    ks.store(smem, tid);
    vs.store(smem + KB, tid);
    kts.store(smem + 2 * KB, tid);
    __syncthreads();

    f32x16 dq[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) dq[db][r] = 0.f;
    const float sl = scale * LOG2E_F;
    // running (key row, key col) of key 8 * rg of the current tile: the first of the 8 keys the two halves of a query hold for group rg
    int kh8[4], kw8[4];
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
        kh8[rg] = 8 * rg / Wp;
        kw8[rg] = 8 * rg % Wp;
    }
    const int dq_ = 32 / Wp, dr_ = 32 % Wp;

    for (int j = 0; j < ntile; ++j) {
        if (j + 1 < ntile) {
            const T* kp = kbase + (size_t)(j + 1) * 32 * ldq;
            const int nr = L - (j + 1) * 32;
            ks.load(kp, ldq, tid, nr);
            kts.load(kp, ldq, tid, nr);
            vs.load(vbase + (size_t)(j + 1) * 32 * ldq, ldq, tid, nr);
        }
        const unsigned char* st = smem + (j & 1) * STG;
        if (valid) {
            f32x16 sacc, dpacc;
#pragma unroll
            for (int r = 0; r < 16; ++r) { sacc[r] = 0.f; dpacc[r] = 0.f; }
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                Frag<T> kf, vf;
                load_rowfrag<T, HD>(kf, st, lane & 31, s, g);
                load_rowfrag<T, HD>(vf, st + KB, lane & 31, s, g);
                mma(sacc, kf, qf[s]);
                mma(dpacc, vf, dof[s]);
            }
            const int nk = L - j * 32;                  // keys of this tile that exist (>= 1)
            float ds[16];
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                // this lane's own run of 4 keys starts 4 * g keys behind key 8 * rg
                int hh = kh8[rg], ww = kw8[rg];
                if (g) {
                    ww += 4;
                    while (ww >= Wp) { ww -= Wp; ++hh; }
                }
                float bias[4];
                if (Wp >= 4) {                          // one row crossing at the most; the column part repeats its first three entries
                    const float b0 = tab[min(hh, Hp - 1)], b1 = tab[min(hh + 1, Hp - 1)];
                    const float* tw = tab + Hp + ww;
                    const int c = Wp - ww;
#pragma unroll
                    for (int t = 0; t < 4; ++t) bias[t] = (t < c ? b0 : b1) + tw[t];
                } else {
#pragma unroll
                    for (int t = 0; t < 4; ++t) {       // key rows of 1 - 3 tokens: (kh, kw) step per key
                        bias[t] = tab[min(hh, Hp - 1)] + tab[Hp + ww];
                        if (++ww == Wp) { ww = 0; ++hh; }
                    }
                }
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int r = rg * 4 + t;
                    const float p = __builtin_amdgcn_exp2f(fmaf(sacc[r], sl, bias[t]) - lse2);
                    ds[r] = (8 * rg + 4 * g + t < nk) ? p * (dpacc[r] - dlt) : 0.f;      // keys >= L: dS exactly 0
                }
                // the 8 values of keys 8 rg .. 8 rg + 7 of this query, in key order, in both halves
                float v8[8];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float own = ds[rg * 4 + t], oth = lane_xor32(own);
                    v8[t] = g ? oth : own;
                    v8[4 + t] = g ? own : oth;
                }
                hh = kh8[rg];
                ww = kw8[rg];
                if (g == 0) {                           // row sums (a key >= L: 0 into a clamped entry)
                    if (Wp >= 8) {
                        const int c = Wp - ww;
                        float r0 = 0.f, r1 = 0.f;
#pragma unroll
                        for (int t = 0; t < 8; ++t) { if (t < c) r0 += v8[t]; else r1 += v8[t]; }
                        tabg[min(hh, Hp - 1)] += r0;
                        if (hh + 1 < Hp) tabg[hh + 1] += r1;       // (otherwise r1 sums keys >= L only: exactly 0)
                    } else {
                        float acc = 0.f;
#pragma unroll
                        for (int t = 0; t < 8; ++t) {
                            acc += v8[t];
                            if (++ww == Wp) {
                                ww = 0;
                                tabg[min(hh, Hp - 1)] += acc;
                                acc = 0.f;
                                ++hh;
                            }
                        }
                        tabg[min(hh, Hp - 1)] += acc;
                    }
                } else {                                // column sums
                    if (Wp >= 8) {                      // 8 different columns
                        int col[8];
                        float cur[8];
#pragma unroll
                        for (int t = 0; t < 8; ++t) {
                            col[t] = ww;
                            if (++ww == Wp) ww = 0;
                        }
#pragma unroll
                        for (int t = 0; t < 8; ++t) cur[t] = tabg[Hp + col[t]];
#pragma unroll
                        for (int t = 0; t < 8; ++t) tabg[Hp + col[t]] = cur[t] + v8[t];
                    } else {
#pragma unroll
                        for (int t = 0; t < 8; ++t) {
                            tabg[Hp + ww] += v8[t];
                            if (++ww == Wp) ww = 0;
                        }
                    }
                }
            }
            Frag<T> dsf[2];
            pack_frag<T>(dsf[0], ds);
            pack_frag<T>(dsf[1], ds + 8);
#pragma unroll
            for (int db = 0; db < DB; ++db)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    Frag<T> ktf;
                    load_trfrag<T, HD>(ktf, st + 2 * KB, db * 32 + (lane & 31), s, g);
                    mma(dq[db], ktf, dsf[s]);
                }
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {            // dr_ < Wp: one wrap at the most, whatever Wp
                kh8[rg] += dq_;
                kw8[rg] += dr_;
                if (kw8[rg] >= Wp) { kw8[rg] -= Wp; kh8[rg] += 1; }
            }
        }
        if (j + 1 < ntile) {
            unsigned char* sn = smem + ((j + 1) & 1) * STG;
            ks.store(sn, tid);
            vs.store(sn + KB, tid);
            kts.store(sn + 2 * KB, tid);
        }
        __syncthreads();
    }

    // bias part of dQ through r-space: dQ^T[d][q] = scale * acc + sum_r Rcat[r][d] dG[q][r]; also emit dG (T) for the rows that exist
    constexpr int ROWB = HD * sizeof(T);
    if (valid) {
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) dq[db][r] *= scale;
        T* dgrow = dG + (((size_t)b * L + qc) * H + h) * NRP;
        for (int s = 0; s < NRP / 16; ++s) {
            float gv[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const int r = 16 * s + 8 * g + t;
                float v = 0.f;
                if (r < 2 * Hp - 1) {
                    const int khh = qh + Hp - 1 - r;
                    if (khh >= 0 && khh < Hp) v = tabg[khh];
                } else {
                    const int rr = r - (2 * Hp - 1);
                    const int kww = qw + Wp - 1 - rr;
                    if (rr < 2 * Wp - 1 && kww >= 0 && kww < Wp) v = tabg[Hp + kww];
                }
                gv[t] = v;
            }
            Frag<T> gf;
            pack_frag<T>(gf, gv);
            if (qlive) {
                if constexpr (sizeof(T) == 2) {
                    *reinterpret_cast<uint4*>(dgrow + 16 * s + 8 * g) = __builtin_bit_cast(uint4, gf.v);
                } else {
                    *reinterpret_cast<float4*>(dgrow + 16 * s + 8 * g) = make_float4(gv[0], gv[1], gv[2], gv[3]);
                    *reinterpret_cast<float4*>(dgrow + 16 * s + 8 * g + 4) = make_float4(gv[4], gv[5], gv[6], gv[7]);
                }
            }
#pragma unroll
            for (int db = 0; db < DB; ++db) {
                Frag<T> rf;
                const int dr = db * 32 + (lane & 31);                                  // rows d >= HD of the last block: zero operand
                const T* rp = rcatT + (size_t)(dr < HD ? dr : 0) * NRP + 16 * s + 8 * g;
                if constexpr (sizeof(T) == 2) rf.set(dr < HD ? *reinterpret_cast<const uint4*>(rp) : zero4());
                else rf.set(dr < HD ? *reinterpret_cast<const uint4*>(rp) : zero4(), dr < HD ? *reinterpret_cast<const uint4*>(rp + 4) : zero4());
                mma(dq[db], rf, gf);
            }
        }
    }
    __syncthreads();      // every wave is done with its tables -> reuse the region as the dQ staging tile
    if (valid) {
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                const int d0 = db * 32 + 8 * rg + 4 * g;
                if (d0 < HD) {
                    T* dst = reinterpret_cast<T*>(wreg + (lane & 31) * ROWB) + d0;
                    *reinterpret_cast<typename TT<T>::Vec4*>(dst) =
                        cvt4(dq[db][rg * 4], dq[db][rg * 4 + 1], dq[db][rg * 4 + 2], dq[db][rg * 4 + 3], (T*)nullptr);
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
                const uint4 v = *reinterpret_cast<const uint4*>(wreg + row * ROWB + ch * 16);
                *reinterpret_cast<uint4*>(dqkv + ((size_t)b * L + qt * 32 + row) * ldq + h * HD + ch * TT<T>::EPC) = v;
            }
        }
    }
}

// ------------------------------------------------------------------------------- kernel B: dK, dV
#define ANYB_AUX_LD 36   // floats per LDS row of the transposed aux tile (32 + 4 pad: conflict-free 16-B reads)
#define ANYB_CAUX 4      // 16-B chunks of the aux tile per thread: (Hp + Wp + 2) * 8 <= ANYB_CAUX * 256
template <typename T, int NW, int HD>
__global__ __launch_bounds__(NW * 64) void attn_any_bwd_dkv_kernel(const T* __restrict__ qkv, size_t ldq, const T* __restrict__ dout,
                                                                   size_t lddo, const float* __restrict__ aux, T* __restrict__ dqkv, int L,
                                                                   int H, int Hp, int Wp, float scale) {
    typedef KvTile<T, HD> KV;
    constexpr int NT = NW * 64;
    constexpr int KB = KV::KB, VB = KV::VB, KS = KV::KS, DB = KV::DB;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 5;
    const int bh = blockIdx.y, b = bh / H, h = bh % H;
    const int D = H * HD, TA = Hp + Wp;
    const int AUXB = (TA + 2) * ANYB_AUX_LD * 4;
    const int STG = 2 * KB + 2 * VB + AUXB;    // Q row, dO row, Q^T, dO^T, aux
    const T* qbase = qkv + (size_t)b * L * ldq + h * HD;
    const T* dobase = dout + (size_t)b * L * lddo + h * HD;
    const int kt = blockIdx.x * NW + wave;
    const bool valid = kt * 32 < L;
    const int key = kt * 32 + (lane & 31);
    const bool klive = key < L;
    const int kc = klive ? key : L - 1;        // (a key >= L: table rows that exist; its P and dS are forced to 0)
    const int khl = kc / Wp, kwl = kc % Wp;

    Frag<T> kf[KS], vf[KS];
    if (valid) {
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            if (klive) {
                load_gfrag<T>(kf[s], qbase + D + (size_t)key * ldq, s, g);
                load_gfrag<T>(vf[s], qbase + 2 * D + (size_t)key * ldq, s, g);
            } else {
                zero_frag<T>(kf[s]);
                zero_frag<T>(vf[s]);
            }
        }
    }
    RowStageB<T, NT, HD> qs, dos;
    TrStageB<T, HD> qts, dots;
    const int NAUX = (TA + 2) * 8;                       // 16-B chunks of the aux tile
    uint4 ra[ANYB_CAUX];
    const int ntile = (L + 31) / 32;
    auto load_all = [&](int j) {
        const int nr = L - j * 32;
        qs.load(qbase + (size_t)j * 32 * ldq, ldq, tid, nr);
        qts.load(qbase + (size_t)j * 32 * ldq, ldq, tid, nr);
        dos.load(dobase + (size_t)j * 32 * lddo, lddo, tid, nr);
        dots.load(dobase + (size_t)j * 32 * lddo, lddo, tid, nr);
        const float* ax = aux + ((size_t)bh * ntile + j) * (TA + 2) * 32;
#pragma unroll
        for (int i = 0; i < ANYB_CAUX; ++i) {
            const int c = tid + NT * i;
            if (c < NAUX) ra[i] = *reinterpret_cast<const uint4*>(ax + (size_t)c * 4);
        }
    };
    auto store_all = [&](int stage) {
        unsigned char* s0 = smem + stage * STG;
        qs.store(s0, tid);
        dos.store(s0 + KB, tid);
        qts.store(s0 + 2 * KB, tid);
        dots.store(s0 + 2 * KB + VB, tid);
#pragma unroll
        for (int i = 0; i < ANYB_CAUX; ++i) {
            const int c = tid + NT * i;
            if (c < NAUX) *reinterpret_cast<uint4*>(s0 + 2 * KB + 2 * VB + (c >> 3) * (ANYB_AUX_LD * 4) + (c & 7) * 16) = ra[i];
        }
    };
    for (int stage = 0; stage < 2; ++stage) {
        KV::zero_pad(smem + stage * STG + 2 * KB, tid, NT);
        KV::zero_pad(smem + stage * STG + 2 * KB + VB, tid, NT);
    }
    load_all(0);
    store_all(0);
    __syncthreads();

    f32x16 dk[DB], dv[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dk[db][r] = 0.f; dv[db][r] = 0.f; }
    const float sl = scale * LOG2E_F;

    for (int j = 0; j < ntile; ++j) {
        if (j + 1 < ntile) load_all(j + 1);
        const unsigned char* st = smem + (j & 1) * STG;
        if (valid) {
            f32x16 sacc, dpacc;
#pragma unroll
            for (int r = 0; r < 16; ++r) { sacc[r] = 0.f; dpacc[r] = 0.f; }
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                Frag<T> qf, dof;
                load_rowfrag<T, HD>(qf, st, lane & 31, s, g);
                load_rowfrag<T, HD>(dof, st + KB, lane & 31, s, g);
                mma(sacc, qf, kf[s]);          // S[q][key]: lane = key, regs = q rows
                mma(dpacc, dof, vf[s]);        // dP[q][key]
            }
            const float* ax = reinterpret_cast<const float*>(st + 2 * KB + 2 * VB);
            const int nq = klive ? L - j * 32 : 0;      // query rows of this tile that exist for this key (a key >= L: none)
            float p[16], ds[16];
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                const int q0 = 8 * rg + 4 * g;
                const float4 bh4 = *reinterpret_cast<const float4*>(ax + khl * ANYB_AUX_LD + q0);
                const float4 bw4 = *reinterpret_cast<const float4*>(ax + (Hp + kwl) * ANYB_AUX_LD + q0);
                const float4 ls4 = *reinterpret_cast<const float4*>(ax + TA * ANYB_AUX_LD + q0);
                const float4 dl4 = *reinterpret_cast<const float4*>(ax + (TA + 1) * ANYB_AUX_LD + q0);
                const float bs[4] = {bh4.x + bw4.x, bh4.y + bw4.y, bh4.z + bw4.z, bh4.w + bw4.w};
                const float ls[4] = {ls4.x, ls4.y, ls4.z, ls4.w}, dl[4] = {dl4.x, dl4.y, dl4.z, dl4.w};
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int r = rg * 4 + t;
                    const bool live = q0 + t < nq;      // rows >= L contribute nothing: P and dS forced to 0, not computed
                    const float pv = __builtin_amdgcn_exp2f(fmaf(sacc[r], sl, bs[t]) - ls[t]);
                    p[r] = live ? pv : 0.f;
                    ds[r] = live ? pv * (dpacc[r] - dl[t]) : 0.f;
                }
            }
            Frag<T> pf[2], dsf[2];
            pack_frag<T>(pf[0], p);
            pack_frag<T>(pf[1], p + 8);
            pack_frag<T>(dsf[0], ds);
            pack_frag<T>(dsf[1], ds + 8);
#pragma unroll
            for (int db = 0; db < DB; ++db)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    Frag<T> qtf, dotf;
                    load_trfrag<T, HD>(dotf, st + 2 * KB + VB, db * 32 + (lane & 31), s, g);
                    load_trfrag<T, HD>(qtf, st + 2 * KB, db * 32 + (lane & 31), s, g);
                    mma(dv[db], dotf, pf[s]);      // dV^T[d][key] += dO^T[d][q] P[q][key]
                    mma(dk[db], qtf, dsf[s]);      // dK^T[d][key] += Q^T[d][q] dS[q][key]
                }
        }
        if (j + 1 < ntile) store_all((j + 1) & 1);
        __syncthreads();
    }

    // store dK (x scale) and dV rows through a per-wave LDS staging tile; no row >= L is stored
    constexpr int ROWB = HD * sizeof(T);
    unsigned char* stg = smem + (size_t)wave * 2 * 32 * ROWB;
    if (valid) {
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                const int d0 = db * 32 + 8 * rg + 4 * g;
                if (d0 >= HD) continue;
                T* dstk = reinterpret_cast<T*>(stg + (lane & 31) * ROWB) + d0;
                T* dstv = reinterpret_cast<T*>(stg + 32 * ROWB + (lane & 31) * ROWB) + d0;
                *reinterpret_cast<typename TT<T>::Vec4*>(dstk) = cvt4(dk[db][rg * 4] * scale, dk[db][rg * 4 + 1] * scale,
                                                                    dk[db][rg * 4 + 2] * scale, dk[db][rg * 4 + 3] * scale, (T*)nullptr);
                *reinterpret_cast<typename TT<T>::Vec4*>(dstv) =
                    cvt4(dv[db][rg * 4], dv[db][rg * 4 + 1], dv[db][rg * 4 + 2], dv[db][rg * 4 + 3], (T*)nullptr);
            }
    }
    __syncthreads();
    if (valid) {
        constexpr int CPR = ROWB / 16;
#pragma unroll
        for (int i = 0; i < 32 * CPR / 64; ++i) {
            const int c = lane + 64 * i, row = c / CPR, ch = c % CPR;
            if (kt * 32 + row < L) {
                T* orow = dqkv + ((size_t)b * L + kt * 32 + row) * ldq + h * HD + ch * TT<T>::EPC;
                *reinterpret_cast<uint4*>(orow + D) = *reinterpret_cast<const uint4*>(stg + row * ROWB + ch * 16);
                *reinterpret_cast<uint4*>(orow + 2 * D) = *reinterpret_cast<const uint4*>(stg + 32 * ROWB + row * ROWB + ch * 16);
            }
        }
    }
}

// ------------------------------------------------------------------------------- host side
#define ANYB_LDS (160 * 1024)
template <typename T, int HD> static int64_t anyb_dq_smem(int Hp, int Wp, int nw, int* tab_stride) {
    typedef KvTile<T, HD> KV;
    int64_t ts = (int64_t)32 * (anyb_ts(Hp, Wp) + anyb_tg(Hp, Wp)) * 4;
    const int64_t stg = 32 * HD * (int64_t)sizeof(T);
    if (ts < stg) ts = stg;
    ts = (ts + 15) / 16 * 16;
    if (ts > ANYB_LDS) return -1;
    *tab_stride = (int)ts;
    return 2 * (int64_t)(2 * KV::KB + KV::VB) + nw * ts;
}
// waves per workgroup of kernel A: the most whose tables fit the LDS beside the staging images (TrStage needs 2 * HD threads); 0: none
template <typename T, int HD> static int anyb_dq_waves(int Hp, int Wp) {
    int ts;
    for (int nw = 4; nw >= (HD == 64 ? 2 : 3); --nw) {
        const int64_t s = anyb_dq_smem<T, HD>(Hp, Wp, nw, &ts);
        if (s > 0 && s <= ANYB_LDS) return nw;
    }
    return 0;
}
template <typename T, int HD> static int64_t anyb_dkv_smem(int Hp, int Wp) {
    typedef KvTile<T, HD> KV;
    const int64_t auxb = (int64_t)(Hp + Wp + 2) * ANYB_AUX_LD * 4;
    int64_t smem = 2 * (2 * KV::KB + 2 * KV::VB + auxb);
    const int64_t stg = (int64_t)4 * 2 * 32 * HD * sizeof(T);
    return smem < stg ? stg : smem;
}
template <typename T, int HD> static bool anyb_fits(int Hp, int Wp) {
    return (int64_t)(Hp + Wp + 2) * 8 <= ANYB_CAUX * 256 && anyb_dkv_smem<T, HD>(Hp, Wp) <= ANYB_LDS && anyb_dq_waves<T, HD>(Hp, Wp) > 0;
}
static bool anyb_fits_any(int dtype, int Hp, int Wp, int hd) {
    if (dtype == PA_BF16) return hd == 80 ? anyb_fits<bf16, 80>(Hp, Wp) : anyb_fits<bf16, 64>(Hp, Wp);
    return hd == 80 ? anyb_fits<float, 80>(Hp, Wp) : anyb_fits<float, 64>(Hp, Wp);
}
static bool anyb_shape_ok(int dtype, int batch, int L, int heads, int Hp, int Wp, int hd) {
    if (dtype != PA_BF16 && dtype != PA_F32) return false;
    if (batch < 1 || heads < 1 || Hp < 1 || Wp < 1 || (int64_t)Hp * Wp != L || L > (1 << 24)) return false;
    if (hd != 64 && hd != 80) return false;
    if ((int64_t)batch * heads > 65535 || (int64_t)batch * L > INT32_MAX) return false;
    if (hd != 64 && heads * hd > 2048) return false;                  // pa_attn_bwd_delta's bound
    return anyb_fits_any(dtype, Hp, Wp, hd);
}

// workspace sections: Delta | aux | dG | slabs of the table contraction
struct AnybWs { int64_t delta, aux, dg, slabs, total; };
static AnybWs anyb_ws(int dtype, int batch, int L, int heads, int Hp, int Wp, int hd) {
    const int64_t es = dtype == PA_BF16 ? 2 : 4, NRP = pa_relpos_rows_padded(Hp, Wp), ntile = (L + 31) / 32;
    AnybWs w;
    w.delta = 0;
    w.aux = w.delta + up256((int64_t)batch * heads * L * 4);
    w.dg = w.aux + up256((int64_t)batch * heads * ntile * (Hp + Wp + 2) * 32 * 4);
    w.slabs = w.dg + up256((int64_t)batch * L * heads * NRP * es);
    w.total = w.slabs + up256(pa_attn_bwd_relpos_workspace_bytes(dtype, batch, L, heads, Hp, Wp, hd));
    return w;
}
extern "C" int64_t pa_attn_any_bwd_workspace_bytes(int dtype, int batch, int L, int heads, int Hp, int Wp, int head_dim) {
    if (!anyb_shape_ok(dtype, batch, L, heads, Hp, Wp, head_dim)) return 0;
    return anyb_ws(dtype, batch, L, heads, Hp, Wp, head_dim).total;
}

template <typename T, int NW, int HD>
static int anyb_dq_launch(const T* qkv, int64_t ldq, const T* rcat, const T* rcatT, const T* dout, int64_t lddo, const float* lse,
                          const float* delta, T* dqkv, T* dG, float* aux, int Bn, int L, int H, int Hp, int Wp, float scale, hipStream_t st) {
    const int NRP = pa_relpos_rows_padded(Hp, Wp);
    int ts = 0;
    const int64_t smem = anyb_dq_smem<T, HD>(Hp, Wp, NW, &ts);
    auto kern = attn_any_bwd_dq_kernel<T, NW, HD>;
    static bool done = false;
    if (!done) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, ANYB_LDS);
        if (e != hipSuccess) return (int)e;
        done = true;
    }
    const int qtiles = (L + 31) / 32;
    PA_LAUNCH(kern, dim3((qtiles + NW - 1) / NW, Bn * H), dim3(NW * 64), (size_t)smem, st, qkv, (size_t)ldq, rcat, rcatT, dout, (size_t)lddo,
              lse, delta, dqkv, dG, aux, L, H, Hp, Wp, NRP, scale, ts, anyb_ts(Hp, Wp), anyb_tg(Hp, Wp));
    return (int)hipGetLastError();
}
template <typename T, int HD>
static int anyb_t(const T* qkv, int64_t ldq, const T* rcat, const T* rcatT, const T* dout, int64_t lddo, const float* lse,
                  const float* delta, T* dqkv, T* dG, float* aux, int Bn, int L, int H, int Hp, int Wp, float scale, hipStream_t st) {
    const int nw = anyb_dq_waves<T, HD>(Hp, Wp);
    int e = (int)hipErrorInvalidValue;
#define ANYB_DQ(NW_) anyb_dq_launch<T, NW_, HD>(qkv, ldq, rcat, rcatT, dout, lddo, lse, delta, dqkv, dG, aux, Bn, L, H, Hp, Wp, scale, st)
    if (nw == 4) e = ANYB_DQ(4);
    else if (nw == 3) e = ANYB_DQ(3);
    else if constexpr (HD == 64) { if (nw == 2) e = ANYB_DQ(2); }
#undef ANYB_DQ
    if (e) return e;
    constexpr int NW = 4;
    auto kern = attn_any_bwd_dkv_kernel<T, NW, HD>;
    static bool done = false;
    if (!done) {
        hipError_t er = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, ANYB_LDS);
        if (er != hipSuccess) return (int)er;
        done = true;
    }
    const int ktiles = (L + 31) / 32;
    const size_t smem = (size_t)anyb_dkv_smem<T, HD>(Hp, Wp);
    PA_LAUNCH(kern, dim3((ktiles + NW - 1) / NW, Bn * H), dim3(NW * 64), smem, st, qkv, (size_t)ldq, dout, (size_t)lddo, aux, dqkv, L, H, Hp, Wp,
              scale);
    return (int)hipGetLastError();
}

static long long g_attn_any_bwd_launches = 0;
extern "C" int64_t pa_attn_any_bwd_launches(void) { return g_attn_any_bwd_launches; }

extern "C" int pa_attn_any_bwd(int dtype, const void* qkv, int64_t ldq, const void* rcat, const void* rcatT, const void* out, int64_t ldo,
                               const void* dout, int64_t lddo, const float* lse, void* dqkv, float* drcat, void* workspace, int batch, int L,
                               int heads, int Hp, int Wp, int head_dim, float scale, hipStream_t st) {
    if (qkv == nullptr || rcat == nullptr || rcatT == nullptr || out == nullptr || dout == nullptr || lse == nullptr || dqkv == nullptr ||
        workspace == nullptr)
        return (int)hipErrorInvalidValue;
    if (!anyb_shape_ok(dtype, batch, L, heads, Hp, Wp, head_dim)) return (int)hipErrorInvalidValue;
    const int es = dtype == PA_BF16 ? 2 : 4;
    // 16-byte vector loads and stores of whole head rows
    const int64_t D = (int64_t)heads * head_dim;
    if (ldq < 3 * D || ldo < D || lddo < D || ldq * es % 16 || ldo * es % 16 || lddo * es % 16) return (int)hipErrorInvalidValue;
    if ((uintptr_t)qkv % 16 || (uintptr_t)rcat % 16 || (uintptr_t)rcatT % 16 || (uintptr_t)out % 16 || (uintptr_t)dout % 16 ||
        (uintptr_t)dqkv % 16 || (uintptr_t)workspace % 16 || (uintptr_t)lse % 4 || (uintptr_t)drcat % 16)
        return (int)hipErrorInvalidValue;
    ++g_attn_any_bwd_launches;
    const AnybWs w = anyb_ws(dtype, batch, L, heads, Hp, Wp, head_dim);
    unsigned char* ws = (unsigned char*)workspace;
    float* delta = (float*)(ws + w.delta);
    float* aux = (float*)(ws + w.aux);
    void* dG = ws + w.dg;
    PA_TRY(pa_attn_bwd_delta(dtype, out, ldo, dout, lddo, delta, batch, L, heads, head_dim, st));
#define ANYB(TT_, HD_) anyb_t<TT_, HD_>((const TT_*)qkv, ldq, (const TT_*)rcat, (const TT_*)rcatT, (const TT_*)dout, lddo, lse, delta, \
                                        (TT_*)dqkv, (TT_*)dG, aux, batch, L, heads, Hp, Wp, scale, st)
    if (dtype == PA_BF16) PA_TRY(head_dim == 80 ? ANYB(bf16, 80) : ANYB(bf16, 64));
    else PA_TRY(head_dim == 80 ? ANYB(float, 80) : ANYB(float, 64));
#undef ANYB
    if (drcat == nullptr) return 0;
    // d[rel_pos_h ; rel_pos_w ; 0] = sum over heads, samples, queries of dG[., r] * q[., d]: the contraction of pa_attn_bwd_relpos, whose
    // K tiles are bounded by batch * L whatever it is a multiple of; slabs summed in a fixed order
    return pa_attn_bwd_relpos(dtype, dG, qkv, ldq, drcat, ws + w.slabs, batch, L, heads, Hp, Wp, head_dim, st);
}

// ------------------------------------------------------------------------------------------------ adjoint of the rel-pos table resize
__global__ void relpos_resize_bwd_kernel(const float* __restrict__ drcat, float* __restrict__ dtab, int out_rows, int sh, int sw, int dh,
                                         int dw, int hd) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= out_rows * hd) return;
    const int r = e / hd, d = e % hd;
    float acc = 0.f;
    if (r < sh + sw) {
        const bool is_w = r >= sh;
        const int i = is_w ? r - sh : r, nin = is_w ? sw : sh, nout = is_w ? dw : dh;
        const float* g = drcat + (size_t)(is_w ? dh : 0) * hd + d;
        if (nin == nout) {
            acc = g[(size_t)i * hd];
        } else {
            for (int j = 0; j < nout; ++j) {            // exactly relpos_resize_kernel's i0, i1, l1 per j
                const float s = fmaxf((float)nin / (float)nout * ((float)j + 0.5f) - 0.5f, 0.f);
                int i0 = (int)s;
                if (i0 > nin - 1) i0 = nin - 1;
                const int i1 = i0 < nin - 1 ? i0 + 1 : i0;
                const float l1 = fminf(fmaxf(s - (float)i0, 0.f), 1.f);
                const float gj = g[(size_t)j * hd];
                if (i0 == i) acc += (1.f - l1) * gj;
                if (i1 == i) acc += l1 * gj;
            }
        }
    }
    dtab[e] = acc;
}
extern "C" int pa_relpos_resize_bwd(const float* drcat, float* dtab, int out_rows, int src_h, int src_w, int dst_h, int dst_w, int head_dim,
                                    hipStream_t st) {
    if (drcat == nullptr || dtab == nullptr || head_dim < 1 || src_h < 1 || src_w < 1 || dst_h < 1 || dst_w < 1) return (int)hipErrorInvalidValue;
    if ((int64_t)src_h + src_w > out_rows || (int64_t)out_rows * head_dim > (1 << 30) || ((int64_t)dst_h + dst_w) * head_dim > (1 << 30))
        return (int)hipErrorInvalidValue;
    const int n = out_rows * head_dim;
    PA_LAUNCH(relpos_resize_bwd_kernel, dim3((n + 255) / 256), dim3(256), 0, st, drcat, dtab, out_rows, src_h, src_w, dst_h, dst_w, head_dim);
    LAUNCH_CHECK();
}
