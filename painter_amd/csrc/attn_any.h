// Staging with a row bound, shared by the any-grid attention kernels (attn_any.hip, attn_any_bwd.hip).
#pragma once
#include "attn_common.h"

// RowStage / TrStage with a row bound: rows >= nrows of the 32-row tile are zeros
template <typename T, int NT, int HD> struct RowStageB : RowStage<T, NT, HD> {
    typedef RowStage<T, NT, HD> S;
    DEVI void load(const T* src, size_t ld, int tid, int nrows) {
#pragma unroll
        for (int i = 0; i < S::CK; ++i) {
            const int c = tid + NT * i;
            if (c < S::NCH) {
                const int row = c / S::SL;
                this->r[i] = row < nrows ? *reinterpret_cast<const uint4*>(src + (size_t)row * ld + (c % S::SL) * TT<T>::EPC) : zero4();
            }
        }
    }
};
template <typename T, int HD> struct TrStageB : TrStage<T, HD> {
    typedef TrStage<T, HD> S;
    DEVI void load(const T* src, size_t ld, int tid, int nrows) {
        if (tid < 8 * S::CBN) {
            const int cb = tid % S::CBN, rb = tid / S::CBN;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = rb * 4 + i;
                if (row < nrows) this->r[i] = *reinterpret_cast<const typename S::Vec4*>(src + (size_t)row * ld + cb * 4);
                else zero_vec(this->r[i]);
            }
        }
    }
};
