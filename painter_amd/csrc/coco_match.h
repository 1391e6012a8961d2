// What COCOeval.evaluateImg does the same way for every iouType, stated once for painter_ap.hip (mask IoU) and painter_kpt.hip (OKS): the
// threshold cap, the stable rank by score, the ignored ground truths of an area range and the greedy walk of ONE detection over the ground
// truths.  Ground truths are bits of two 64-bit words (at most 128 per picture).  What differs between the two scorers stays in their
// kernels: where a detection's row of IoU / OKS doubles and its area come from, which LDS words take a record's bits, the class table.
#pragma once
#include "common.h"

namespace coco {

DEVI bool bit_of(u64 w0, u64 w1, int g) { return (((g < 64 ? w0 : w1) >> (g & 63)) & 1ull) != 0ull; }

// evaluateImg's `iou = min([t, 1 - 1e-10])`
DEVI double cap_threshold(double thr) {
    const double cap = 1 - 1e-10;
    return thr < cap ? thr : cap;
}

// Stable rank of entry `me` among scores[0 .. n) by descending score (O(n) counting per entry): equal scores to the lower index, or with
// `ties_to_higher` to the higher one.
DEVI int rank_by_score(const float* scores, int n, int me, bool ties_to_higher) {
    const float s = scores[me];
    int rank = 0;
    for (int o = 0; o < n; ++o) {
        const float so = scores[o];
        rank += (so > s || (so == s && (ties_to_higher ? o > me : o < me))) ? 1 : 0;
    }
    return rank;
}

// The ignored ground truths of the area range [lo, hi]: those of the starting words (crowd; for keypoints also the unlabelled) and those
// whose area lies outside.
DEVI void ignore_words(const double* garea, int G, double lo, double hi, u64 start0, u64 start1, u64* out) {
    u64 b[2] = {start0, start1};
    for (int g = 0; g < G; ++g)
        if (garea[g] < lo || garea[g] > hi) b[g >> 6] |= 1ull << (g & 63);
    out[0] = b[0];
    out[1] = b[1];
}

// The walk of one detection at one (range, threshold): row[g] = its IoU / OKS with ground truth g, thr0 the capped threshold, ign / crowd /
// taken the ignored, crowd and already matched ground truths, skip(g) true for one that is not a candidate at all (another class).
// evaluateImg's "ignored ones last, stop at the first ignored one once a non-ignored one is held" is ONE pass in table order with two
// running bests (non-ignored, ignored; >= keeps the later of equals, as the walk does), and the ignored best counts only when there is no
// other; the row is read four at a time.  -> the ground truth taken, now also in `taken`, or -1.
template <typename Skip>
DEVI int match_one(const double* __restrict__ row, int G, double thr0, u64 ign0, u64 ign1, u64 crowd0, u64 crowd1, u64& taken0, u64& taken1,
                   Skip skip) {
    const u64 free0 = ~taken0 | crowd0, free1 = ~taken1 | crowd1;          // a matched one stays open only when it is crowd
    double best = thr0, best_ign = thr0;                  // of the non-ignored and of the ignored ground truths
    int m = -1, m_ign = -1;
    for (int g0 = 0; g0 < G; g0 += 4) {
        double v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = g0 + i < G ? row[g0 + i] : -INFINITY;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int g = g0 + i;
            if (v[i] < thr0) continue;
            if (!bit_of(free0, free1, g)) continue;
            if (skip(g)) continue;
            if (bit_of(ign0, ign1, g)) {
                if (v[i] >= best_ign) { best_ign = v[i]; m_ign = g; }
            } else if (v[i] >= best) {
                best = v[i];
                m = g;
            }
        }
    }
    if (m < 0) m = m_ign;
    if (m > -1) {
        if (m < 64) taken0 |= 1ull << m;
        else taken1 |= 1ull << (m - 64);
    }
    return m;
}

}  // namespace coco
