// Shared by the post-processing files that compare painted pixels with palette colours.
//   Byte packing (painter_inst.hip, painter_pano.hip): R | G << 8 | B << 16 in one dword, so that the L1 distance of a pixel and a
//   colour is ONE v_sad_u8.  Integer only.
//   nearest_colour (painter_io.hip: pa_palette_argmin; painter_score.hip: pa_semseg_confusion): the evaluators' float32 colour -> class
//   decode, one statement of its operation order for every kernel that needs a pixel's class.
#pragma once
#include "common.h"

namespace {

DEVI uint32_t pack_colour(const float* __restrict__ pal, int c) {
    return ((uint32_t)(int)pal[3 * c] & 255u) | (((uint32_t)(int)pal[3 * c + 1] & 255u) << 8) | (((uint32_t)(int)pal[3 * c + 2] & 255u) << 16);
}
DEVI uint32_t pack_pixel(const uint8_t* __restrict__ pic, int64_t p) {
    return (uint32_t)pic[3 * p] | ((uint32_t)pic[3 * p + 1] << 8) | ((uint32_t)pic[3 * p + 2] << 16);
}

// ADE20kSemSegEvaluatorCustom.py:124-138.  DIST: 0 abs, 1 square, 2 (abs + square) / 2 per channel, summed over the channels in float32
// ((c0 + c1) + c2, no fused multiply-add: the files that include this are built with -ffp-contract=off); strict < keeps the first
// minimum.  pal: K colours of 3 floats, in LDS where every lane reads the same colour (a broadcast, no bank conflict).
template <int DIST> DEVI float channel_dist(float d) {
    if constexpr (DIST == 0) return fabsf(d);
    else if constexpr (DIST == 1) return d * d;
    else return (fabsf(d) + d * d) / 2.f;
}
template <int DIST> DEVI int nearest_colour(float p0, float p1, float p2, const float* pal, int K) {
    float best = 0.f;
    int arg = 0;
    for (int k = 0; k < K; ++k) {
        float e = channel_dist<DIST>(p0 - pal[3 * k]) + channel_dist<DIST>(p1 - pal[3 * k + 1]);
        e = e + channel_dist<DIST>(p2 - pal[3 * k + 2]);
        if (k == 0 || e < best) {
            best = e;
            arg = k;
        }
    }
    return arg;
}

}  // namespace
