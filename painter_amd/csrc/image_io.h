// Pixel helpers shared by the inference pre-/post-processing files (seggpt_io.hip, painter_io.hip): the ImageNet constants, the
// (v / div - mean) / std normalisation and the unpatchify index math of the lower half of the stitched canvas.  Both files are built
// with -ffp-contract=off (build.py) and carry `#pragma clang fp contract(off)`: every operation below rounds once, in the
// reference's order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"

#pragma clang fp contract(off)

namespace {

__device__ __constant__ double kMean[3] = {0.485, 0.456, 0.406};      // seggpt_engine.py:9, painter_inference_*.py imagenet_mean
__device__ __constant__ double kStd[3] = {0.229, 0.224, 0.225};       // seggpt_engine.py:10, painter_inference_*.py imagenet_std

// (v / div - mean) / std, one rounding per operation, then narrowed to float32 (numpy float64 -> torch .float()).
DEVI float normalise(uint8_t u, double div, int c) {
    double v = (double)u / div;
    v = v - kMean[c];
    v = v / kStd[c];
    return (float)v;
}

// Element (r, x, c) of the LOWER res_h x res_w half of unpatchify(pred) (models_seggpt.py:376-389, models_painter.py unpatchify), then
// v * std + mean in float64.  pred = one sample's tokens [2*res_h/P * wp][P*P*3].
DEVI double denormalised(const float* __restrict__ pred, int r, int x, int c, int res_h, int wp, int P) {
    const int row = res_h + r;
    const int token = (row / P) * wp + x / P;
    const int within = ((row % P) * P + x % P) * 3 + c;
    double o = (double)pred[(size_t)token * (P * P * 3) + within];
    o = o * kStd[c];
    o = o + kMean[c];
    return o;
}

// clip(denormalised * scale, 0, scale): torch.clip = max with 0, then min with scale (NaN propagates through both selects).
DEVI double decoded_scaled(const float* __restrict__ pred, int r, int x, int c, int res_h, int wp, int P, double scale) {
    double o = denormalised(pred, r, x, c, res_h, wp, P);
    o = o * scale;
    o = o < 0.0 ? 0.0 : o;
    o = o > scale ? scale : o;
    return o;
}

}  // namespace
