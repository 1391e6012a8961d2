// Byte packing shared by the post-processing files that compare painted pixels with palette colours (painter_inst.hip,
// painter_pano.hip): R | G << 8 | B << 16 in one dword, so that the L1 distance of a pixel and a colour is ONE v_sad_u8.  Integer only.
#pragma once
#include "common.h"

namespace {

DEVI uint32_t pack_colour(const float* __restrict__ pal, int c) {
    return ((uint32_t)(int)pal[3 * c] & 255u) | (((uint32_t)(int)pal[3 * c + 1] & 255u) << 8) | (((uint32_t)(int)pal[3 * c + 2] & 255u) << 16);
}
DEVI uint32_t pack_pixel(const uint8_t* __restrict__ pic, int64_t p) {
    return (uint32_t)pic[3 * p] | ((uint32_t)pic[3 * p + 1] << 8) | ((uint32_t)pic[3 * p + 2] << 16);
}

}  // namespace
