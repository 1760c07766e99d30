// Quantised coefficients -> libjpeg's decoded pixels on gfx950: the reconstruction half of a
// baseline 4:2:0 decode (jpeg_recon.hip), shared by the decoder (jpeg_decode.hip: coefficients from
// a file's scan) and the encoder (jpeg.hip: the coefficients it has just quantised).
//
// What differs between the callers is in ReconImage: where the image's quantisers are (one set of
// 192 uint16 per file for the decoder, one shared set per call for the encoder) and where its
// pixels go (a slot of a strided atlas, or a tightly packed face).  Coefficients: int16
// [mcu][6][64], zigzag order, the MCUs of image f at [mcu0[f], mcu0[f + 1]).
#pragma once
#include <cstdint>

#include "common.hpp"

namespace vtf {

// one image of a call
struct ReconImage {
    int32_t h, w;
    int32_t mw;       // MCUs per row
    int32_t quant;    // its quantisers: quant[q * 192 ...) = Y, Cb, Cr tables of 64, zigzag order
    int64_t out;      // byte offset of its pixel (0, 0) in the output
    int64_t rstride;  // bytes from one of its rows to the next
};

// index of the part that owns element i of a partition given by its ascending bounds[0..N]
__device__ inline int owner(const int32_t* __restrict__ bounds, int N, int i) {
    int lo = 0, hi = N;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (bounds[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// k_jpeg_idct and k_jpeg_pixels on st: every image with status jpg::ST_OK gets its pixels; one
// whose values leave int16 (no 8-bit image's do) is marked jpg::ST_CORRUPT instead.  yplane /
// cplane: scratch of mcus * 256 and mcus * 128 bytes.
void launch_recon(const ReconImage* images, const int32_t* mcu0, int M, int64_t mcus, const uint16_t* quant,
                  const int16_t* coef, int32_t* status, uint8_t* yplane, uint8_t* cplane, uint8_t* out,
                  hipStream_t st);

}  // namespace vtf
