// What the two translation units of the device JPEG decoder share: jpeg_decode.hip (host side of
// a call, the serial stage 1, stage 2) and jpeg_decode_split.hip (the split-scan stage 1).
#pragma once

#include "common.hpp"
#include "jpeg_entropy.hpp"

namespace vtf {

// one decodable file of a call
struct DecFile {
    int64_t scan_begin, scan_end;  // in the uploaded bytes
    int32_t h, w;
    int32_t mw;    // MCUs per row
    int32_t set;   // index of its HuffSet
    int32_t slot;  // its index among the call's N files
    int32_t pad;
};

// The body of vtf_jpeg_decode (seg_bytes < 0: stage 1 is k_jpeg_entropy) and of
// vtf_jpeg_decode_split (seg_bytes > 0: stage 1 is launch_entropy_split).  Throws vtf::Error.
void jpeg_decode_call(const uint8_t* data, const int64_t* offsets, int64_t N, uint8_t* d_bgr, int Hmax, int Wmax,
                      int64_t frame_stride, int64_t row_stride, int32_t* out_sizes, int32_t* out_status, int seg_bytes,
                      hipStream_t st);

// Stage 1 by split scans, on st: the M files' coefficients into coef (zeroed) and their statuses.
// h_files / d_files: the same table on the host and on the device.  Uses ar's slots 6 to 10 and
// mailbox 1.
void launch_entropy_split(Arena& ar, const uint8_t* d_data, int64_t nbytes, const DecFile* h_files,
                          const DecFile* d_files, const int32_t* d_mcu0, int M, const jpg::HuffSet* d_sets,
                          int16_t* coef, int32_t* d_status, int seg_bytes, hipStream_t st);

}  // namespace vtf
