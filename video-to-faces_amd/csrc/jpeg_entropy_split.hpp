// Split-scan entropy decoding of the device JPEG decoder as shared host / device code:
// k_jpeg_entropy_split (jpeg_decode_split.hip) decodes one scan with many lanes, and
// split_decode_host() below runs the same passes over an array of "lanes" on the CPU
// (tests/host/jpeg_split_check.cpp, under ASan + UBSan, against entropy_decode).
//
// A baseline Huffman scan self-synchronises (Klein & Wiseman; Weissenberger & Schmidt, "Accelerating
// JPEG Decompression on GPUs"): apart from the DC predictors, the decoder's state at a bit position
// is (block in the MCU 0..5, zigzag index 0..63, 0 = a DC symbol is next), and a decoder started in
// the wrong state falls into step with the right one after a few symbols.  Per file:
//   a. unstuff    the scan bytes without the 00 after every FF: bit positions index a plain stream;
//   b. cut        segments of seg_bytes;
//   c. speculate  lane i decodes segment i from (first bit, block 0, index 0) and records its exit
//                 state (the first symbol boundary at or past the segment's end) and how many blocks
//                 it completed; segment 0 starts in the true state;
//   d. sync       entry(i) = exit(i - 1); a lane whose entry changed decodes again; until no entry
//                 changes.  The accepted result is the fixed point; lane r is right after round r,
//                 so fewer than nseg rounds are ever needed, and the loop enforces that;
//   e. count      exclusive scan of the blocks completed = every segment's first block;
//   f. write      every lane decodes once more from its verified entry and stores coefficients; the
//                 DC slot gets the DC difference.  Errors count only here;
//   g. DC         per component, the inclusive wrapping 32-bit prefix sum of the differences in block
//                 order, stored as (int16_t): what entropy_decode's running predictors give.
// Memory safety on arbitrary bytes: the reader loads stream[i] only for 0 <= i < nbytes and feeds
// zero bits past the end; a symbol consumes at least one bit, so a lane's loop ends at its segment's
// end; every store is checked against the file's mcus * 384 coefficients.
#pragma once

#include <vector>

#include "jpeg_entropy.hpp"

namespace vtf {
namespace jpg {

constexpr int SPLIT_SEG_DEFAULT = 128;  // bytes per segment when the caller passes 0
constexpr int SPLIT_SEG_MIN = 4, SPLIT_SEG_MAX = 4096;

// A decoder state in one word, so that a lane publishes it with one store: bits 0..5 zigzag index,
// 6..8 block in the MCU, 9.. bit position in the unstuffed stream.
constexpr uint64_t SPLIT_UNKNOWN = 1ull << 62;  // exit state of a lane that met an invalid code
constexpr uint64_t SPLIT_DIRTY = 1ull << 63;    // on an entry: changed this round, decode again

VTF_HD inline uint64_t split_pack(int64_t pos, int b, int k) {
    return ((uint64_t)pos << 9) | ((uint64_t)b << 6) | (uint64_t)k;
}

// Bit reader over the unstuffed stream.  It is a BitReader as far as huff_symbol() and
// receive_extend() are concerned (they use acc / n only); filling is by 32-bit words.
struct SplitReader : BitReader {
    const uint8_t* s;
    int64_t nbytes, next;  // next: the first byte not yet in the accumulator

    VTF_HD void open(const uint8_t* stream, int64_t len, int64_t bitpos) {
        s = stream, nbytes = len, next = bitpos >> 3;
        data = nullptr, pos = 0, end = 0, cache = 0, cn = 0, pad = 0;
        acc = 0, n = 0;
        more();
        n -= (int)(bitpos & 7);
    }
    // at least 32 valid bits afterwards
    VTF_HD void more() {
        if (n > 32) return;
        uint32_t w = 0;
        if (next + 4 <= nbytes) {
            uint8_t b[4];
            __builtin_memcpy(b, s + next, 4);
            w = ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3];
        } else {
            for (int i = 0; i < 4; i++) w = (w << 8) | (next + i < nbytes ? s[next + i] : 0u);
        }
        acc = (acc << 32) | w;
        n += 32, next += 4;
    }
    VTF_HD int64_t bitpos() const { return next * 8 - n; }
};

// What one lane needs to decode a segment of one file
struct SplitFile {
    const uint8_t* stream;  // unstuffed scan
    int64_t nbytes;
    const HuffSet* hs;
    int64_t blocks;  // mcus * 6
    int16_t* coef;   // [blocks][64], zeroed (WRITE only)
};

// Decodes from `entry` until the bit position reaches seg_end (a symbol boundary at or past it).
// -> exit state (SPLIT_UNKNOWN after an invalid symbol), blocks completed in *done.  WRITE: stores
// the coefficients of blocks first_block..., stops at the file's last block, and returns true on
// an error of the file (an invalid symbol or a consumed padding bit before the last block's end).
template <bool WRITE>
VTF_HD inline bool split_decode_segment(const SplitFile& F, uint64_t entry, int64_t seg_end, int64_t first_block,
                                        uint64_t* exit_state, int32_t* done) {
    int k = (int)(entry & 63), b = (int)((entry >> 6) & 7);
    if (b > 5) b = 0;
    SplitReader rd;
    rd.open(F.stream, F.nbytes, (int64_t)((entry & ~(SPLIT_DIRTY | SPLIT_UNKNOWN)) >> 9));
    int64_t blk = first_block;
    int32_t nd = 0;
    bool bad = false;
    while (rd.bitpos() < seg_end) {  // every round consumes at least one bit
        if (WRITE && blk >= F.blocks) break;  // bytes after the last block are ignored
        rd.more();
        const int c = b < 4 ? 0 : b - 3;
        if (k == 0) {
            const int s = huff_symbol(rd, &F.hs->dc[c]);
            if (s < 0 || s > 11) {
                bad = true;
                break;
            }
            const int diff = s ? receive_extend(rd, s) : 0;
            if (WRITE && blk * 64 < F.blocks * 64) F.coef[blk * 64] = (int16_t)diff;
            k = 1;
        } else {
            const int rs = huff_symbol(rd, &F.hs->ac[c]);
            if (rs < 0) {
                bad = true;
                break;
            }
            const int r = rs >> 4, s = rs & 15;
            if (s == 0) {
                k = r != 15 ? 64 : k + 16;  // EOB, ZRL
            } else {
                k += r;
                if (s > 10 || k > 63) {
                    bad = true;
                    break;
                }
                const int v = receive_extend(rd, s);
                if (WRITE && blk * 64 + k < F.blocks * 64) F.coef[blk * 64 + k] = (int16_t)v;
                k++;
            }
        }
        if (k >= 64) {  // the block is complete
            if (WRITE && rd.bitpos() > F.nbytes * 8) {  // it took padding bits
                bad = true;
                break;
            }
            k = 0, b = b == 5 ? 0 : b + 1;
            nd++, blk++;
        }
    }
    *done = nd;
    *exit_state = bad ? SPLIT_UNKNOWN : split_pack(rd.bitpos(), b, k);
    return bad;  // (WRITE: the lane stopped before the last block, so this is the file's error)
}

// the state a lane speculates from, and falls back to while its predecessor's exit is unknown
VTF_HD inline uint64_t split_spec_entry(int64_t seg, int seg_bytes) { return split_pack(seg * seg_bytes * 8, 0, 0); }
VTF_HD inline int64_t split_seg_end(const SplitFile& F, int64_t seg, int seg_bytes) {
    const int64_t e = (seg + 1) * seg_bytes;
    return (e < F.nbytes ? e : F.nbytes) * 8;
}

// pass c for lane i
VTF_HD inline void split_speculate(const SplitFile& F, int64_t i, int seg_bytes, uint64_t* entry, uint64_t* exits,
                                   int32_t* done) {
    entry[i] = split_spec_entry(i, seg_bytes);
    split_decode_segment<false>(F, entry[i], split_seg_end(F, i, seg_bytes), 0, &exits[i], &done[i]);
}
// pass d, first half for lane i >= 1: take the predecessor's exit as the entry (every lane does
// this before any lane decodes, so a round reads only the round before)
VTF_HD inline void split_sync_read(int64_t i, int seg_bytes, uint64_t* entry, const uint64_t* exits) {
    uint64_t e = exits[i - 1];
    if (e == SPLIT_UNKNOWN) e = split_spec_entry(i, seg_bytes);
    if (e != entry[i]) entry[i] = e | SPLIT_DIRTY;
}
// pass d, second half: decode again if the entry changed; -> whether it did
VTF_HD inline bool split_sync_decode(const SplitFile& F, int64_t i, int seg_bytes, uint64_t* entry, uint64_t* exits,
                                     int32_t* done) {
    if (!(entry[i] & SPLIT_DIRTY)) return false;
    entry[i] &= ~SPLIT_DIRTY;
    split_decode_segment<false>(F, entry[i], split_seg_end(F, i, seg_bytes), 0, &exits[i], &done[i]);
    return true;
}
// pass f for lane i; first[i] = the exclusive scan of done[].  -> the file is corrupt
VTF_HD inline bool split_write(const SplitFile& F, int64_t i, int seg_bytes, const uint64_t* entry,
                               const int32_t* first) {
    uint64_t ex;
    int32_t nd;
    return split_decode_segment<true>(F, entry[i], split_seg_end(F, i, seg_bytes), first[i], &ex, &nd);
}

// pass e adds block counts up to the file's blocks and no further (associative for counts >= 0;
// a + b cannot overflow: a <= cap < 2^25, b <= the bits of a segment)
VTF_HD inline int32_t split_sat_add(int32_t a, int32_t b, int32_t cap) { return a + b < cap ? a + b : cap; }

// is byte i of the scan data[begin, end) kept by pass a?  Dropped: the 00 after an FF, and an FF
// as the last byte (a marker's first half: the serial reader ends the scan there)
VTF_HD inline bool split_keeps(const uint8_t* data, int64_t begin, int64_t end, int64_t i) {
    const uint8_t v = data[i];
    if (v == 0x00) return !(i > begin && data[i - 1] == 0xFF);
    if (v == 0xFF) return i + 1 < end;
    return true;
}

// Passes a-g on the host, one lane after another: what the kernel computes.  coef = mcus * 384
// zeroed int16.  -> ST_OK / ST_CORRUPT; *rounds = sync rounds run (fewer than the segments).
inline int split_decode_host(const uint8_t* data, int64_t begin, int64_t end, const HuffSet* hs, int mcus,
                             int16_t* coef, int seg_bytes, int64_t* nseg_out, int64_t* rounds) {
    if (seg_bytes == 0) seg_bytes = SPLIT_SEG_DEFAULT;
    if (end < begin) end = begin;
    std::vector<uint8_t> stream;
    for (int64_t i = begin; i < end; i++)
        if (split_keeps(data, begin, end, i)) stream.push_back(data[i]);
    // an exact-size heap block: a read one byte past the stream is a sanitizer report
    std::vector<uint8_t> exact(stream);
    exact.shrink_to_fit();
    SplitFile F{exact.data(), (int64_t)exact.size(), hs, (int64_t)mcus * 6, coef};
    const int64_t nseg = (F.nbytes + seg_bytes - 1) / seg_bytes;
    std::vector<uint64_t> entry((size_t)nseg), exits((size_t)nseg);
    std::vector<int32_t> done((size_t)nseg);
    for (int64_t i = 0; i < nseg; i++) split_speculate(F, i, seg_bytes, entry.data(), exits.data(), done.data());
    int64_t r = 0;
    for (int64_t round = 1; round < nseg; round++) {
        r++;
        for (int64_t i = 1; i < nseg; i++) split_sync_read(i, seg_bytes, entry.data(), exits.data());
        bool changed = false;
        for (int64_t i = 1; i < nseg; i++)
            changed = split_sync_decode(F, i, seg_bytes, entry.data(), exits.data(), done.data()) || changed;
        if (!changed) break;
    }
    if (nseg_out) *nseg_out = nseg;
    if (rounds) *rounds = r;
    // (in place: done[] becomes first[]; the sums saturate at the file's blocks, where writing stops)
    int32_t total = 0;
    for (int64_t i = 0; i < nseg; i++) {
        const int32_t d = done[(size_t)i];
        done[(size_t)i] = total;
        total = split_sat_add(total, d, (int32_t)F.blocks);
    }
    bool bad = total < F.blocks;
    for (int64_t i = 0; i < nseg; i++) bad = split_write(F, i, seg_bytes, entry.data(), done.data()) || bad;
    if (bad) return ST_CORRUPT;
    uint32_t pred[3] = {0, 0, 0};
    for (int64_t j = 0; j < F.blocks; j++) {
        const int b = (int)(j % 6), c = b < 4 ? 0 : b - 3;
        pred[c] += (uint32_t)(int32_t)coef[j * 64];
        coef[j * 64] = (int16_t)pred[c];
    }
    return ST_OK;
}

}  // namespace jpg
}  // namespace vtf
