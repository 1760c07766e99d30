// The entropy decoder of the device JPEG decoder as shared host / device code: k_jpeg_entropy
// (jpeg_decode.hip) runs entropy_decode() on the GPU, tests/host/jpeg_decode_fuzz.cpp runs the same
// function on the CPU under ASan + UBSan.  No HIP header is needed on the host side.
//
// One interleaved 4:2:0 baseline scan -> quantised coefficients [mcus][6][64] int16 in zigzag order
// (Y00, Y01, Y10, Y11, Cb, Cr per MCU), jdhuff.c decode_mcu_slow's result.  Memory safety on
// arbitrary bytes:
//   - the bit reader reads data[pos] only for begin <= pos < end and feeds zero bits past the end
//     or past a marker; consuming one of those bits makes the file corrupt;
//   - the coefficient index k is checked against 63 before every store, and every store lands in
//     the block being decoded, inside coef[0, mcus * 384);
//   - table indices are masked to the table sizes.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VTF_HD __host__ __device__
#else
#define VTF_HD
#endif

namespace vtf {
namespace jpg {

enum { ST_OK = 0, ST_UNSUPPORTED = 1, ST_CORRUPT = 2, ST_TOO_LARGE = 3 };

constexpr int LOOK_BITS = 9;

// One Huffman table, built by build_huff() from a DHT segment
struct HuffTable {
    uint16_t look[1 << LOOK_BITS];  // by the next 9 bits: length << 8 | symbol, 0 = a longer code
    int32_t maxcode[17];            // [l]: largest code of length l, -1 = none
    int32_t valoff[17];             // [l]: index of the first symbol of length l minus its code
    uint8_t vals[256];
};

// The tables of one file, per component
struct HuffSet {
    HuffTable dc[3], ac[3];
};

// bits[16] = codes per length, vals = n symbols in code order.  The caller has checked that the
// canonical codes fit their lengths (jpeg_parse.hpp).
inline void build_huff(const uint8_t* bits, const uint8_t* vals, int n, HuffTable& t) {
    for (int i = 0; i < (1 << LOOK_BITS); i++) t.look[i] = 0;
    for (int i = 0; i < 256; i++) t.vals[i] = i < n ? vals[i] : 0;
    int code = 0, k = 0;
    t.maxcode[0] = -1, t.valoff[0] = 0;
    for (int l = 1; l <= 16; l++) {
        t.valoff[l] = k - code;
        for (int i = 0; i < bits[l - 1] && k < 256; i++, k++, code++) {
            if (l <= LOOK_BITS) {
                const int lo = code << (LOOK_BITS - l);
                for (int j = 0; j < (1 << (LOOK_BITS - l)); j++)
                    t.look[(lo + j) & ((1 << LOOK_BITS) - 1)] = (uint16_t)((l << 8) | t.vals[k]);
            }
        }
        t.maxcode[l] = bits[l - 1] ? code - 1 : -1;
        code <<= 1;
    }
}

// MSB-first bit reader with the FF 00 unstuffing inside.  The bytes come in through an 8-byte cache
// (one load per 8 bytes while at least 8 remain before `end`, single bytes after that), and four
// bytes without a 0xFF go into the accumulator at once.
struct BitReader {
    const uint8_t* data;
    int64_t pos, end;  // pos: the first byte not yet consumed (the cache's first byte when cn > 0)
    uint64_t cache;    // the next cn bytes, the first one in the low 8 bits
    int cn;
    uint64_t acc;      // the low `n` bits are valid, the oldest on top
    int n;
    int pad;           // how many of the valid bits are zeros fed past the end / a marker

    VTF_HD void init(const uint8_t* d, int64_t begin, int64_t e) {
        data = d, pos = begin, end = e < begin ? begin : e;
        cache = 0, cn = 0, acc = 0, n = 0, pad = 0;
    }
    VTF_HD void refill() {
        if (pos + 8 <= end) {
            uint8_t b[8];
            __builtin_memcpy(b, data + pos, 8);
            cache = 0;
            for (int i = 7; i >= 0; i--) cache = (cache << 8) | b[i];
            cn = 8;
        } else if (pos < end) {
            cache = data[pos];
            cn = 1;
        }
    }
    // at least 32 valid bits afterwards
    VTF_HD void fill() {
        while (n <= 32) {
            if (cn == 0) refill();
            uint32_t b = 0;
            if (cn == 0) {  // past the end
                pad += 8;
            } else {
                const uint32_t v = (uint32_t)cache, x = ~v;
                if (cn >= 4 && ((x - 0x01010101u) & ~x & 0x80808080u) == 0) {  // four bytes, none 0xFF
                    acc = (acc << 32) | __builtin_bswap32(v);
                    n += 32;
                    cache >>= 32, cn -= 4, pos += 4;
                    continue;
                }
                b = v & 0xFF;
                if (b != 0xFF) {
                    cache >>= 8, cn -= 1, pos += 1;
                } else {
                    int next = -1;
                    if (cn >= 2) next = (int)((v >> 8) & 0xFF);
                    else if (pos + 1 < end) next = data[pos + 1];
                    if (next == 0x00) {  // a stuffed 0xFF
                        if (cn >= 2) cache >>= 16, cn -= 2;
                        else cn = 0;
                        pos += 2;
                    } else {  // a marker, or 0xFF as the last byte: the scan is over
                        end = pos, cn = 0;
                        b = 0;
                        pad += 8;
                    }
                }
            }
            acc = (acc << 8) | b;
            n += 8;
        }
    }
    // the next nb (1..16) bits without consuming them; needs n >= nb
    VTF_HD uint32_t peek(int nb) const { return (uint32_t)(acc >> (n - nb)) & ((1u << nb) - 1); }
    VTF_HD void skip(int nb) { n -= nb; }
    VTF_HD bool overrun() const { return n < pad; }
};

// Decodes one symbol; -1 for a bit pattern that is no code.  Needs 16 bits in the reader (a symbol
// and its value bits take at most 16 + 11: fill() before every symbol is enough).
VTF_HD inline int huff_symbol(BitReader& br, const HuffTable* t) {
    const uint32_t c16 = br.peek(16);
    const uint32_t e = t->look[c16 >> (16 - LOOK_BITS)];
    if (e) {
        br.skip((int)(e >> 8));
        return (int)(e & 255);
    }
    for (int l = LOOK_BITS + 1; l <= 16; l++) {
        const int code = (int)(c16 >> (16 - l));
        if (code <= t->maxcode[l]) {
            br.skip(l);
            return t->vals[(t->valoff[l] + code) & 255];
        }
    }
    return -1;
}

// s (1..15) more bits as a signed value (jdhuff.c HUFF_EXTEND)
VTF_HD inline int receive_extend(BitReader& br, int s) {
    const int v = (int)br.peek(s);
    br.skip(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// data[begin, end) = the scan's bytes, hs = the file's tables, coef = mcus * 384 zeroed int16.
// Returns ST_OK or ST_CORRUPT; on ST_CORRUPT decoding stopped at the bad block.
VTF_HD inline int entropy_decode(const uint8_t* data, int64_t begin, int64_t end, const HuffSet* hs, int mcus,
                                 int16_t* coef) {
    BitReader br;
    br.init(data, begin, end);
    int pred[3] = {0, 0, 0};
    for (int m = 0; m < mcus; m++) {
        for (int b = 0; b < 6; b++) {
            const int c = b < 4 ? 0 : b - 3;
            int16_t* blk = coef + ((int64_t)m * 6 + b) * 64;
            const HuffTable* dct = &hs->dc[c];
            const HuffTable* act = &hs->ac[c];
            br.fill();
            int s = huff_symbol(br, dct);
            if (s < 0 || s > 11) return ST_CORRUPT;
            if (s) pred[c] = (int)((uint32_t)pred[c] + (uint32_t)receive_extend(br, s));  // (wraps, no UB)
            blk[0] = (int16_t)pred[c];
            for (int k = 1; k < 64;) {
                br.fill();
                const int rs = huff_symbol(br, act);
                if (rs < 0) return ST_CORRUPT;
                const int r = rs >> 4;
                s = rs & 15;
                if (s == 0) {
                    if (r != 15) break;  // EOB
                    k += 16;             // ZRL
                    continue;
                }
                if (s > 10) return ST_CORRUPT;
                k += r;
                if (k > 63) return ST_CORRUPT;
                blk[k++] = (int16_t)receive_extend(br, s);
            }
            if (br.overrun()) return ST_CORRUPT;
        }
    }
    return ST_OK;
}

}  // namespace jpg
}  // namespace vtf
