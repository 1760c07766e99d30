// Header parser of the device JPEG decoder (jpeg_decode.hip): plain host C++, no HIP, so a
// stand-alone program can compile it (tests/host/jpeg_decode_fuzz.cpp).
//
// parse() walks the marker segments of one file up to its first scan and classifies it:
//   KIND_DEVICE       baseline (SOF0) 8-bit, three components sampled 2x2 / 1x1 / 1x1, one interleaved
//                     scan (Ss 0, Se 63, Ah = Al = 0), 8-bit quantisation tables, no restart interval, no
//                     Adobe APP14 segment, EXIF orientation absent or 1, and nothing but EOI after the scan;
//   KIND_UNSUPPORTED  a JPEG whose headers are whole but which is something else (progressive, other
//                     sampling, grayscale, CMYK, DRI, several scans, 16-bit DQT, arithmetic coding, ...);
//   KIND_INVALID      no SOI, or the headers end before the scan starts.
// Every read is inside [data, data + len).
#pragma once

#include <cstdint>
#include <cstring>

namespace vtf {
namespace jpg {

enum { KIND_DEVICE = 0, KIND_UNSUPPORTED = 1, KIND_INVALID = 2 };

// why a file is KIND_UNSUPPORTED (bits of Parsed::why, info[5] of vtf_jpeg_probe)
enum {
    WHY_SOF = 1,          // not SOF0 (progressive, extended, lossless, arithmetic)
    WHY_PRECISION = 2,    // not 8-bit samples, or a 16-bit quantisation table
    WHY_COMPONENTS = 4,   // not three YCbCr components (grayscale, CMYK, RGB named by its component ids)
    WHY_SAMPLING = 8,     // not 2x2, 1x1, 1x1
    WHY_RESTART = 16,     // DRI with a nonzero interval
    WHY_ADOBE = 32,       // APP14 Adobe segment (colour transform flag)
    WHY_ORIENTATION = 64, // EXIF orientation other than 1
    WHY_SCAN = 128,       // scan parameters, not interleaved, or more after the scan than EOI
    WHY_TABLES = 256,     // a table the scan names is missing or malformed
    WHY_SIZE = 512,       // zero width, height from a DNL marker, or a file of 2 GiB or more
};

struct HuffSpec {
    uint8_t bits[16];   // codes per length 1..16
    uint8_t vals[256];  // symbols in code order (zero padded)
    int n;              // number of symbols; -1 = not defined
};

struct Parsed {
    int kind, why;
    int h, w, ncomp;
    int64_t scan_begin, scan_end;  // entropy-coded bytes: [scan_begin, scan_end), no marker inside
    uint16_t q[3][64];             // quantisation table of each component, zigzag order
    HuffSpec dc[3], ac[3];         // Huffman tables of each component
};

namespace detail {

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// EXIF orientation of an APP1 body [p, p + n) ("Exif\0\0" + TIFF); 1 when absent or unreadable
inline int exif_orientation(const uint8_t* p, int64_t n) {
    if (n < 14 || std::memcmp(p, "Exif\0\0", 6) != 0) return 1;
    const uint8_t* t = p + 6;
    const int64_t tn = n - 6;
    bool le;
    if (t[0] == 'I' && t[1] == 'I') le = true;
    else if (t[0] == 'M' && t[1] == 'M') le = false;
    else return 1;
    auto u16 = [&](int64_t at) -> uint32_t { return le ? t[at] | (t[at + 1] << 8) : (t[at] << 8) | t[at + 1]; };
    auto u32 = [&](int64_t at) -> uint32_t {
        return le ? u16(at) | (u16(at + 2) << 16) : (u16(at) << 16) | u16(at + 2);
    };
    if (u16(2) != 42) return 1;
    const int64_t ifd = u32(4);
    if (ifd < 8 || ifd + 2 > tn) return 1;
    const int64_t cnt = u16(ifd);
    for (int64_t i = 0; i < cnt; i++) {
        const int64_t e = ifd + 2 + 12 * i;
        if (e + 12 > tn) return 1;
        if (u16(e) == 0x0112) return u16(e + 2) == 3 ? (int)u16(e + 8) : 1;
    }
    return 1;
}

}  // namespace detail

inline int parse(const uint8_t* data, int64_t len, Parsed& P) {
    using detail::be16;
    std::memset(&P, 0, sizeof(P));
    P.kind = KIND_INVALID;
    if (!data || len < 4 || data[0] != 0xFF || data[1] != 0xD8) return P.kind;
    if (len >= ((int64_t)1 << 31)) {
        P.kind = KIND_UNSUPPORTED, P.why = WHY_SIZE;
        return P.kind;
    }
    uint16_t qt[4][64];
    bool have_q[4] = {false, false, false, false};
    // tables as the file defines them: [0..3] DC, [4..7] AC (static storage would not be
    // thread-safe; 8 x 276 bytes on the stack is fine)
    HuffSpec ht[8];
    for (auto& t : ht) t.n = -1;
    int comp_id[3] = {0, 0, 0}, comp_hv[3] = {0, 0, 0}, comp_tq[3] = {0, 0, 0};
    bool have_sof = false, have_jfif = false;
    int why = 0;
    int64_t at = 2;
    for (;;) {
        // next marker: 0xFF, any number of fill 0xFF bytes, the code
        if (at + 2 > len || data[at] != 0xFF) return P.kind;
        while (at < len && data[at] == 0xFF) at++;
        if (at >= len) return P.kind;
        const int m = data[at++];
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;  // stand-alone markers
        if (m == 0x00 || m == 0xD8 || m == 0xD9) return P.kind;  // stuffing, SOI, EOI: no scan here
        if (at + 2 > len) return P.kind;
        const int L = be16(data + at);
        if (L < 2 || at + L > len) return P.kind;
        const uint8_t* s = data + at + 2;  // segment body [s, s + n)
        const int n = L - 2;
        at += L;
        if (m == 0xC0 || m == 0xC1 || m == 0xC2 || m == 0xC3 || (m >= 0xC5 && m <= 0xC7) ||
            (m >= 0xC9 && m <= 0xCB) || (m >= 0xCD && m <= 0xCF)) {
            if (have_sof || n < 6) return P.kind;
            have_sof = true;
            if (m != 0xC0) why |= WHY_SOF;
            if (s[0] != 8) why |= WHY_PRECISION;
            P.h = be16(s + 1), P.w = be16(s + 3), P.ncomp = s[5];
            if (n < 6 + 3 * P.ncomp || P.ncomp == 0) return P.kind;
            if (P.w == 0 || P.h == 0) why |= WHY_SIZE;
            if (P.ncomp != 3) {
                why |= WHY_COMPONENTS;
            } else {
                for (int c = 0; c < 3; c++) {
                    comp_id[c] = s[6 + 3 * c], comp_hv[c] = s[7 + 3 * c], comp_tq[c] = s[8 + 3 * c];
                    if (comp_tq[c] > 3) why |= WHY_TABLES;
                }
                if (comp_hv[0] != 0x22 || comp_hv[1] != 0x11 || comp_hv[2] != 0x11) why |= WHY_SAMPLING;
            }
        } else if (m == 0xC4) {  // DHT: any number of tables
            int64_t o = 0;
            while (o < n) {
                if (o + 17 > n) return P.kind;
                const int tc = s[o] >> 4, th = s[o] & 15;
                int cnt = 0;
                for (int i = 0; i < 16; i++) cnt += s[o + 1 + i];
                if (o + 17 + cnt > n) return P.kind;
                if (tc > 1 || th > 3 || cnt > 256) {
                    why |= WHY_TABLES;
                } else {
                    HuffSpec& t = ht[tc * 4 + th];
                    std::memcpy(t.bits, s + o + 1, 16);
                    std::memset(t.vals, 0, 256);
                    std::memcpy(t.vals, s + o + 17, cnt);
                    t.n = cnt;
                    // canonical codes must fit their length (jdhuff.c jpeg_make_d_derived_tbl)
                    uint32_t code = 0;
                    for (int l = 1; l <= 16; l++) {
                        code += t.bits[l - 1];
                        if (code > (1u << l)) {
                            t.n = -1;
                            why |= WHY_TABLES;
                            break;
                        }
                        code <<= 1;
                    }
                }
                o += 17 + cnt;
            }
        } else if (m == 0xCC) {  // DAC: arithmetic coding conditioning
            why |= WHY_SOF;
        } else if (m == 0xDB) {  // DQT: any number of tables
            int64_t o = 0;
            while (o < n) {
                const int pq = s[o] >> 4, tq = s[o] & 15;
                const int sz = pq ? 128 : 64;
                if (pq > 1 || o + 1 + sz > n) return P.kind;
                if (pq) why |= WHY_PRECISION;
                if (tq > 3) {
                    why |= WHY_TABLES;
                } else {
                    for (int k = 0; k < 64; k++)
                        qt[tq][k] = pq ? (uint16_t)be16(s + o + 1 + 2 * k) : (uint16_t)s[o + 1 + k];
                    have_q[tq] = true;
                }
                o += 1 + sz;
            }
        } else if (m == 0xDD) {  // DRI
            if (n < 2) return P.kind;
            if (be16(s) != 0) why |= WHY_RESTART;
        } else if (m == 0xE0) {  // APP0
            if (n >= 14 && std::memcmp(s, "JFIF\0", 5) == 0) have_jfif = true;
        } else if (m == 0xEE) {  // APP14
            if (n >= 5 && std::memcmp(s, "Adobe", 5) == 0) why |= WHY_ADOBE;
        } else if (m == 0xE1) {  // APP1
            if (detail::exif_orientation(s, n) != 1) why |= WHY_ORIENTATION;
        } else if (m == 0xDA) {  // SOS: the headers are whole
            if (!have_sof || n < 1) return P.kind;
            const int ns = s[0];
            if (n < 1 + 2 * ns + 3) return P.kind;
            if (at >= len) return P.kind;  // nothing after the headers
            if (ns != P.ncomp) why |= WHY_SCAN;
            // jdapimin.c default_decompress_parms: without a JFIF (or Adobe) segment, components named
            // 'R', 'G', 'B' are RGB samples, not YCbCr
            if (P.ncomp == 3 && !have_jfif && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B')
                why |= WHY_COMPONENTS;
            if (!why) {
                for (int c = 0; c < 3; c++) {
                    if (s[1 + 2 * c] != comp_id[c]) why |= WHY_SCAN;
                    const int td = s[2 + 2 * c] >> 4, ta = s[2 + 2 * c] & 15;
                    if (td > 3 || ta > 3 || ht[td].n < 0 || ht[4 + ta].n < 0 || !have_q[comp_tq[c]]) {
                        why |= WHY_TABLES;
                        continue;
                    }
                    P.dc[c] = ht[td], P.ac[c] = ht[4 + ta];
                    std::memcpy(P.q[c], qt[comp_tq[c]], sizeof(P.q[c]));
                }
                if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) why |= WHY_SCAN;
            }
            // the scan ends at the first marker (0xFF followed by anything but the stuffed 0x00)
            P.scan_begin = at;
            int64_t e = at;
            for (;;) {
                const void* f = std::memchr(data + e, 0xFF, (size_t)(len - e));
                if (!f) {
                    e = len;
                    break;
                }
                e = (const uint8_t*)f - data;
                if (e + 1 >= len || data[e + 1] != 0x00) break;
                e += 2;
            }
            P.scan_end = e;
            // a marker after the scan other than EOI: restart markers, further scans, DNL
            if (e + 1 < len && data[e + 1] != 0xD9) why |= WHY_SCAN;
            P.why = why;
            P.kind = why ? KIND_UNSUPPORTED : KIND_DEVICE;
            return P.kind;
        }
        // every other segment (APPn, COM, ...) is skipped
    }
}

}  // namespace jpg
}  // namespace vtf
