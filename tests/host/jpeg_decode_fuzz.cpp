// CPU robustness check of the device JPEG decoder's host-side parser (jpeg_parse.hpp) and of the
// entropy decoder the kernel runs (jpeg_entropy.hpp, __host__ __device__).  Built by
// tests/test_jpeg_decode.py with -fsanitize=address,undefined and run as
//   jpeg_decode_fuzz a.jpg a.coef b.jpg b.coef ...
// where X.coef holds the expected int16 coefficients [mcus][6][64] of X.jpg.  For every file:
//   - the unmodified bytes parse as decodable and decode to exactly the expected coefficients;
//   - every truncation, and a few thousand seeded byte flips and random tails, go through the
//     parser and (when still decodable) the entropy decoder; the kind and the status must be
//     defined values.
// Every input and every coefficient buffer is a heap block of its exact size, so a read or a write
// one byte outside is a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "../../video-to-faces_amd/csrc/jpeg_entropy.hpp"
#include "../../video-to-faces_amd/csrc/jpeg_parse.hpp"

using namespace vtf::jpg;

static std::vector<uint8_t> read_file(const char* path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) {
        std::fprintf(stderr, "cannot read %s\n", path);
        std::exit(2);
    }
    return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {  // xorshift64*
    g_rng ^= g_rng >> 12, g_rng ^= g_rng << 25, g_rng ^= g_rng >> 27;
    return (uint32_t)((g_rng * 0x2545F4914F6CDD1Dull) >> 32);
}

struct Counts {
    long kinds[3] = {0, 0, 0}, ok = 0, corrupt = 0, skipped = 0;
};

#define REQUIRE(cond, ...)                 \
    do {                                   \
        if (!(cond)) {                     \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fprintf(stderr, "\n");    \
            std::exit(1);                  \
        }                                  \
    } while (0)

// parser + entropy decoder on one input; returns the status (-1: not decoded) and the coefficients
static int run(const std::vector<uint8_t>& in, Counts& n, std::vector<int16_t>* coef_out = nullptr) {
    // an exact-size heap copy (a vector's capacity may exceed its size)
    uint8_t* data = (uint8_t*)std::malloc(in.size() ? in.size() : 1);
    if (!in.empty()) std::memcpy(data, in.data(), in.size());
    Parsed P;
    const int kind = parse(data, (int64_t)in.size(), P);
    REQUIRE(kind == KIND_DEVICE || kind == KIND_UNSUPPORTED || kind == KIND_INVALID, "undefined kind %d", kind);
    n.kinds[kind]++;
    int st = -1;
    if (kind == KIND_DEVICE) {
        REQUIRE(P.h > 0 && P.w > 0 && P.scan_begin > 0 && P.scan_begin <= P.scan_end &&
                    P.scan_end <= (int64_t)in.size(),
                "bad parse result %d x %d, scan [%lld, %lld) of %zu", P.h, P.w, (long long)P.scan_begin,
                (long long)P.scan_end, in.size());
        const int64_t mcus = (int64_t)((P.w + 15) >> 4) * ((P.h + 15) >> 4);
        if (mcus > 4096) {  // a flipped size field: too much memory for this program
            n.skipped++;
        } else {
            HuffSet* hs = (HuffSet*)std::malloc(sizeof(HuffSet));
            for (int c = 0; c < 3; c++) {
                build_huff(P.dc[c].bits, P.dc[c].vals, P.dc[c].n, hs->dc[c]);
                build_huff(P.ac[c].bits, P.ac[c].vals, P.ac[c].n, hs->ac[c]);
            }
            int16_t* coef = (int16_t*)std::calloc((size_t)mcus * 384, sizeof(int16_t));
            st = entropy_decode(data, P.scan_begin, P.scan_end, hs, (int)mcus, coef);
            REQUIRE(st == ST_OK || st == ST_CORRUPT, "undefined status %d", st);
            (st == ST_OK ? n.ok : n.corrupt)++;
            if (coef_out) coef_out->assign(coef, coef + mcus * 384);
            std::free(coef);
            std::free(hs);
        }
    }
    std::free(data);
    return st;
}

int main(int argc, char** argv) {
    REQUIRE(argc >= 3 && argc % 2 == 1, "usage: %s file.jpg file.coef ...", argv[0]);
    Counts n;
    for (int a = 1; a + 1 < argc; a += 2) {
        const std::vector<uint8_t> file = read_file(argv[a]);
        const std::vector<uint8_t> want_b = read_file(argv[a + 1]);
        // unmodified: decodable, ok, the expected coefficients
        std::vector<int16_t> got;
        const int st = run(file, n, &got);
        REQUIRE(st == ST_OK, "%s: status %d", argv[a], st);
        REQUIRE(got.size() * 2 == want_b.size(), "%s: %zu coefficients, fixture has %zu", argv[a], got.size(),
                want_b.size() / 2);
        const int16_t* want = (const int16_t*)want_b.data();
        for (size_t i = 0; i < got.size(); i++)
            REQUIRE(got[i] == want[i], "%s: MCU %zu block %zu k %zu: %d, want %d", argv[a], i / 384, i / 64 % 6, i % 64,
                    got[i], want[i]);
        // every truncation
        for (size_t len = 0; len < file.size(); len++) run(std::vector<uint8_t>(file.begin(), file.begin() + len), n);
        // seeded byte flips (half of them inside the scan) and random tails
        Parsed P;
        parse(file.data(), (int64_t)file.size(), P);
        for (int it = 0; it < 3000; it++) {
            std::vector<uint8_t> v(file);
            const int flips = 1 + rnd() % 4;
            for (int i = 0; i < flips; i++) {
                size_t at = rnd() % v.size();
                if (rnd() & 1) at = (size_t)P.scan_begin + rnd() % (size_t)(v.size() - P.scan_begin);
                v[at] = (rnd() & 3) == 0 ? 0xFF : (uint8_t)rnd();
            }
            run(v, n);
        }
        for (int it = 0; it < 1000; it++) {
            std::vector<uint8_t> v(file.begin(), file.begin() + rnd() % file.size());
            const int tail = rnd() % 64;
            for (int i = 0; i < tail; i++) v.push_back((rnd() & 7) == 0 ? 0xFF : (uint8_t)rnd());
            run(v, n);
        }
    }
    std::printf("inputs: %ld decodable, %ld unsupported, %ld invalid; decoded: %ld ok, %ld corrupt, %ld skipped\n",
                n.kinds[0], n.kinds[1], n.kinds[2], n.ok, n.corrupt, n.skipped);
    return 0;
}
