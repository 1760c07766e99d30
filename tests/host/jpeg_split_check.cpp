// CPU check of the split-scan entropy decoder (jpeg_entropy_split.hpp) against the serial one
// (jpeg_entropy.hpp).  Built by tests/test_mjpeg.py with -fsanitize=address,undefined and run as
//   jpeg_split_check a.jpg b.jpg ... --damage c.jpg d.jpg ...
// For every input and every seg_bytes in {4, 8, 16, 64, 128, 4096} the host driver of passes a-g
// (split_decode_host, the code the kernel's lanes run) and entropy_decode must give
//   - the same status,
//   - when that is ST_OK, byte-equal coefficients,
//   - with at most (number of segments) sync rounds.
// The files after --damage are also run with every truncation and 4,000 seeded byte flips inside
// the scan.  Every input, unstuffed stream and coefficient buffer is a heap block of its exact
// size, so a read or a write one byte outside is a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "../../video-to-faces_amd/csrc/jpeg_entropy_split.hpp"
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

#define REQUIRE(cond, ...)                     \
    do {                                       \
        if (!(cond)) {                         \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fprintf(stderr, "\n");        \
            std::exit(1);                      \
        }                                      \
    } while (0)

struct Counts {
    long ok = 0, corrupt = 0, not_decodable = 0, max_rounds = 0;
};

static const int SEGS[] = {4, 8, 16, 64, 128, 4096};

// -> the serial status, -1 when the parser does not hand the input to the device
static int run(const std::vector<uint8_t>& in, const char* what, Counts& n) {
    uint8_t* data = (uint8_t*)std::malloc(in.size() ? in.size() : 1);
    if (!in.empty()) std::memcpy(data, in.data(), in.size());
    Parsed P;
    int st = -1;
    const int64_t mcus = parse(data, (int64_t)in.size(), P) == KIND_DEVICE
                             ? (int64_t)((P.w + 15) >> 4) * ((P.h + 15) >> 4)
                             : 0;
    if (mcus == 0 || mcus > 4096) {  // (a flipped size field: too much memory for this program)
        n.not_decodable++;
    } else {
        HuffSet* hs = (HuffSet*)std::malloc(sizeof(HuffSet));
        for (int c = 0; c < 3; c++) {
            build_huff(P.dc[c].bits, P.dc[c].vals, P.dc[c].n, hs->dc[c]);
            build_huff(P.ac[c].bits, P.ac[c].vals, P.ac[c].n, hs->ac[c]);
        }
        const size_t nc = (size_t)mcus * 384;
        int16_t* want = (int16_t*)std::calloc(nc, sizeof(int16_t));
        st = entropy_decode(data, P.scan_begin, P.scan_end, hs, (int)mcus, want);
        (st == ST_OK ? n.ok : n.corrupt)++;
        for (int seg : SEGS) {
            int16_t* got = (int16_t*)std::calloc(nc, sizeof(int16_t));
            int64_t nseg = 0, rounds = 0;
            const int st2 = split_decode_host(data, P.scan_begin, P.scan_end, hs, (int)mcus, got, seg, &nseg, &rounds);
            REQUIRE(st2 == st, "%s, seg_bytes %d: status %d, serial %d", what, seg, st2, st);
            REQUIRE(rounds <= nseg, "%s, seg_bytes %d: %lld rounds for %lld segments", what, seg, (long long)rounds,
                    (long long)nseg);
            if (rounds > n.max_rounds) n.max_rounds = (long)rounds;
            if (st == ST_OK)
                for (size_t i = 0; i < nc; i++)
                    REQUIRE(got[i] == want[i], "%s, seg_bytes %d: MCU %zu block %zu k %zu: %d, serial %d", what, seg,
                            i / 384, i / 64 % 6, i % 64, got[i], want[i]);
            std::free(got);
        }
        std::free(want);
        std::free(hs);
    }
    std::free(data);
    return st;
}

int main(int argc, char** argv) {
    REQUIRE(argc >= 2, "usage: %s file.jpg ... [--damage file.jpg ...]", argv[0]);
    Counts n;
    bool damage = false;
    for (int a = 1; a < argc; a++) {
        if (std::strcmp(argv[a], "--damage") == 0) {
            damage = true;
            continue;
        }
        const std::vector<uint8_t> file = read_file(argv[a]);
        REQUIRE(run(file, argv[a], n) == ST_OK, "%s: the undamaged file does not decode", argv[a]);
        if (!damage) continue;
        for (size_t len = 0; len < file.size(); len++) run(std::vector<uint8_t>(file.begin(), file.begin() + len), argv[a], n);
        Parsed P;
        parse(file.data(), (int64_t)file.size(), P);
        for (int it = 0; it < 4000; it++) {
            std::vector<uint8_t> v(file);
            const int flips = 1 + rnd() % 4;
            for (int i = 0; i < flips; i++) {
                const size_t at = (size_t)P.scan_begin + rnd() % (size_t)(P.scan_end - P.scan_begin);
                v[at] = (rnd() & 3) == 0 ? 0xFF : (uint8_t)rnd();
            }
            run(v, argv[a], n);
        }
    }
    std::printf("serial: %ld ok, %ld corrupt, %ld not decodable; split agrees for every seg_bytes; most rounds %ld\n",
                n.ok, n.corrupt, n.not_decodable, n.max_rounds);
    return 0;
}
