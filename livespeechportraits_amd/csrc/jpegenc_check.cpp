// jpegenc_check.cpp -- the host/device half of the JPEG encoder's options (jpegenc_core.h) as a stand-alone program for AddressSanitizer and
// UBSan: it never runs on a device and is never loaded into Python.
//   jpegenc_check <bundle>
// bundle: "LSEH", uint32 count, then per histogram: uint32 freq[256], uint8 bits[17], uint32 n, uint8 huffval[n] (what the Python restatement of
// jpeg_gen_optimal_table gives).  Every histogram goes through huff_merge<1> + huff_finish + huff_codes and must give those tables and a
// prefix-free canonical code without an all-ones word; then the interval bookkeeping is walked block by block against a plain loop over MCUs
// for a list of geometries, and the capacity formula is checked against the bytes such a frame can at most take.
#include "jpegenc_core.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace lspenc;

static int failures = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            ++failures;                   \
            std::fprintf(stderr, "FAIL "); \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fprintf(stderr, "\n");   \
        }                                 \
    } while (0)

static void check_table(size_t idx, const uint32_t *freq, const unsigned char *want_bits, const std::vector<unsigned char> &want_vals)
{
    uint16_t codesize[kSymbols];
    unsigned char bits[17], vals[256];
    uint32_t codes[256];
    huff_merge<1>(freq, 0, codesize, OneLane());
    const int n = huff_finish(codesize, bits, vals);
    CHECK(n == (int)want_vals.size(), "histogram %zu: %d symbols, expected %zu", idx, n, want_vals.size());
    CHECK(std::memcmp(bits, want_bits, 17) == 0, "histogram %zu: the counts per length differ", idx);
    CHECK(n == (int)want_vals.size() && (n == 0 || std::memcmp(vals, want_vals.data(), (size_t)n) == 0), "histogram %zu: the symbol order differs", idx);
    int total = 0;
    uint64_t kraft = 0;                                  // in units of 2^-16
    for (int l = 1; l <= 16; ++l) {
        total += bits[l];
        kraft += (uint64_t)bits[l] << (16 - l);
    }
    CHECK(total == n, "histogram %zu: the counts add up to %d, not %d", idx, total, n);
    CHECK(kraft < (1u << 16) || n == 0, "histogram %zu: no room for the all-ones code (Kraft sum %llu / 65536)", idx, (unsigned long long)kraft);
    huff_codes(bits, vals, codes);
    for (int s = 0; s < 256; ++s) {
        const uint32_t len = codes[s] >> 16, code = codes[s] & 0xffffu;
        CHECK((len != 0) == (freq[s] != 0), "histogram %zu: symbol %d has count %u and length %u", idx, s, freq[s], len);
        if (len) CHECK(len <= 16 && code < (1u << len) - 1u, "histogram %zu: symbol %d has code %u of %u bits", idx, s, code, len);
    }
}

static void check_intervals(int mcux, int mcuy, int bpm, int restart)
{
    const int nmcu = mcux * mcuy, nblk = nmcu * bpm;
    const int nint = interval_count(nmcu, restart), ibl = interval_blocks(nmcu, restart, bpm);
    std::vector<int> last(3);
    int seen = 0, g = 0;
    for (int m = 0; m < nmcu; ++m) {
        const bool first = restart > 0 ? m % restart == 0 : m == 0;
        if (first) {
            last.assign(3, -1);
            if (m) ++seen;
        }
        for (int j = 0; j < bpm; ++j, ++g) {
            const int c = bpm == 1 ? 0 : j < 4 ? 0 : j - 3;
            CHECK(interval_of(g, ibl) == seen, "%dx%d bpm %d restart %d: block %d in interval %d, expected %d", mcux, mcuy, bpm, restart, g, interval_of(g, ibl), seen);
            CHECK(pred_block(g, ibl, bpm) == last[c], "%dx%d bpm %d restart %d: block %d predicted from %d, expected %d", mcux, mcuy, bpm, restart, g,
                  pred_block(g, ibl, bpm), last[c]);
            last[c] = g;
            const bool ends = j == bpm - 1 && (m == nmcu - 1 || (restart > 0 && (m + 1) % restart == 0));
            CHECK((g + 1 == interval_end(interval_of(g, ibl), ibl, nblk)) == ends, "%dx%d bpm %d restart %d: end of interval at block %d", mcux, mcuy, bpm, restart, g);
        }
    }
    CHECK(seen + 1 == nint, "%dx%d bpm %d restart %d: %d intervals, expected %d", mcux, mcuy, bpm, restart, nint, seen + 1);
    // the most a frame can take: every block at its bit bound, every interval padded to a byte, every byte stuffed
    for (int optimize = 0; optimize < 2; ++optimize) {
        const uint64_t bb = optimize ? kBlockBitsOpt : kBlockBitsStd;
        uint64_t bytes = 0;
        for (int i = 0; i < nint; ++i) bytes += padded_bytes((uint32_t)((uint64_t)(interval_end(i, ibl, nblk) - i * ibl) * bb));
        const uint64_t worst = (optimize ? kPrefixBound : 0) + 2 * bytes + 2 * (uint64_t)(nint - 1) + 2;
        CHECK(worst <= capacity_bound((uint64_t)nblk, (uint64_t)nint, optimize), "%dx%d bpm %d restart %d optimize %d: %llu bytes pass the bound", mcux, mcuy, bpm,
              restart, optimize, (unsigned long long)worst);
    }
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: jpegenc_check <bundle>\n");
        return 2;
    }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    char magic[4];
    uint32_t count = 0;
    if (std::fread(magic, 1, 4, f) != 4 || std::memcmp(magic, "LSEH", 4) != 0 || std::fread(&count, 4, 1, f) != 1) {
        std::fprintf(stderr, "not a histogram bundle\n");
        return 2;
    }
    size_t done = 0;
    for (uint32_t k = 0; k < count; ++k) {
        std::vector<uint32_t> freq(256);
        unsigned char bits[17];
        uint32_t n = 0;
        if (std::fread(freq.data(), 4, 256, f) != 256 || std::fread(bits, 1, 17, f) != 17 || std::fread(&n, 4, 1, f) != 1 || n > 256) {
            std::fprintf(stderr, "truncated bundle at histogram %u\n", k);
            return 2;
        }
        std::vector<unsigned char> vals(n);
        if (n && std::fread(vals.data(), 1, n, f) != n) {
            std::fprintf(stderr, "truncated bundle at histogram %u\n", k);
            return 2;
        }
        check_table(k, freq.data(), bits, vals);
        ++done;
    }
    std::fclose(f);
    size_t geometries = 0;
    const int shapes[][3] = {{1, 1, 1}, {1, 1, 6}, {3, 3, 6}, {5, 3, 1}, {3, 2, 6}, {32, 32, 6}, {64, 64, 1}, {7, 1, 6}, {1, 9, 1}};
    for (const auto &s : shapes)
        for (int restart : {0, 1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 1000, 65535}) {
            check_intervals(s[0], s[1], s[2], restart);
            ++geometries;
        }
    std::printf("jpegenc_check: %zu histograms, %zu geometries; %d failures\n", done, geometries, failures);
    return failures ? 1 : 0;
}
