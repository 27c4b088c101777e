// jpegdec_check.cpp -- the host half of the JPEG decoder (jpegdec_core.h, jpegdec_plan.h) as a stand-alone program for AddressSanitizer and
// UBSan (make check-jpegdec).  Host code only: it is never run on a device and never loaded into Python.
//
//   jpegdec_check <bundle> <seed> <truncated files> <corruptions per file>
//
// The bundle (written by tests/test_jpeg_decode_cpu.py) is "LSDB", a uint32 count, then per file: uint32 length, uint32 expected status,
// uint32 count of expected int16 coefficients, the file's bytes, the coefficients (MCU order, natural order inside a block).  A bundle that
// starts with "LSDP" instead (tests/test_jpeg_progressive_cpu.py) has the same layout and is planned with kFlagProgressive throughout: its entries
// are progressive files, baseline files beside them, and the refusals of that flag.  The program
//   1. plans and decodes every file alone and all of them as one batch: status and coefficients must be the expected ones;
//   2. does the same for every truncation length of the first <truncated files> files;
//   3. and for <corruptions per file> single-byte changes of every file, positions and values from a 64-bit LCG started at <seed>.
// For a changed file any status is right, and so are the original coefficients; what must not happen is a sanitizer report.  Every input is
// copied into an allocation of exactly its size, so a read one byte past the end is a report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpegdec_plan.h"

using namespace lspdec;

namespace {

struct Entry {
    std::vector<uint8_t> bytes;
    uint32_t status;
    std::vector<int16_t> coef;
};

struct Result {
    uint32_t status;
    std::vector<int16_t> coef;
};

// plan + stage 1 of a batch; every file lives in its own exact-size allocation
uint32_t g_flags = 0;                                   // of the bundle: every plan of the run is made with them

std::vector<Result> run(const std::vector<const std::vector<uint8_t> *> &batch)
{
    std::vector<uint8_t *> copies;
    std::vector<const uint8_t *> ptrs;
    std::vector<size_t> lens;
    for (const auto *f : batch) {
        uint8_t *c = static_cast<uint8_t *>(std::malloc(f->size() ? f->size() : 1));
        if (f->size()) std::memcpy(c, f->data(), f->size());
        copies.push_back(c);
        ptrs.push_back(c);
        lens.push_back(f->size());
    }
    const int n = (int)batch.size();
    const int64_t need = plan(ptrs.data(), lens.data(), nullptr, n, 8192, nullptr, g_flags);
    std::vector<Result> out(n);
    if (need < 0) {
        std::fprintf(stderr, "plan refused the batch (%lld)\n", (long long)need);
        std::exit(2);
    }
    void *blob = std::aligned_alloc(16, (size_t)need);
    if (plan(ptrs.data(), lens.data(), nullptr, n, 8192, blob, g_flags) != need) {
        std::fprintf(stderr, "plan wrote another size than it announced\n");
        std::exit(2);
    }
    for (int i = 0; i < n; ++i) {
        const FileDesc &d = files_of(blob)[i];
        out[i].status = d.status;
        if (d.status != ST_OK) continue;
        out[i].coef.assign((size_t)d.nblk * 64, 0);
        out[i].status = host_coefficients(blob, i, out[i].coef.data());
        if (out[i].status != ST_OK) out[i].coef.clear();
    }
    std::free(blob);
    for (uint8_t *c : copies) std::free(c);
    return out;
}

uint32_t read32(FILE *f)
{
    uint8_t b[4];
    if (std::fread(b, 1, 4, f) != 4) {
        std::fprintf(stderr, "bundle ends early\n");
        std::exit(2);
    }
    return b[0] | (b[1] << 8) | (b[2] << 16) | ((uint32_t)b[3] << 24);
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 5) {
        std::fprintf(stderr, "usage: jpegdec_check <bundle> <seed> <truncated files> <corruptions per file>\n");
        return 2;
    }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    uint64_t lcg = std::strtoull(argv[2], nullptr, 10);
    const size_t ntrunc = std::strtoul(argv[3], nullptr, 10), ncorrupt = std::strtoul(argv[4], nullptr, 10);
    char magic[4];
    if (std::fread(magic, 1, 4, f) != 4 || (std::memcmp(magic, "LSDB", 4) && std::memcmp(magic, "LSDP", 4))) {
        std::fprintf(stderr, "not a bundle\n");
        return 2;
    }
    g_flags = std::memcmp(magic, "LSDP", 4) ? 0u : kFlagProgressive;
    std::vector<Entry> entries(read32(f));
    for (Entry &e : entries) {
        const uint32_t len = read32(f);
        e.status = read32(f);
        const uint32_t ncoef = read32(f);
        e.bytes.resize(len);
        e.coef.resize(ncoef);
        if ((len && std::fread(e.bytes.data(), 1, len, f) != len) || (ncoef && std::fread(e.coef.data(), 2, ncoef, f) != ncoef)) {
            std::fprintf(stderr, "bundle ends early\n");
            return 2;
        }
    }
    std::fclose(f);

    int failures = 0;
    const auto expect = [&](const char *what, size_t i, const Result &r, const Entry &e) {
        if (r.status != e.status || (e.status == ST_OK && r.coef != e.coef)) {
            std::fprintf(stderr, "%s: file %zu: status %u (expected %u)%s\n", what, i, r.status, e.status, r.status == e.status ? ", other coefficients" : "");
            ++failures;
        }
    };
    // 1. alone, and as one batch
    std::vector<const std::vector<uint8_t> *> all;
    for (size_t i = 0; i < entries.size(); ++i) {
        expect("alone", i, run({&entries[i].bytes})[0], entries[i]);
        all.push_back(&entries[i].bytes);
    }
    const std::vector<Result> together = run(all);
    for (size_t i = 0; i < entries.size(); ++i) expect("batch", i, together[i], entries[i]);

    // 2. every truncation length of the first files, 3. single-byte corruptions of all
    size_t counts[4] = {0, 0, 0, 0}, same = 0, ran = 0;
    const auto mutated = [&](const char *what, size_t i, const std::vector<uint8_t> &m) {
        const Result r = run({&m})[0];
        ++ran;
        ++counts[r.status < 4 ? r.status : 3];
        if (r.status == ST_OK && entries[i].status == ST_OK && r.coef == entries[i].coef) ++same;
        if (r.status > ST_RANGE) {
            std::fprintf(stderr, "%s of file %zu: status %u is no status\n", what, i, r.status);
            ++failures;
        }
    };
    for (size_t i = 0; i < entries.size() && i < ntrunc; ++i)
        for (size_t len = 0; len < entries[i].bytes.size(); ++len) {
            const std::vector<uint8_t> m(entries[i].bytes.begin(), entries[i].bytes.begin() + len);
            const Result r = run({&m})[0];
            ++ran;
            ++counts[r.status < 4 ? r.status : 3];
            if (r.status == ST_OK && !(entries[i].status == ST_OK && r.coef == entries[i].coef)) {     // a shorter file that decodes is the same picture
                std::fprintf(stderr, "truncation of file %zu to %zu bytes decodes to other coefficients\n", i, len);
                ++failures;
            }
        }
    for (size_t i = 0; i < entries.size(); ++i)
        for (size_t k = 0; k < ncorrupt && !entries[i].bytes.empty(); ++k) {
            lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
            std::vector<uint8_t> m = entries[i].bytes;
            const size_t at = (size_t)((lcg >> 33) % m.size());
            m[at] ^= (uint8_t)(1 + ((lcg >> 20) % 255));                       // never the same byte again
            mutated("corruption", i, m);
        }
    std::printf("jpegdec_check: %zu files, %zu changed inputs: %zu decoded (%zu to the original coefficients), %zu unsupported, %zu corrupt, %zu range; %d failures\n",
                entries.size(), ran, counts[0], same, counts[1], counts[2], counts[3], failures);
    return failures ? 1 : 0;
}
