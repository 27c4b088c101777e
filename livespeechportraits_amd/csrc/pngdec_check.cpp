// pngdec_check.cpp -- the host half of the PNG decoder (pngdec_core.h, pngdec_plan.h) as a stand-alone program for AddressSanitizer and UBSan
// (make check-pngdec).  Host code only: it is never run on a device and never loaded into Python.
//
//   pngdec_check <bundle> <seed> <truncated files> <changes per file>
//
// The bundle (written by tests/test_png_decode_cpu.py) is "LSPB", a uint32 count, then per file: uint32 length, uint32 expected status, uint32 count
// of expected scanline bytes, the file's bytes, the filtered scanlines.  Its entries are fixtures, refusals and re-sealed changes (one byte of the
// deflate body flipped, Adler-32 and CRCs made right again: the inputs that reach the stream-level code).  The program
//   1. plans and decodes every file alone and all of them as one batch, with the code the kernels run (the lanes as loops): the status after all
//      three stages and the scanlines of stage 1 must be the expected ones;
//   2. does the same for every truncation length of the first <truncated files> files;
//   3. and for <changes per file> single-byte changes of every file that decodes, positions and values from a 64-bit LCG started at <seed>.
// Every byte of a PNG file is under a CRC or is a length, so a truncated or changed file must be refused; what must not happen besides is a
// sanitizer report.  Every input is copied into an allocation of exactly its size, so a read one byte past the end is a report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "pngdec_plan.h"

using namespace lsppng;

namespace {

struct Entry {
    std::vector<uint8_t> bytes;
    uint32_t status;
    std::vector<uint8_t> lines;
};

struct Result {
    uint32_t status;
    std::vector<uint8_t> lines;
};

// plan + the three stages of a batch; every file lives in its own exact-size allocation, and so do the scanlines and the pixels
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
    const int64_t need = plan(ptrs.data(), lens.data(), nullptr, n, 8192, nullptr);
    std::vector<Result> out(n);
    if (need < 0) {
        std::fprintf(stderr, "plan refused the batch (%lld)\n", (long long)need);
        std::exit(2);
    }
    void *blob = std::aligned_alloc(16, (size_t)need);
    if (plan(ptrs.data(), lens.data(), nullptr, n, 8192, blob) != need) {
        std::fprintf(stderr, "plan wrote another size than it announced\n");
        std::exit(2);
    }
    std::unique_ptr<InflateMem> mem(new InflateMem());
    for (int i = 0; i < n; ++i) {
        const FileDesc &d = files_of(blob)[i];
        out[i].status = d.status;
        if (d.status != ST_OK) continue;
        uint8_t *lines = static_cast<uint8_t *>(std::malloc(d.raw_bytes));
        out[i].status = host_scanlines(blob, i, mem.get(), lines);
        if (out[i].status == ST_OK) {
            out[i].lines.assign(lines, lines + d.raw_bytes);
            uint8_t *px = static_cast<uint8_t *>(std::malloc((size_t)d.width * d.height * d.ncomp));
            out[i].status = host_pixels(blob, i, lines, px);
            std::free(px);
        }
        if (out[i].status != ST_OK) out[i].lines.clear();
        std::free(lines);
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
        std::fprintf(stderr, "usage: pngdec_check <bundle> <seed> <truncated files> <changes per file>\n");
        return 2;
    }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    uint64_t lcg = std::strtoull(argv[2], nullptr, 10);
    const size_t ntrunc = std::strtoul(argv[3], nullptr, 10), nchange = std::strtoul(argv[4], nullptr, 10);
    char magic[4];
    if (std::fread(magic, 1, 4, f) != 4 || std::memcmp(magic, "LSPB", 4)) {
        std::fprintf(stderr, "not a bundle\n");
        return 2;
    }
    std::vector<Entry> entries(read32(f));
    for (Entry &e : entries) {
        const uint32_t len = read32(f);
        e.status = read32(f);
        const uint32_t nlines = read32(f);
        e.bytes.resize(len);
        e.lines.resize(nlines);
        if ((len && std::fread(e.bytes.data(), 1, len, f) != len) || (nlines && std::fread(e.lines.data(), 1, nlines, f) != nlines)) {
            std::fprintf(stderr, "bundle ends early\n");
            return 2;
        }
    }
    std::fclose(f);

    int failures = 0;
    const auto expect = [&](const char *what, size_t i, const Result &r, const Entry &e) {
        if (r.status != e.status || (e.status == ST_OK && r.lines != e.lines)) {
            std::fprintf(stderr, "%s: file %zu: status %u (expected %u)%s\n", what, i, r.status, e.status, r.status == e.status ? ", other scanlines" : "");
            ++failures;
        }
    };
    // 1. alone, and as one batch
    std::vector<const std::vector<uint8_t> *> all;
    size_t decoded = 0;
    for (size_t i = 0; i < entries.size(); ++i) {
        expect("alone", i, run({&entries[i].bytes})[0], entries[i]);
        all.push_back(&entries[i].bytes);
        decoded += entries[i].status == ST_OK;
    }
    const std::vector<Result> together = run(all);
    for (size_t i = 0; i < entries.size(); ++i) expect("batch", i, together[i], entries[i]);

    // 2. every truncation length of the first files, 3. single-byte changes of the files that decode
    size_t ran = 0;
    const auto refused = [&](const char *what, size_t i, size_t at, const std::vector<uint8_t> &m) {
        const Result r = run({&m})[0];
        ++ran;
        if (r.status != ST_UNSUPPORTED && r.status != ST_CORRUPT) {
            std::fprintf(stderr, "%s of file %zu at %zu: status %u, a changed file must be refused\n", what, i, at, r.status);
            ++failures;
        }
    };
    for (size_t i = 0; i < entries.size() && i < ntrunc; ++i)
        for (size_t len = 0; len < entries[i].bytes.size(); ++len) refused("truncation", i, len, std::vector<uint8_t>(entries[i].bytes.begin(), entries[i].bytes.begin() + len));
    for (size_t i = 0; i < entries.size(); ++i)
        for (size_t k = 0; k < nchange && entries[i].status == ST_OK && entries[i].bytes.size() < 4096; ++k) {
            lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
            std::vector<uint8_t> m = entries[i].bytes;
            const size_t at = (size_t)((lcg >> 33) % m.size());
            m[at] ^= (uint8_t)(1 + ((lcg >> 20) % 255));                       // never the same byte again
            refused("change", i, at, m);
        }
    std::printf("pngdec_check: %zu files (%zu decode), %zu truncated or changed inputs, all refused; %d failures\n", entries.size(), decoded, ran, failures);
    return failures ? 1 : 0;
}
