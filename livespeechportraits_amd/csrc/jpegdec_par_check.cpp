// jpegdec_par_check.cpp -- the parallel route of the JPEG decoder's stage 1 (jpegdec_core.h decode_subsequence, jpegdec_plan.h
// host_parallel_segment: the kernel's subsequence decoder, fixed point and write pass with the lanes as loops) against the serial host decoder,
// as a stand-alone program for AddressSanitizer and UBSan (make check-jpegdec-par).  Host code only: it is never run on a device and never
// loaded into Python.
//
//   jpegdec_par_check <bundle> <seed> <truncated files> <corruptions per file>
//
// The bundle is jpegdec_check.cpp's ("LSDB" or "LSDP", the latter planned with kFlagProgressive throughout); the expected statuses and
// coefficients it carries are not read: the yardstick is the serial decoder on the same bytes.  The program plans every input twice, without and
// with kFlagParallel, and runs stage 1 on both plans:
//   1. every file alone and all of them as one batch;
//   2. every truncation length of the first <truncated files> files;
//   3. <corruptions per file> single-byte changes of every file, positions and values from a 64-bit LCG started at <seed>.
// Status must equal status, and on status 0 the coefficients must be equal.  Every input is copied into an allocation of exactly its size, so
// a read one byte past the end is a report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpegdec_plan.h"

using namespace lspdec;

namespace {

struct Result {
    uint32_t status;
    std::vector<int16_t> coef;
};

uint32_t g_flags = 0;                                   // of the bundle: every plan of the run is made with them
ParStats g_stats{};                                     // over the whole run
size_t g_subsequences = 0;

std::vector<Result> run(const std::vector<const std::vector<uint8_t> *> &batch, uint32_t flags)
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
    const int64_t need = plan(ptrs.data(), lens.data(), nullptr, n, 8192, nullptr, flags);
    std::vector<Result> out(n);
    if (need < 0) {
        std::fprintf(stderr, "plan refused the batch (%lld)\n", (long long)need);
        std::exit(2);
    }
    void *blob = std::aligned_alloc(16, (size_t)need);
    if (plan(ptrs.data(), lens.data(), nullptr, n, 8192, blob, flags) != need) {
        std::fprintf(stderr, "plan wrote another size than it announced\n");
        std::exit(2);
    }
    if (flags & kFlagParallel)
        for (uint32_t k = 0; k < header_of(blob)->nsegs; ++k) g_subsequences += subsequences_of(segs_of(blob)[k].begin, segs_of(blob)[k].end);
    for (int i = 0; i < n; ++i) {
        const FileDesc &d = files_of(blob)[i];
        out[i].status = d.status;
        if (d.status != ST_OK) continue;
        out[i].coef.assign((size_t)d.nblk * 64, 0);
        ParStats st{};
        out[i].status = host_coefficients(blob, i, out[i].coef.data(), &st);
        if (st.rounds > g_stats.rounds) g_stats.rounds = st.rounds;
        g_stats.midblock += st.midblock;
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
        std::fprintf(stderr, "usage: jpegdec_par_check <bundle> <seed> <truncated files> <corruptions per file>\n");
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
    std::vector<std::vector<uint8_t>> entries(read32(f));
    for (auto &e : entries) {
        const uint32_t len = read32(f);
        read32(f);                                                             // the expected status: not the yardstick here
        const uint32_t ncoef = read32(f);
        e.resize(len);
        if ((len && std::fread(e.data(), 1, len, f) != len) || std::fseek(f, 2l * ncoef, SEEK_CUR)) {
            std::fprintf(stderr, "bundle ends early\n");
            return 2;
        }
    }
    std::fclose(f);

    int failures = 0;
    size_t ran = 0, counts[4] = {0, 0, 0, 0};
    const auto compare = [&](const char *what, size_t i, size_t detail, const std::vector<const std::vector<uint8_t> *> &batch) {
        const std::vector<Result> serial = run(batch, g_flags), parallel = run(batch, g_flags | kFlagParallel);
        for (size_t j = 0; j < batch.size(); ++j) {
            ++ran;
            ++counts[serial[j].status < 4 ? serial[j].status : 3];
            if (parallel[j].status != serial[j].status || (serial[j].status == ST_OK && parallel[j].coef != serial[j].coef)) {
                std::fprintf(stderr, "%s: file %zu (%zu): parallel status %u, serial status %u%s\n", what, batch.size() > 1 ? j : i, detail, parallel[j].status,
                             serial[j].status, parallel[j].status == serial[j].status ? ", other coefficients" : "");
                ++failures;
            }
        }
    };
    std::vector<const std::vector<uint8_t> *> all;
    for (size_t i = 0; i < entries.size(); ++i) {
        compare("alone", i, 0, {&entries[i]});
        all.push_back(&entries[i]);
    }
    compare("batch", 0, 0, all);
    for (size_t i = 0; i < entries.size() && i < ntrunc; ++i)
        for (size_t len = 0; len < entries[i].size(); ++len) {
            const std::vector<uint8_t> m(entries[i].begin(), entries[i].begin() + len);
            compare("truncation", i, len, {&m});
        }
    for (size_t i = 0; i < entries.size(); ++i)
        for (size_t k = 0; k < ncorrupt && !entries[i].empty(); ++k) {
            lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
            std::vector<uint8_t> m = entries[i];
            const size_t at = (size_t)((lcg >> 33) % m.size());
            m[at] ^= (uint8_t)(1 + ((lcg >> 20) % 255));                       // never the same byte again
            compare("corruption", i, at, {&m});
        }
    std::printf("jpegdec_par_check: %zu files, %zu inputs compared: %zu decoded, %zu unsupported, %zu corrupt, %zu range; %zu subsequences of %u bytes, "
                "most rounds %u, %u entries inside a block; %d failures\n",
                entries.size(), ran, counts[0], counts[1], counts[2], counts[3], g_subsequences, kSubseqBytes, g_stats.rounds, g_stats.midblock, failures);
    return failures ? 1 : 0;
}
