// pngenc_check.cpp -- the host half of the PNG encoder (pngenc_core.h) as a stand-alone program for AddressSanitizer and UBSan (make check-pngenc).
// Host code only: it is never run on a device and never loaded into Python.
//
//   pngenc_check <bundle>
//
// The bundle (written by tests/test_png_encode_cpu.py) is "LSPE", a uint32 count, then per case five uint32 (width, height, components, level,
// filter with 5 for the heuristic) and the height * width * components pixels.  Every case is encoded with the code the kernels run (the lanes as
// loops), twice: the two files must be equal and no larger than the capacity.  The file is then decoded by the host half of the decoder
// (pngdec_plan.h: every CRC, the Adler-32, the stream ending exactly) and the pixels must be the case's.  Every buffer is an allocation of exactly
// its size, so a read or a write one byte past an end is a report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "pngdec_plan.h"
#include "pngenc_core.h"

namespace {

uint32_t read32(FILE *f)
{
    uint8_t b[4];
    if (std::fread(b, 1, 4, f) != 4) {
        std::fprintf(stderr, "bundle ends early\n");
        std::exit(2);
    }
    return b[0] | (b[1] << 8) | (b[2] << 16) | ((uint32_t)b[3] << 24);
}

struct File {
    uint8_t *bytes;
    size_t size;
    uint32_t forms[3];
};

File encode(const lsppngenc::Geom &g, const uint8_t *px)
{
    using namespace lsppngenc;
    std::unique_ptr<ChunkMem> mem(new ChunkMem());
    uint8_t *lines = static_cast<uint8_t *>(std::malloc(g.raw));
    uint8_t *slots = static_cast<uint8_t *>(std::malloc((size_t)g.nchunks * kSlotBytes));
    ChunkRec *recs = static_cast<ChunkRec *>(std::malloc(g.nchunks * sizeof(ChunkRec)));
    File f{static_cast<uint8_t *>(std::malloc(kHeaderBytes + g.cap)), 0, {0, 0, 0}};
    f.size = encode_host(g, px, *mem, lines, slots, recs, f.bytes, f.forms, nullptr);
    std::free(lines);
    std::free(slots);
    std::free(recs);
    return f;
}

// the decoder's host half over one file: the status, and the pixels on status 0
uint32_t decode(const uint8_t *file, size_t size, std::vector<uint8_t> &px)
{
    using namespace lsppng;
    uint8_t *copy = static_cast<uint8_t *>(std::malloc(size));
    std::memcpy(copy, file, size);
    const uint8_t *ptrs[1] = {copy};
    const size_t lens[1] = {size};
    const int64_t need = plan(ptrs, lens, nullptr, 1, 8192, nullptr);
    if (need < 0) {
        std::free(copy);
        return 99;
    }
    void *blob = std::aligned_alloc(16, ((size_t)need + 15) & ~(size_t)15);
    plan(ptrs, lens, nullptr, 1, 8192, blob);
    const FileDesc &d = files_of(blob)[0];
    uint32_t st = d.status;
    if (st == ST_OK) {
        std::unique_ptr<InflateMem> mem(new InflateMem());
        uint8_t *lines = static_cast<uint8_t *>(std::malloc(d.raw_bytes));
        st = host_scanlines(blob, 0, mem.get(), lines);
        if (st == ST_OK) {
            px.resize((size_t)d.width * d.height * d.ncomp);
            st = host_pixels(blob, 0, lines, px.data());
        }
        std::free(lines);
    }
    std::free(blob);
    std::free(copy);
    return st;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: pngenc_check <bundle>\n");
        return 2;
    }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    char magic[4];
    if (std::fread(magic, 1, 4, f) != 4 || std::memcmp(magic, "LSPE", 4)) {
        std::fprintf(stderr, "not a bundle\n");
        return 2;
    }
    const uint32_t count = read32(f);
    int failures = 0;
    uint32_t forms[3] = {0, 0, 0};
    size_t in_bytes = 0, out_bytes = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t w = read32(f), h = read32(f), comps = read32(f), level = read32(f), filter = read32(f);
        lsppngenc::Geom g{};
        if (!lsppngenc::make_geom((int)w, (int)h, (int)comps, (int)level, filter == lsppngenc::kFilterHeuristic ? -1 : (int)filter, 8192, &g)) {
            std::fprintf(stderr, "case %u: geometry refused\n", i);
            return 2;
        }
        const size_t npx = (size_t)w * h * comps;
        uint8_t *px = static_cast<uint8_t *>(std::malloc(npx));
        if (std::fread(px, 1, npx, f) != npx) {
            std::fprintf(stderr, "bundle ends early\n");
            return 2;
        }
        const File a = encode(g, px), b = encode(g, px);
        if (a.size != b.size || std::memcmp(a.bytes, b.bytes, a.size)) {
            std::fprintf(stderr, "case %u: two encodes differ\n", i);
            ++failures;
        }
        if (a.size > lsppngenc::kHeaderBytes + g.cap || (level == 0 && a.size != lsppngenc::kHeaderBytes + g.cap)) {
            std::fprintf(stderr, "case %u: %zu bytes against a capacity of %llu\n", i, a.size, (unsigned long long)g.cap);
            ++failures;
        }
        std::vector<uint8_t> back;
        const uint32_t st = decode(a.bytes, a.size, back);
        if (st != 0 || back.size() != npx || std::memcmp(back.data(), px, npx)) {
            std::fprintf(stderr, "case %u (%u x %u x %u, level %u, filter %u): status %u%s\n", i, w, h, comps, level, filter, st, st ? "" : ", other pixels");
            ++failures;
        }
        for (int k = 0; k < 3; ++k) forms[k] += a.forms[k];
        in_bytes += npx;
        out_bytes += a.size;
        std::free(a.bytes);
        std::free(b.bytes);
        std::free(px);
    }
    std::fclose(f);
    std::printf("pngenc_check: %u cases, %zu -> %zu bytes, chunks stored / fixed / dynamic %u / %u / %u; %d failures\n", count, in_bytes, out_bytes, forms[0],
                forms[1], forms[2], failures);
    return failures ? 1 : 0;
}
