// jpeggeom_check.cpp -- the host/device geometry of the JPEG encoder's format handles (jpegenc_geom.h) as a stand-alone program for
// AddressSanitizer and UBSan: it never runs on a device and is never loaded into Python.
//   jpeggeom_check <bundle>
// bundle: "LSGM", uint32 count, then per geometry: int32 w, h, comps, hs, vs, blocks, and int32 [blocks][6] (component, block column, block row,
// dummy, previous block of the component, DC source: what the Python restatement of jccoefct.c's walk gives).  Every geometry goes through
// make_geom + block_of and must give that map; on top of it, what the kernels rely on is checked directly: a DC source is a real block of the
// same MCU at or before the block, the chain of predictions visits every block of a component once, every real block has a sample inside the
// picture, and the coefficient index of every block lies inside the frame's part of the workspace.
#include "jpegenc_geom.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace lspgeom;

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

static void check_geometry(const int32_t *head, const int32_t *want)
{
    const int w = head[0], h = head[1], comps = head[2], hs = head[3], vs = head[4], blocks = head[5];
    const Geom g = make_geom(w, h, comps, hs, vs);
    CHECK(g.nblk == blocks, "%dx%d comps %d (%d, %d): %d blocks, expected %d", w, h, comps, hs, vs, g.nblk, blocks);
    if (g.nblk != blocks) return;
    std::vector<short> coef((size_t)g.nblk * 64, 0);           // what the kernels index with these numbers
    std::vector<int> last(3, -1);
    for (int i = 0; i < g.nblk; ++i) {
        const Block b = block_of(g, i);
        const int32_t got[6] = {b.comp, b.bx, b.by, b.dummy, b.prev, b.dc_src};
        CHECK(std::memcmp(got, want + (size_t)i * 6, sizeof(got)) == 0, "%dx%d comps %d (%d, %d): block %d is (%d %d %d %d %d %d)", w, h, comps, hs, vs, i, got[0],
              got[1], got[2], got[3], got[4], got[5]);
        CHECK(b.comp >= 0 && b.comp < comps && table_of(g, i) == (b.comp ? 1 : 0), "block %d: component %d, table %d", i, b.comp, table_of(g, i));
        CHECK(b.prev == last[b.comp], "block %d: previous block %d, expected %d", i, b.prev, last[b.comp]);
        last[b.comp] = i;
        CHECK(b.dc_src >= i / g.bpm * g.bpm && b.dc_src <= i && (b.dc_src == i) == !b.dummy, "block %d: DC source %d", i, b.dc_src);
        CHECK(!block_of(g, b.dc_src).dummy, "block %d: its DC source %d is a dummy block", i, b.dc_src);
        coef[(size_t)b.dc_src * 64] += 1;
        if (!b.dummy) {
            const int cw = b.comp ? ceil_div(w, hs) : w, ch = b.comp ? ceil_div(h, vs) : h;
            CHECK(b.bx * 8 < cw && b.by * 8 < ch, "block %d: real, at (%d, %d) outside its %dx%d plane", i, b.bx, b.by, cw, ch);
        }
        for (int ibl : {g.bpm, 2 * g.bpm, 3 * g.bpm, g.nblk}) {
            const int pg = pred_block(b, i, ibl);
            CHECK(pg == (b.prev >= 0 && b.prev / ibl == i / ibl ? b.prev : -1), "block %d: predicted from %d in intervals of %d blocks", i, pg, ibl);
        }
    }
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: jpeggeom_check <bundle>\n");
        return 2;
    }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    char magic[4];
    uint32_t count = 0;
    if (std::fread(magic, 1, 4, f) != 4 || std::memcmp(magic, "LSGM", 4) != 0 || std::fread(&count, 4, 1, f) != 1) {
        std::fprintf(stderr, "not a geometry bundle\n");
        return 2;
    }
    size_t done = 0, blocks = 0;
    for (uint32_t k = 0; k < count; ++k) {
        int32_t head[6];
        if (std::fread(head, 4, 6, f) != 6 || head[5] < 1 || head[5] > (1 << 20)) {
            std::fprintf(stderr, "truncated bundle at geometry %u\n", k);
            return 2;
        }
        std::vector<int32_t> want((size_t)head[5] * 6);
        if (std::fread(want.data(), 4, want.size(), f) != want.size()) {
            std::fprintf(stderr, "truncated bundle at geometry %u\n", k);
            return 2;
        }
        check_geometry(head, want.data());
        blocks += (size_t)head[5];
        ++done;
    }
    std::fclose(f);
    std::printf("jpeggeom_check: %zu geometries, %zu blocks; %d failures\n", done, blocks, failures);
    return failures ? 1 : 0;
}
