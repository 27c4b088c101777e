// resize_check.cpp -- the host half of the resampler (resize_core.h: Pillow's coefficient builder and the plan layout) as plain C++ with its own
// main, built under AddressSanitizer and UBSan (make check-resize).  Plans every geometry given as "in_w in_h out_w out_h filter" -- five
// numbers per plan, on the command line or on stdin -- and prints one line per plan: the geometry, then either
//   ok <bytes> <digest> <path_h> <path_v> <row0> <rows>     (digest: rszcore::plan_digest, FNV-1a over ksize, bounds and coefficients)
// or
//   refused <reason>
// Host code only: it never runs on a device and is never loaded into Python.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "resize_core.h"

static int plan_one(const long g[5]) {
    std::printf("%ld %ld %ld %ld %ld ", g[0], g[1], g[2], g[3], g[4]);
    for (int i = 0; i < 5; ++i)
        if (g[i] < -1000000 || g[i] > 1000000) {
            std::printf("refused a number out of range\n");
            return 0;
        }
    const int in_w = (int)g[0], in_h = (int)g[1], out_w = (int)g[2], out_h = (int)g[3], filter = (int)g[4];
    if (const char *why = rszcore::check_geometry(in_w, in_h, out_w, out_h, filter)) {
        std::printf("refused %s\n", why);
        return 0;
    }
    const uint64_t need = rszcore::plan_bytes(in_w, in_h, out_w, out_h, filter);
    if (need > rszcore::kMaxPlanBytes) {
        std::printf("refused a block of %" PRIu64 " bytes\n", need);
        return 0;
    }
    std::vector<unsigned char> blob((size_t)need);           // exactly the bytes asked for: one byte past them is ASan's to catch
    const uint64_t wrote = rszcore::build_plan(in_w, in_h, out_w, out_h, filter, blob.data());
    if (wrote != need || !rszcore::valid_plan(blob.data())) {
        std::printf("BROKEN wrote %" PRIu64 " of %" PRIu64 "\n", wrote, need);
        return 1;
    }
    rszcore::PlanHeader h;
    std::memcpy(&h, blob.data(), sizeof(h));
    // what the kernels lean on: every window inside its axis and inside ksize, the row window inside the image
    const int axes[2][4] = {{h.need_h, out_w, in_w, h.ksize_h}, {1, out_h, in_h, h.ksize_v}};
    const uint32_t at[2] = {h.bounds_h, h.bounds_v};
    for (int a = 0; a < 2; ++a) {
        if (!axes[a][0]) continue;
        const int32_t *b = (const int32_t *)(blob.data() + at[a]);
        for (int i = 0; i < axes[a][1]; ++i)
            if (b[2 * i] < 0 || b[2 * i + 1] < 0 || b[2 * i + 1] > axes[a][3] || b[2 * i] + b[2 * i + 1] > axes[a][2]) {
                std::printf("BROKEN window %d of axis %d\n", i, a);
                return 1;
            }
        for (int i = 1; i < axes[a][1]; ++i)                    // the horizontal kernel takes a tile's window from its first and last output
            if (b[2 * i] < b[2 * i - 2] || b[2 * i] + b[2 * i + 1] < b[2 * i - 2] + b[2 * i - 1]) {
                std::printf("BROKEN order at window %d of axis %d\n", i, a);
                return 1;
            }
    }
    if (h.row0 < 0 || h.rows < 1 || h.row0 + h.rows > in_h) {
        std::printf("BROKEN row window\n");
        return 1;
    }
    std::printf("ok %" PRIu64 " %016" PRIx64 " %d %d %d %d\n", need, rszcore::plan_digest(blob.data()), h.path_h, h.need_v || !h.need_h ? h.path_v : 0, h.row0, h.rows);
    return 0;
}

int main(int argc, char **argv) {
    std::vector<long> v;
    if (argc > 1) {
        for (int i = 1; i < argc; ++i) v.push_back(std::strtol(argv[i], nullptr, 10));
    } else {
        long x;
        while (std::scanf("%ld", &x) == 1) v.push_back(x);
    }
    if (v.empty() || v.size() % 5) {
        std::fprintf(stderr, "usage: resize_check in_w in_h out_w out_h filter [...]   (or the same numbers on stdin)\n");
        return 2;
    }
    int bad = 0;
    for (size_t i = 0; i < v.size(); i += 5) bad |= plan_one(&v[i]);
    return bad;
}
