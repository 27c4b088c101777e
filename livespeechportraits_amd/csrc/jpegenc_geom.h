// jpegenc_geom.h -- the host/device geometry of the JPEG encoder's format handles (include/lspjpeg.h lspjpeg_create_format): frames of any size
// in 4:4:4, 4:2:2, 4:2:0 or grey, with libjpeg's MCU grid and its dummy blocks.  Plain C++ with no allocation and no library calls: the kernels of
// jpeg.hip, lspjpeg_create_format, lspjpeg_host_block_map and the stand-alone checker (jpeggeom_check.cpp, built with sanitizers) run the SAME
// text.
//
// With luma factors (hs, vs) = (2, 2) 4:2:0, (2, 1) 4:2:2, (1, 1) 4:4:4:
//   * colour: ceil(W / 8hs) x ceil(H / 8vs) MCUs; an MCU is its hs * vs luma blocks, row-major, then Cb, then Cr (jccoefct.c compress_data);
//   * grey: a non-interleaved scan, one block per MCU, ceil(W / 8) x ceil(H / 8) of them, no dummy blocks;
//   * a luma block whose column >= ceil(W / 8) or row >= ceil(H / 8) is dummy: it is not transformed, its AC coefficients are 0 and its quantised DC
//     is that of the block before it in the MCU -- which may be dummy too, so the value comes from the last real block before it (`dc_src`).  The
//     first luma block of an MCU and the chroma blocks are never dummy.
#ifndef LSPJPEGENC_GEOM_H
#define LSPJPEGENC_GEOM_H

#include <stdint.h>

#ifdef __HIPCC__
#define LSPGEOM_HD __host__ __device__
#else
#define LSPGEOM_HD
#endif

namespace lspgeom {

struct Geom {
    int w, h, comps, hs, vs;
    int mcux, mcuy;                                  // the MCU grid
    int lbx, lby;                                    // real luma blocks per row and column: ceil(W / 8), ceil(H / 8)
    int nlum, bpm;                                   // luma blocks and blocks per MCU
    int nmcu, nblk;                                  // per frame, dummy blocks included
};

struct Block {
    int comp, bx, by;                                // component (0 Y, 1 Cb, 2 Cr), block column and row in the component's plane
    int dummy;
    int prev;                                        // the previous block of the component in the frame, -1 for the first
    int dc_src;                                      // the block whose quantised DC this one codes: itself unless dummy
};

LSPGEOM_HD inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// (hs, vs) must be (1, 1) for comps == 1; the caller has checked the values
LSPGEOM_HD inline Geom make_geom(int w, int h, int comps, int hs, int vs)
{
    Geom g;
    g.w = w;
    g.h = h;
    g.comps = comps;
    g.hs = hs;
    g.vs = vs;
    g.lbx = ceil_div(w, 8);
    g.lby = ceil_div(h, 8);
    g.mcux = ceil_div(w, 8 * hs);
    g.mcuy = ceil_div(h, 8 * vs);
    g.nlum = hs * vs;
    g.bpm = comps == 3 ? g.nlum + 2 : 1;
    g.nmcu = g.mcux * g.mcuy;
    g.nblk = g.nmcu * g.bpm;
    return g;
}

// Huffman / quantisation table id of block i: 0 luma, 1 chroma
LSPGEOM_HD inline int table_of(const Geom &g, int i) { return g.comps == 3 && i % g.bpm >= g.nlum ? 1 : 0; }

LSPGEOM_HD inline bool luma_dummy(const Geom &g, int mx, int my, int j) { return mx * g.hs + j % g.hs >= g.lbx || my * g.vs + j / g.hs >= g.lby; }

LSPGEOM_HD inline Block block_of(const Geom &g, int i)
{
    Block b;
    const int m = i / g.bpm, j = i % g.bpm;
    const int mx = m % g.mcux, my = m / g.mcux;
    b.dummy = 0;
    b.dc_src = i;
    if (j < g.nlum) {                                // (grey: nlum == bpm == 1)
        b.comp = 0;
        b.bx = mx * g.hs + j % g.hs;
        b.by = my * g.vs + j / g.hs;
        b.prev = j > 0 ? i - 1 : m > 0 ? i - g.bpm + g.nlum - 1 : -1;
        if (luma_dummy(g, mx, my, j)) {
            b.dummy = 1;
            int k = j - 1;                           // block 0 of an MCU is real: the loop ends there at the latest
            while (k > 0 && luma_dummy(g, mx, my, k)) --k;
            b.dc_src = i - j + k;
        }
    } else {
        b.comp = j - g.nlum + 1;
        b.bx = mx;
        b.by = my;
        b.prev = m > 0 ? i - g.bpm : -1;
    }
    return b;
}

// the block whose DC predicts block i's under restart intervals of ibl blocks (whole MCUs): b.prev inside i's interval, -1 at its start
LSPGEOM_HD inline int pred_block(const Block &b, int i, int ibl) { return b.prev >= i / ibl * ibl ? b.prev : -1; }

}  // namespace lspgeom
#endif
