// jpegdec_plan.h -- the host half of the JPEG decoder behind include/lspjpegdec.h: the planner that lays a batch of files out in one descriptor
// block, and stage 1 run on the host over that block.  Plain C++ (no HIP, no allocation): jpegdec.hip wraps it in the C ABI, jpegdec_check.cpp
// builds it with sanitizers and runs it over fixtures, truncations and corruptions; jpegdec_par_check.cpp does the same for the parallel route.
#ifndef LSPJPEGDEC_PLAN_H
#define LSPJPEGDEC_PLAN_H

#include "decode_out.h"
#include "jpegdec_core.h"

namespace lspdec {

constexpr uint32_t kMagic = 0x4a44534cu;            // "LSDJ"

struct BlobHeader {
    uint32_t magic, nfiles, nsegs, has_outputs;
    uint32_t max_blocks, max_pixels;
    uint32_t parallel;                              // kFlagParallel: stage 1 of the baseline files decodes inside a restart interval in parallel; 0 without the flag
    uint32_t pad1;
    uint64_t total_blocks, bytes, workspace_bytes;
    uint64_t files_off, segs_off, tables_off, status_off, data_off;
    uint64_t planes_ws_off;                         // the plane area inside the workspace (the coefficients come first)
    uint64_t pad2;
    // progressive files (kFlagProgressive): their scans, the restart intervals of those, and the table snapshots; all empty without the flag
    uint32_t nprog, nscans, npsegs, nptabs;
    uint64_t scans_off, psegs_off, ptables_off, pad3;
};
static_assert(sizeof(BlobHeader) % 16 == 0, "the areas behind the header stay 16-byte aligned");

using lspout::OutputDesc;
using lspout::up;

inline const BlobHeader *header_of(const void *blob)
{
    const BlobHeader *h = static_cast<const BlobHeader *>(blob);
    return h && h->magic == kMagic ? h : nullptr;
}
inline const FileDesc *files_of(const void *blob) { return reinterpret_cast<const FileDesc *>(static_cast<const char *>(blob) + header_of(blob)->files_off); }
inline const SegDesc *segs_of(const void *blob) { return reinterpret_cast<const SegDesc *>(static_cast<const char *>(blob) + header_of(blob)->segs_off); }
inline const HuffTable *tables_of(const void *blob) { return reinterpret_cast<const HuffTable *>(static_cast<const char *>(blob) + header_of(blob)->tables_off); }
inline const ScanDesc *scans_of(const void *blob) { return reinterpret_cast<const ScanDesc *>(static_cast<const char *>(blob) + header_of(blob)->scans_off); }
inline const SegDesc *psegs_of(const void *blob) { return reinterpret_cast<const SegDesc *>(static_cast<const char *>(blob) + header_of(blob)->psegs_off); }
inline const HuffTable *ptables_of(const void *blob) { return reinterpret_cast<const HuffTable *>(static_cast<const char *>(blob) + header_of(blob)->ptables_off); }

// parser + scan walker: the status of a whole file, its segment count and where its entropy-coded data ends
inline uint32_t examine(const uint8_t *p, size_t n, uint32_t max_side, Parsed *f, uint32_t *nseg, uint64_t *scan_end)
{
    *nseg = 0;
    *scan_end = 0;
    if (parse_markers(p, n, max_side, f) != ST_OK) return f->status;
    // the Huffman tables the scan uses must describe prefix codes (jdhuff.c jpeg_make_d_derived_tbl refuses the others)
    for (uint32_t c = 0; c < f->ncomp; ++c)
        for (int cls = 0; cls < 2; ++cls) {
            const int id = cls ? f->ac_sel[c] : f->dc_sel[c];
            if (!f->huff_seen[cls][id]) continue;
            HuffTable t;
            if (!build_table(f->huff_bits[cls][id], f->huff_vals[cls][id], &t)) return f->status = ST_CORRUPT;
        }
    const uint32_t st = walk_scan(p, n, *f, 0, 0, nullptr, 0, nseg, scan_end);
    if (st != ST_OK) {
        *nseg = 0;
        return f->status = st;
    }
    return ST_OK;
}

// examine() under flags: a file the baseline parser calls UNSUPPORTED goes to the progressive walker when kFlagProgressive is set.  *progressive
// says which of f / pf holds the answer.
inline uint32_t examine_flags(const uint8_t *p, size_t n, uint32_t max_side, uint32_t flags, Parsed *f, uint32_t *nseg, uint64_t *scan_end, ProgFile *pf,
                              bool *progressive)
{
    *progressive = false;
    const uint32_t st = examine(p, n, max_side, f, nseg, scan_end);
    if (st != ST_UNSUPPORTED || !(flags & kFlagProgressive)) return st;
    *progressive = true;
    return walk_progressive(p, n, max_side, pf, 0, 0, nullptr, 0, nullptr, 0, nullptr, 0);
}

// Returns the size of the block; writes it when blob is not null.  -1: an output form that does not fit its file; -2: past 4 GiB / 2^32 segments.
inline int64_t plan(const uint8_t *const *files, const size_t *lens, const OutputDesc *outs, int n, uint32_t max_side, void *blob, uint32_t flags = 0)
{
    uint64_t nsegs = 0, data = 0, nscans = 0, npsegs = 0, nptabs = 0;
    uint32_t nprog = 0;
    Parsed f;
    ProgFile pf;
    bool prog;
    for (int i = 0; i < n; ++i) {
        uint32_t ns;
        uint64_t e;
        if (examine_flags(files[i], lens[i], max_side, flags, &f, &ns, &e, &pf, &prog) != ST_OK) continue;
        if (prog) {
            ++nprog;
            nscans += pf.nscan;
            npsegs += pf.nseg;
            nptabs += pf.ntab;
            data += pf.data_end - pf.data_begin;
        } else {
            nsegs += ns;
            data += e - f.scan_begin;
        }
    }
    BlobHeader h{};
    h.magic = kMagic;
    h.nfiles = (uint32_t)n;
    h.parallel = flags & kFlagParallel ? 1u : 0u;
    h.files_off = sizeof(BlobHeader);
    h.segs_off = up(h.files_off + (uint64_t)n * sizeof(FileDesc), 16);
    h.tables_off = up(h.segs_off + nsegs * sizeof(SegDesc), 16);
    h.status_off = h.tables_off + (uint64_t)n * 4 * sizeof(HuffTable);
    h.scans_off = up(h.status_off + (uint64_t)n * 4, 16);
    h.psegs_off = up(h.scans_off + nscans * sizeof(ScanDesc), 16);
    h.ptables_off = up(h.psegs_off + npsegs * sizeof(SegDesc), 16);
    h.data_off = up(h.ptables_off + nptabs * sizeof(HuffTable), 16);
    h.bytes = up(h.data_off + data, 16) + 16;                                  // the kernel's 16-byte loads stay inside the block
    if (h.bytes >> 32 || nsegs >> 32 || npsegs >> 32) return -2;
    h.nsegs = (uint32_t)nsegs;
    h.nprog = nprog;
    h.nscans = (uint32_t)nscans;
    h.npsegs = (uint32_t)npsegs;
    h.nptabs = (uint32_t)nptabs;
    if (!blob) return (int64_t)h.bytes;

    char *b = static_cast<char *>(blob);
    for (uint64_t k = 0; k < h.bytes; ++k) b[k] = 0;
    FileDesc *fd = reinterpret_cast<FileDesc *>(b + h.files_off);
    SegDesc *sd = reinterpret_cast<SegDesc *>(b + h.segs_off);
    HuffTable *ht = reinterpret_cast<HuffTable *>(b + h.tables_off);
    uint32_t *status = reinterpret_cast<uint32_t *>(b + h.status_off);
    ScanDesc *scd = reinterpret_cast<ScanDesc *>(b + h.scans_off);
    SegDesc *psd = reinterpret_cast<SegDesc *>(b + h.psegs_off);
    HuffTable *pht = reinterpret_cast<HuffTable *>(b + h.ptables_off);
    uint64_t at = h.data_off, planes = 0;
    uint32_t seg = 0, scan = 0, pseg = 0, ptab = 0;
    h.has_outputs = 1;                                                         // until a decodable file turns up without one
    for (int i = 0; i < n; ++i) {
        FileDesc &d = fd[i];
        uint32_t ns;
        uint64_t e;
        d.status = status[i] = examine_flags(files[i], lens[i], max_side, flags, &f, &ns, &e, &pf, &prog);
        d.table0 = 4 * (uint32_t)i;
        d.seg0 = seg;
        d.scan0 = scan;
        if (d.status != ST_OK) continue;
        if (prog) {                                                            // the fields both kinds of file share, out of the progressive walker's record
            f = Parsed{};
            f.width = pf.width;
            f.height = pf.height;
            f.ncomp = pf.ncomp;
            f.hs = pf.hs;
            f.vs = pf.vs;
            f.restart = pf.restart0;
            for (int c = 0; c < 4; ++c) {
                f.comp_q[c] = pf.comp_q[c];
                for (int k = 0; k < 64; ++k) f.q[c][k] = pf.q[c][k];
            }
            ns = 0;
        }
        d.width = f.width;
        d.height = f.height;
        d.ncomp = f.ncomp;
        d.hs = f.hs;
        d.vs = f.vs;
        d.mcux = (f.width + 8 * f.hs - 1) / (8 * f.hs);
        d.mcuy = (f.height + 8 * f.vs - 1) / (8 * f.vs);
        d.bpm = f.ncomp == 1 ? 1 : f.hs * f.vs + 2;
        d.nblk = d.mcux * d.mcuy * d.bpm;
        d.restart = f.restart;
        d.nseg = ns;
        d.coef_off = h.total_blocks;
        for (uint32_t c = 0; c < f.ncomp; ++c) {
            d.dc_sel[c] = f.dc_sel[c];
            d.ac_sel[c] = f.ac_sel[c];
            d.plane_w[c] = d.mcux * 8 * (c == 0 ? f.hs : 1);
            d.plane_h[c] = d.mcuy * 8 * (c == 0 ? f.vs : 1);
            d.plane_off[c] = planes;
            planes += up((uint64_t)d.plane_w[c] * d.plane_h[c], 16);
            for (int k = 0; k < 64; ++k) d.q[c][k] = f.q[f.comp_q[c]][k];
        }
        if (prog) {
            // the bytes from the first scan's data up to the EOI marker (the markers between the scans travel along), and the scans, their restart
            // intervals and their tables with offsets into the block
            const uint64_t nbytes = pf.data_end - pf.data_begin;
            for (uint64_t k = 0; k < nbytes; ++k) b[at + k] = (char)files[i][pf.data_begin + k];
            const uint64_t begin = pf.data_begin;
            ProgFile again;
            walk_progressive(files[i], lens[i], max_side, &again, at - begin, (uint32_t)i, scd + scan, h.nscans - scan, psd + pseg, h.npsegs - pseg, pht + ptab,
                             h.nptabs - ptab);
            d.progressive = 1;
            d.nscan = again.nscan;
            for (uint32_t s = 0; s < again.nscan; ++s) {                       // the walker counted from this file's first entry
                scd[scan + s].seg0 += pseg;
                scd[scan + s].table0 += ptab;
            }
            scan += again.nscan;
            pseg += again.nseg;
            ptab += again.ntab;
            at += nbytes;
        } else {
            for (int id = 0; id < 2; ++id)
                for (int cls = 0; cls < 2; ++cls) {
                    uint8_t bits[17], vals[256];
                    if (f.huff_seen[cls][id]) {
                        for (int l = 0; l < 17; ++l) bits[l] = f.huff_bits[cls][id][l];
                        for (int k = 0; k < 256; ++k) vals[k] = f.huff_vals[cls][id][k];
                    } else {
                        default_huffman(cls, id, bits, vals);
                    }
                    if (!build_table(bits, vals, &ht[d.table0 + 2 * id + cls]))    // an unused table of the file may be no prefix code: an empty table
                        for (int l = 0; l < 17; ++l) ht[d.table0 + 2 * id + cls].maxcode[l] = -1;
                }
            // the entropy-coded bytes, and the segments with offsets into the block
            const uint64_t nbytes = e - f.scan_begin;
            for (uint64_t k = 0; k < nbytes; ++k) b[at + k] = (char)files[i][f.scan_begin + k];
            uint32_t got;
            uint64_t end;
            walk_scan(files[i], lens[i], f, at - f.scan_begin, (uint32_t)i, sd + seg, ns, &got, &end);
            seg += ns;
            at += nbytes;
        }
        h.total_blocks += d.nblk;
        if (d.nblk > h.max_blocks) h.max_blocks = d.nblk;
        if (d.width * d.height > h.max_pixels) h.max_pixels = d.width * d.height;
        if (outs && outs[i].ptr) {
            const OutputDesc &o = outs[i];
            if (!lspout::output_fits(o, f.ncomp, (int64_t)d.width * d.height)) return -1;
            d.out_ptr = o.ptr;
            d.table_ptr = o.table;
            d.plane_stride = o.plane_stride;
            d.form = o.form;
        } else {
            h.has_outputs = 0;
        }
    }
    h.planes_ws_off = up(h.total_blocks * 64 * sizeof(int16_t), 256);
    h.workspace_bytes = up(h.planes_ws_off + planes, 256) + 256;
    *reinterpret_cast<BlobHeader *>(b) = h;
    return (int64_t)h.bytes;
}

struct MemSrc {
    const uint8_t *base;
    uint8_t at(uint64_t pos) const { return base[pos]; }
};

// stage 1 of a progressive file on the host: its scans in file order over the same coefficients, with the procedures the kernel runs
inline uint32_t host_progressive(const void *blob, const FileDesc &d, int16_t *out)
{
    uint8_t comp_of[kMaxBlocksPerMcu];
    int bpm;
    block_components(d.ncomp, d.hs, d.vs, comp_of, &bpm);
    const MemSrc src{static_cast<const uint8_t *>(blob)};
    for (uint32_t s = 0; s < d.nscan; ++s) {
        const ScanDesc &sc = scans_of(blob)[d.scan0 + s];
        const HuffTable *tabs = ptables_of(blob) + sc.table0;
        const int bpu = sc.ncomp > 1 ? bpm : 1;
        ScanState st{};
        for (uint32_t g = 0; g < sc.nseg; ++g) {
            const SegDesc &sg = psegs_of(blob)[sc.seg0 + g];
            BitReader<MemSrc> br(src, sg.begin, sg.end);
            st = ScanState{};                                                  // predictions and the end-of-band run start again at every RSTn
            for (uint32_t u = 0; u < sg.nmcu; ++u) {
                const uint32_t at = prog_block_index(d, sc, (sg.mcu0 + u) * bpu);
                if (at + bpu > d.nblk) return ST_CORRUPT;
                const uint32_t r = prog_units<NaturalOrder>(br, sc, tabs, comp_of, bpu, st, out + (uint64_t)at * 64, 1);
                if (r != ST_OK) return r;
            }
            if (!br.drained()) return ST_CORRUPT;
        }
        if (st.eobrun) return ST_CORRUPT;                                      // a run that reaches past the scan's last block
    }
    return ST_OK;
}

// what the parallel route did, for checks: the most rounds the fixed point of any chunk took, and how many true entry states stood inside a block
struct ParStats {
    uint32_t rounds, midblock;
};

// One restart interval on the parallel route (kFlagParallel), as jpegdec_entropy_parallel runs it with the lanes as loops: per chunk of kParLanes
// subsequences the fixed point over the entry states, the exclusive scan over blocks started and DC sums, and the write pass from the true
// entries (those with no dead exit in front of them).  `out` is the file's coefficient array, zeroed by the caller.  Returns the status of the earliest failure in stream order.
inline uint32_t host_parallel_segment(const void *blob, const FileDesc &d, const SegDesc &sg, int16_t *out, ParStats *stats)
{
    const MemSrc src{static_cast<const uint8_t *>(blob)};
    const ParGeom g = par_geom(d);
    const HuffTable *tables = tables_of(blob) + d.table0;
    const uint32_t total = sg.nmcu * g.bpm, nsub = subsequences_of(sg.begin, sg.end);
    int16_t *coef = out + (uint64_t)sg.mcu0 * g.bpm * 64;
    ParState entry[kParLanes], guess[kParLanes], carry{sg.begin * 8, 0, 0, 0};
    ParResult res[kParLanes];
    bool changed[kParLanes];
    uint32_t blocks = 0;
    int pred[3] = {0, 0, 0};
    for (uint32_t c0 = 0; c0 < nsub; c0 += kParLanes) {
        const uint32_t nl = nsub - c0 < kParLanes ? nsub - c0 : kParLanes;
        const uint64_t cb = sg.begin + (uint64_t)c0 * kSubseqBytes;
        const auto limit = [&](uint32_t lane) {
            const uint64_t e = cb + (uint64_t)(lane + 1) * kSubseqBytes;
            return e < sg.end ? e : sg.end;
        };
        for (uint32_t lane = 0; lane < nl; ++lane) {
            guess[lane] = guess_state(src, sg.begin, sg.end, cb + (uint64_t)lane * kSubseqBytes);
            entry[lane] = lane ? guess[lane] : carry;
            changed[lane] = true;
        }
        for (uint32_t rounds = 1;; ++rounds) {
            for (uint32_t lane = 0; lane < nl; ++lane)
                if (changed[lane]) decode_subsequence<false>(src, sg.begin, sg.end, limit(lane), entry[lane], tables, g, 0, 0, nullptr, nullptr, false, &res[lane]);
            bool any = false;
            changed[0] = false;
            for (uint32_t lane = 1; lane < nl; ++lane) {
                const ParState want = res[lane - 1].exit.dead ? guess[lane] : res[lane - 1].exit;     // behind a dead exit the lane's own guess stands again
                changed[lane] = !same_state(want, entry[lane]);
                if (changed[lane]) {
                    entry[lane] = want;
                    any = true;
                }
            }
            if (!any) {
                if (stats && rounds > stats->rounds) stats->rounds = rounds;
                break;
            }
        }
        bool valid = true;
        for (uint32_t lane = 0; lane < nl; ++lane) {
            const ParState &e = entry[lane];
            valid = valid && !e.dead && !(lane && res[lane - 1].exit.dead);     // true entries reach as far as the exits before them are alive
            if (valid && (e.k == 0 || blocks > 0)) {
                if (stats && e.k) ++stats->midblock;
                ParResult w;
                decode_subsequence<true>(src, sg.begin, sg.end, limit(lane), e, tables, g, e.k ? blocks - 1 : blocks, total, pred, coef, c0 + lane + 1 == nsub, &w);
                if (w.status != ST_OK) return w.status;                        // the lanes are visited in stream order: the first failure
                if (w.done) return ST_OK;                                      // what stands behind the interval's last block is no state of the file
            }
            blocks += res[lane].blocks;
            for (int c = 0; c < 3; ++c) pred[c] += res[lane].dc[c];
        }
        carry = res[nl - 1].exit;
    }
    return ST_CORRUPT;                                                         // unreachable: a true entry with a dead exit fails or finishes in the write pass, and the last lane reports data that ends early
}

// stage 1 of file i on the host: the status the kernel would leave, and (on ST_OK only) the coefficients
inline uint32_t host_coefficients(const void *blob, int i, int16_t *out, ParStats *stats = nullptr)
{
    const FileDesc &d = files_of(blob)[i];
    if (d.status != ST_OK) return d.status;
    uint8_t comp_of[kMaxBlocksPerMcu];
    int bpm;
    block_components(d.ncomp, d.hs, d.vs, comp_of, &bpm);
    const MemSrc src{static_cast<const uint8_t *>(blob)};
    for (uint64_t k = 0; k < (uint64_t)d.nblk * 64; ++k) out[k] = 0;
    if (d.progressive) return host_progressive(blob, d, out);
    for (uint32_t s = 0; s < d.nseg; ++s) {
        const SegDesc &sg = segs_of(blob)[d.seg0 + s];
        if (header_of(blob)->parallel) {
            const uint32_t st = host_parallel_segment(blob, d, sg, out, stats);
            if (st != ST_OK) return st;
            continue;
        }
        BitReader<MemSrc> br(src, sg.begin, sg.end);
        int pred[3] = {0, 0, 0};
        for (uint32_t m = 0; m < sg.nmcu; ++m) {
            const uint32_t st = decode_mcu(br, tables_of(blob) + d.table0, d.dc_sel, d.ac_sel, comp_of, bpm, pred, out + (uint64_t)(sg.mcu0 + m) * bpm * 64);
            if (st != ST_OK) return st;
        }
        if (!br.drained()) return ST_CORRUPT;
    }
    return ST_OK;
}

}  // namespace lspdec
#endif
