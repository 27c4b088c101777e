// pngdec_plan.h -- the host half of the PNG decoder behind include/lsppng.h: the chunk walker, the planner that lays a batch of files out in one
// descriptor block, and the three stages run on the host over that block with the code the kernels run (pngdec_core.h).  Plain C++ (no HIP, no
// allocation): pngdec.hip wraps it in the C ABI, pngdec_check.cpp builds it with sanitizers and runs it over fixtures, truncations and changes.
#ifndef LSPPNGDEC_PLAN_H
#define LSPPNGDEC_PLAN_H

#include "decode_out.h"
#include "pngdec_core.h"

namespace lsppng {

constexpr uint32_t kMagic = 0x4e50534cu;            // "LSPN"

struct BlobHeader {
    uint32_t magic, nfiles, has_outputs, max_pixels;
    uint64_t bytes, workspace_bytes;
    uint64_t files_off, status_off, data_off;
    uint64_t pad;
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

inline uint32_t crc32_of(const uint8_t *p, size_t n)
{
    struct Table {
        uint32_t v[256];
        Table()
        {
            for (uint32_t i = 0; i < 256; ++i) {
                uint32_t c = i;
                for (int k = 0; k < 8; ++k) c = c & 1 ? 0xedb88320u ^ (c >> 1) : c >> 1;
                v[i] = c;
            }
        }
    };
    static const Table t;
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; ++i) c = t.v[(c ^ p[i]) & 255] ^ (c >> 8);
    return c ^ 0xffffffffu;
}

inline uint32_t be32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
inline bool is_type(const uint8_t *p, const char *name) { return p[0] == (uint8_t)name[0] && p[1] == (uint8_t)name[1] && p[2] == (uint8_t)name[2] && p[3] == (uint8_t)name[3]; }

struct Parsed {
    uint32_t status;
    uint32_t width, height, color_type, depth, channels, ncomp, bpp, rowbytes, npal;
    uint64_t idat_bytes, raw_bytes;
    uint8_t palette[768];
};

// The chunk walker: the status of the container (include/lsppng.h lists what is CORRUPT and what UNSUPPORTED; a CORRUPT container is CORRUPT whatever
// else it holds), the geometry, the palette, and (idat != nullptr) the concatenated IDAT payload, which must have room for idat_bytes of an earlier walk.
inline uint32_t examine(const uint8_t *p, size_t n, uint32_t max_side, Parsed *f, uint8_t *idat = nullptr)
{
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 13, 10, 26, 10};
    *f = Parsed{};
    f->status = ST_CORRUPT;
    if (n < 8) return ST_CORRUPT;
    for (int k = 0; k < 8; ++k)
        if (p[k] != sig[k]) return ST_CORRUPT;
    size_t at = 8;
    bool first = true, seen_plte = false, seen_idat = false, idat_done = false, seen_iend = false, unsupported = false;
    while (at < n) {
        if (n - at < 12) return ST_CORRUPT;
        const uint32_t len = be32(p + at);
        if (len > n - at - 12) return ST_CORRUPT;
        const uint8_t *type = p + at + 4, *data = p + at + 8;
        for (int k = 0; k < 4; ++k)
            if (!((type[k] >= 'A' && type[k] <= 'Z') || (type[k] >= 'a' && type[k] <= 'z'))) return ST_CORRUPT;
        if (crc32_of(type, 4 + (size_t)len) != be32(data + len)) return ST_CORRUPT;
        if (first != is_type(type, "IHDR")) return ST_CORRUPT;                 // not first, or repeated
        if (seen_idat && !is_type(type, "IDAT")) idat_done = true;
        if (first) {
            if (len != 13) return ST_CORRUPT;
            f->width = be32(data);
            f->height = be32(data + 4);
            f->depth = data[8];
            f->color_type = data[9];
            if (f->width == 0 || f->height == 0 || (f->width >> 31) || (f->height >> 31) || data[10] != 0 || data[11] != 0 || data[12] > 1) return ST_CORRUPT;
            const uint32_t d = f->depth, ct = f->color_type;
            const bool pow2 = d == 1 || d == 2 || d == 4 || d == 8 || d == 16;
            const bool legal = pow2 && (ct == 0 || (ct == 3 && d <= 8) || ((ct == 2 || ct == 4 || ct == 6) && d >= 8));
            if (!legal) return ST_CORRUPT;
            f->channels = ct == 0 || ct == 3 ? 1 : ct == 4 ? 2 : ct == 2 ? 3 : 4;
            f->ncomp = ct == 0 || ct == 4 ? 1 : 3;
            unsupported = data[12] == 1 || d == 16 || (ct == 0 && d < 8) || f->width > max_side || f->height > max_side;
            if (!unsupported) {
                f->bpp = f->channels * d >= 8 ? f->channels * d / 8 : 1;
                f->rowbytes = (f->width * f->channels * d + 7) / 8;
                f->raw_bytes = (uint64_t)f->height * (1 + f->rowbytes);
            }
        } else if (is_type(type, "PLTE")) {
            if (f->color_type == 3) {
                if (seen_plte || seen_idat || len % 3 != 0 || len == 0 || len / 3 > (1u << f->depth)) return ST_CORRUPT;
                seen_plte = true;
                f->npal = len / 3;
                for (uint32_t k = 0; k < len; ++k) f->palette[k] = data[k];
            }
        } else if (is_type(type, "IDAT")) {
            if (idat_done || (f->color_type == 3 && !seen_plte)) return ST_CORRUPT;
            seen_idat = true;
            if (idat)
                for (uint32_t k = 0; k < len; ++k) idat[f->idat_bytes + k] = data[k];
            f->idat_bytes += len;
        } else if (is_type(type, "IEND")) {
            if (len != 0) return ST_CORRUPT;
            seen_iend = true;
            at += 12;
            break;
        } else if (is_type(type, "acTL") || is_type(type, "fcTL") || is_type(type, "fdAT") || !(type[0] & 0x20)) {
            unsupported = true;                                                // APNG, or a critical chunk this decoder does not know
        }
        first = false;
        at += 12 + (size_t)len;
    }
    if (!seen_iend || at != n || !seen_idat) return ST_CORRUPT;
    if (unsupported) return f->status = ST_UNSUPPORTED;
    return f->status = ST_OK;
}

// the zlib header (RFC 1950) of the concatenated payload: deflate, a window of at most 32 KiB, the check bits, no preset dictionary
inline uint32_t zlib_header_status(const uint8_t *z, uint64_t n)
{
    if (n < 2) return ST_CORRUPT;
    const uint32_t cmf = z[0], flg = z[1];
    if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 32)) return ST_CORRUPT;
    return ST_OK;
}

// examine() and the zlib header; the payload's first two bytes are found without a buffer
inline uint32_t examine_all(const uint8_t *p, size_t n, uint32_t max_side, Parsed *f)
{
    if (examine(p, n, max_side, f) != ST_OK) return f->status;
    uint8_t z[2] = {0, 0};
    uint64_t got = 0;
    for (size_t at = 8; got < 2 && at + 12 <= n;) {                            // the container has been walked: every chunk lies inside the file
        const uint32_t len = be32(p + at);
        if (is_type(p + at + 4, "IDAT"))
            for (uint32_t k = 0; k < len && got < 2; ++k) z[got++] = p[at + 8 + k];
        at += 12 + (size_t)len;
    }
    return f->status = zlib_header_status(z, f->idat_bytes < got ? f->idat_bytes : got);
}

// Returns the size of the block; writes it when blob is not null.  -1: an output form that does not fit its file; -2: past 4 GiB.
inline int64_t plan(const uint8_t *const *files, const size_t *lens, const OutputDesc *outs, int n, uint32_t max_side, void *blob)
{
    Parsed f;
    uint64_t data = 0;
    for (int i = 0; i < n; ++i)
        if (examine_all(files[i], lens[i], max_side, &f) == ST_OK) data += up(f.idat_bytes, 16);
    BlobHeader h{};
    h.magic = kMagic;
    h.nfiles = (uint32_t)n;
    h.files_off = sizeof(BlobHeader);
    h.status_off = h.files_off + (uint64_t)n * sizeof(FileDesc);
    h.data_off = up(h.status_off + (uint64_t)n * 4, 16);
    h.bytes = h.data_off + data + 16;                                          // the kernel's 16-byte loads stay inside the block
    if (h.bytes >> 32) return -2;
    if (!blob) return (int64_t)h.bytes;

    uint8_t *b = static_cast<uint8_t *>(blob);
    for (uint64_t k = 0; k < h.bytes; ++k) b[k] = 0;
    FileDesc *fd = reinterpret_cast<FileDesc *>(b + h.files_off);
    uint32_t *status = reinterpret_cast<uint32_t *>(b + h.status_off);
    uint64_t at = h.data_off, ws = 0;
    h.has_outputs = 1;                                                         // until a decodable file turns up without one
    for (int i = 0; i < n; ++i) {
        FileDesc &d = fd[i];
        d.status = status[i] = examine_all(files[i], lens[i], max_side, &f);
        if (d.status != ST_OK) continue;
        examine(files[i], lens[i], max_side, &f, b + at);
        d.width = f.width;
        d.height = f.height;
        d.color_type = f.color_type;
        d.depth = f.depth;
        d.channels = f.channels;
        d.ncomp = f.ncomp;
        d.bpp = f.bpp;
        d.rowbytes = f.rowbytes;
        d.raw_bytes = (uint32_t)f.raw_bytes;                                   // <= 8192 * (1 + 4 * 8192)
        d.npal = f.npal;
        for (int k = 0; k < 768; ++k) d.palette[k] = f.palette[k];
        d.idat_begin = at;
        d.idat_end = at + f.idat_bytes;
        at += up(f.idat_bytes, 16);
        d.ws_off = ws;
        ws += up(f.raw_bytes, 256) + 256;
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
    h.workspace_bytes = ws + 256;
    *reinterpret_cast<BlobHeader *>(b) = h;
    return (int64_t)h.bytes;
}

// stage 1 of file i on the host: the status the kernel would leave and (on ST_OK only) the filtered scanlines, raw_bytes of them.  `mem` is the
// working memory the kernel keeps in LDS.
inline uint32_t host_scanlines(const void *blob, int i, InflateMem *mem, uint8_t *out)
{
    const FileDesc &d = files_of(blob)[i];
    if (d.status != ST_OK) return d.status;
    Inflater<HostLanes> inf(HostLanes{}, mem, static_cast<const uint8_t *>(blob), header_of(blob)->bytes, d.idat_begin + 2, d.idat_end, out, d.raw_bytes);
    return inf.run();
}

// stages 2 and 3 on the host, over the scanlines of stage 1 (reconstructed in place): the status, and on ST_OK the pixels [H][W][ncomp]
inline uint32_t host_pixels(const void *blob, int i, uint8_t *scanlines, uint8_t *px)
{
    const FileDesc &d = files_of(blob)[i];
    if (d.status != ST_OK) return d.status;
    const uint32_t st = unfilter_host(d, scanlines);
    if (st != ST_OK) return st;
    for (uint32_t y = 0; y < d.height; ++y)
        for (uint32_t x = 0; x < d.width; ++x) {
            uint32_t v[3];
            pixel_of(d, scanlines + (size_t)y * (1 + d.rowbytes) + 1, x, v);
            lspout::store_pixel(d.ncomp == 3 ? lspout::kFormRgb8 : lspout::kFormGray8, reinterpret_cast<uint64_t>(px), 0, 0, d.ncomp, (size_t)y * d.width + x, v);
        }
    return ST_OK;
}

}  // namespace lsppng
#endif
