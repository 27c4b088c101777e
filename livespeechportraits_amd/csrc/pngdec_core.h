// pngdec_core.h -- the host/device half of the PNG decoder (include/lsppng.h): inflate of one file's zlib stream with its Adler-32, the unfilter
// arithmetic of the PNG specification and the pixel fetch.  Plain C++ with no allocation and no library calls.  The inflater is written once over a
// "lanes" policy: on the device the 64 lanes of one wave run it (pngdec.hip WaveLanes), on the host the lanes are loops (HostLanes), so the stream the
// stand-alone checker (pngdec_check.cpp, built with sanitizers) has walked is the stream the kernel reads, within the same bounds.
//
// The symbol walk is lane-uniform: every lane holds the same bit reader and the same positions.  The lanes do what has width: staging the stream
// into an LDS ring in 16-byte loads, filling the first-level decode table of a Huffman code, the match copy (lane i writes
// out[p + i] = out[p - dist + (i mod dist)], 64 bytes per step, overlapping matches included), the flush of the 32 KiB window to memory in 16-byte
// stores and the Adler-32 sums of the flushed bytes.
//
// Bounds, whatever the file says: input bytes are taken below the stream's end only (Inflater::refill), staging loads stay inside the descriptor
// block (Inflater::ensure), output stops at the expected size (Inflater::room), a distance is checked against the bytes produced, window and ring
// indices are masked, table indices are bounded by the table sizes (code lengths are < 16, symbols < 288 / 32).  Every step of the walk consumes at
// least one input bit or ends the walk, so its length is bounded by the stream's.
#ifndef LSPPNGDEC_CORE_H
#define LSPPNGDEC_CORE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define LSPPNG_HD __host__ __device__
#else
#define LSPPNG_HD
#endif

namespace lsppng {

// status words (include/lsppng.h LSPPNG_DEC_STATUS_*)
enum : uint32_t { ST_OK = 0, ST_UNSUPPORTED = 1, ST_CORRUPT = 2 };

constexpr uint32_t kLanes = 64;
constexpr uint32_t kWindow = 32768;                  // deflate's largest distance: the output ring
constexpr uint32_t kInRing = 4096;                   // the staged stream
constexpr uint32_t kStageAhead = 1024;               // bytes staged ahead of the reader: one round of 64 lanes x 16 bytes
constexpr uint32_t kFlush = 1024;                    // bytes per flush of the window: 64 lanes x 16 bytes
constexpr int kFastBits = 10;                        // first-level table: codes of up to 10 bits in one lookup
static_assert(kInRing >= 2 * kStageAhead + 1024 && (kInRing & (kInRing - 1)) == 0 && (kWindow & (kWindow - 1)) == 0, "ring sizes");
static_assert(kFlush == kLanes * 16 && kStageAhead == kLanes * 16, "one 16-byte access per lane and round");

// ---- one file of a batch, as the kernels see it
struct FileDesc {
    uint32_t status;           // what the planner found (ST_*): a file that is not ST_OK is skipped by every launch
    uint32_t width, height;
    uint32_t color_type, depth;
    uint32_t channels;         // samples per pixel in the file: 1 (grey, palette), 2 (grey + alpha), 3, 4
    uint32_t ncomp;            // components of the output: 1 or 3
    uint32_t bpp;              // max(1, channels * depth / 8): the distance of the unfilter's left neighbour
    uint32_t rowbytes;         // ceil(width * channels * depth / 8)
    uint32_t raw_bytes;        // height * (1 + rowbytes): what the zlib stream must inflate to
    uint32_t npal;             // PLTE entries (type 3)
    uint32_t form;
    uint64_t idat_begin, idat_end;   // the concatenated IDAT payload inside the block: zlib header, deflate data, Adler-32
    uint64_t ws_off;           // of the file's scanlines inside the workspace (256-byte aligned)
    uint64_t out_ptr, table_ptr;
    int64_t plane_stride;
    uint8_t palette[768];
};
static_assert(sizeof(FileDesc) % 16 == 0, "FileDesc is part of the descriptor block's layout");

// ---- a canonical Huffman code in decode form: codes per length and symbols in code order (the walk of zlib's contrib/puff), and a first-level
// table indexed by the next kFastBits bits, (symbol << 4) | length, 0 where the code there is longer or absent
struct HuffCode {
    uint16_t count[16];
    uint16_t symbol[288];
    uint16_t fast[1 << kFastBits];
};

// the working memory of one inflate: LDS on the device
struct InflateMem {
    alignas(16) uint8_t window[kWindow];
    alignas(16) uint8_t inring[kInRing];
    HuffCode lit, dist;
    uint16_t lens[320];        // the code lengths of the block being set up (288 + 32 for the fixed codes)
    uint16_t code_of[320];     // their canonical codes, for the first-level fill
    int32_t verdict;           // of the serial part of a table build, for all lanes
};

LSPPNG_HD inline void copy16(void *dst, const void *src)
{
    __builtin_memcpy(__builtin_assume_aligned(dst, 16), __builtin_assume_aligned(src, 16), 16);
}

// the lanes as loops: the host twin
struct HostLanes {
    template <class F> LSPPNG_HD void each(F f) const
    {
        for (uint32_t l = 0; l < kLanes; ++l) f(l);
    }
    template <class F> LSPPNG_HD void one(F f) const { f(); }
    template <class F> LSPPNG_HD uint64_t sum(F f) const
    {
        uint64_t s = 0;
        for (uint32_t l = 0; l < kLanes; ++l) s += f(l);
        return s;
    }
    LSPPNG_HD void sync() const {}
};

enum CodeKind { CODE_LENGTHS, CODE_LITLEN, CODE_DIST };

template <class X> struct Inflater {
    X x;
    InflateMem *m;
    const uint8_t *blob;       // the descriptor block; staging loads stay below blob_bytes
    uint64_t blob_bytes;
    uint64_t pos, end;         // the next byte of the stream to enter the bit buffer; the stream's end
    uint64_t filled;           // staged up to here (a multiple of 16)
    uint64_t bitbuf;
    uint32_t bitcnt;
    bool bad;                  // a take() past the stream's end
    uint8_t *out;              // the file's scanlines in memory
    uint32_t produced, flushed, limit;
    uint32_t a1, a2;           // Adler-32 of the flushed bytes

    LSPPNG_HD Inflater(X lanes, InflateMem *mem, const uint8_t *b, uint64_t nbytes, uint64_t begin, uint64_t stop, uint8_t *dst, uint32_t expect)
        : x(lanes), m(mem), blob(b), blob_bytes(nbytes), pos(begin), end(stop), filled(begin & ~15ull), bitbuf(0), bitcnt(0), bad(false), out(dst),
          produced(0), flushed(0), limit(expect), a1(1), a2(0)
    {
    }

    // stage the stream: afterwards every byte of [pos, min(end, pos + kStageAhead)) is in the ring
    LSPPNG_HD void ensure()
    {
        uint64_t want = pos + kStageAhead;
        if (want > end) want = end;
        if (filled >= want) return;
        x.sync();
        while (filled < want) {
            const uint64_t base = filled;
            x.each([&](uint32_t l) {
                const uint64_t off = base + (uint64_t)l * 16;
                if (off + 16 <= blob_bytes) copy16(m->inring + (off & (kInRing - 1)), blob + off);
            });
            filled += kStageAhead;
        }
        x.sync();
    }
    LSPPNG_HD void refill()
    {
        while (bitcnt <= 56 && pos < end) {
            bitbuf |= (uint64_t)m->inring[pos & (kInRing - 1)] << bitcnt;
            bitcnt += 8;
            ++pos;
        }
    }
    // at least 57 bits in the buffer, or all that is left of the stream
    LSPPNG_HD void need()
    {
        ensure();
        refill();
    }
    LSPPNG_HD uint32_t take(uint32_t n)
    {
        if (bitcnt < n) {
            bad = true;
            return 0;
        }
        const uint32_t v = (uint32_t)(bitbuf & ((1ull << n) - 1));
        bitbuf >>= n;
        bitcnt -= n;
        return v;
    }
    // the symbol of the code that starts at the next bit; -1: a pattern in no code, or the stream ends inside it
    LSPPNG_HD int decode(const HuffCode &h)
    {
        const uint32_t e = h.fast[bitbuf & ((1u << kFastBits) - 1)];
        if (e) {
            if (bitcnt < (e & 15u)) return -1;
            bitbuf >>= (e & 15u);
            bitcnt -= (e & 15u);
            return (int)(e >> 4);
        }
        int code = 0, first = 0, index = 0;
        for (uint32_t len = 1; len <= 15; ++len) {
            code |= (int)((bitbuf >> (len - 1)) & 1);
            const int count = h.count[len];
            if (code - count < first) {
                if (bitcnt < len) return -1;
                bitbuf >>= len;
                bitcnt -= len;
                return h.symbol[index + (code - first)];
            }
            index += count;
            first += count;
            first <<= 1;
            code <<= 1;
        }
        return -1;
    }

    // A code from m->lens[at .. at + n): the serial part by one lane, the first-level table by all.  false: over-subscribed, or incomplete where
    // that is not admitted (the code-length code always; a literal/length or distance code unless it is a single code of one bit; a distance code
    // may also be empty: RFC 1951 3.2.7, a block of literals only).
    LSPPNG_HD bool build(HuffCode &h, uint32_t at, uint32_t n, CodeKind kind)
    {
        x.sync();
        InflateMem *mm = m;
        x.one([&]() {
            uint16_t offs[16], next[16];
            for (int l = 0; l < 16; ++l) h.count[l] = 0;
            for (uint32_t s = 0; s < n; ++s) ++h.count[mm->lens[at + s] & 15];
            int left = 1;
            bool over = false;
            for (int l = 1; l <= 15; ++l) {
                left <<= 1;
                left -= h.count[l];
                if (left < 0) {
                    over = true;
                    break;
                }
            }
            bool ok = !over;
            if (ok && left > 0) {
                const bool single = h.count[1] == 1 && h.count[0] == n - 1;
                const bool empty = h.count[0] == n;
                ok = kind != CODE_LENGTHS && (single || (empty && kind == CODE_DIST));
            }
            offs[1] = 0;
            next[1] = 0;
            for (int l = 1; l < 15; ++l) {
                offs[l + 1] = (uint16_t)(offs[l] + h.count[l]);
                next[l + 1] = (uint16_t)((next[l] + h.count[l]) << 1);
            }
            if (ok)
                for (uint32_t s = 0; s < n; ++s) {
                    const uint32_t l = mm->lens[at + s] & 15;
                    if (l) {
                        h.symbol[offs[l]++] = (uint16_t)s;
                        mm->code_of[at + s] = next[l]++;
                    }
                }
            mm->verdict = ok ? 1 : 0;
        });
        x.each([&](uint32_t lane) {
            for (uint32_t i = lane; i < (1u << kFastBits); i += kLanes) h.fast[i] = 0;
        });
        x.sync();
        if (!m->verdict) return false;
        x.each([&](uint32_t lane) {
            for (uint32_t s = lane; s < n; s += kLanes) {
                const uint32_t l = mm->lens[at + s] & 15;
                if (l == 0 || l > (uint32_t)kFastBits) continue;
                uint32_t code = mm->code_of[at + s], rev = 0;
                for (uint32_t k = 0; k < l; ++k) rev |= ((code >> k) & 1u) << (l - 1 - k);
                for (uint32_t i = rev; i < (1u << kFastBits); i += 1u << l) h.fast[i] = (uint16_t)((s << 4) | l);
            }
        });
        x.sync();
        return true;
    }

    LSPPNG_HD bool room(uint32_t n) const { return n <= limit - produced; }

    // the window's oldest kFlush bytes (or what is left) to memory, 16 bytes per lane, and into the Adler-32
    LSPPNG_HD void flush_some()
    {
        const uint32_t n = produced - flushed < kFlush ? produced - flushed : kFlush, at = flushed;
        x.sync();
        InflateMem *mm = m;
        uint8_t *dst = out;
        const uint64_t sums = x.sum([&](uint32_t l) -> uint64_t {
            const uint32_t o = l * 16;
            if (o >= n) return 0;
            const uint8_t *src = mm->window + ((at + o) & (kWindow - 1));
            const uint32_t cnt = n - o < 16 ? n - o : 16;
            if (cnt == 16)
                copy16(dst + at + o, src);
            else
                for (uint32_t j = 0; j < cnt; ++j) dst[at + o + j] = src[j];
            uint32_t s = 0, t = 0;
            for (uint32_t j = 0; j < cnt; ++j) {
                s += src[j];
                t += (n - (o + j)) * src[j];
            }
            return (uint64_t)s | ((uint64_t)t << 32);
        });
        const uint32_t s = (uint32_t)sums, t = (uint32_t)(sums >> 32);      // s <= 1024 * 255, t <= 255 * 1024 * 1025 / 2: both sums fit 32 bits
        a2 = (uint32_t)(((uint64_t)a2 + (uint64_t)n * a1 + t) % 65521u);
        a1 = (a1 + s) % 65521u;
        flushed += n;
    }
    LSPPNG_HD void flush_full()
    {
        while (produced - flushed >= kFlush) flush_some();
    }

    LSPPNG_HD bool match(uint32_t len, uint32_t dist)
    {
        if (dist > produced || !room(len)) return false;
        InflateMem *mm = m;
        x.sync();
        while (len) {
            const uint32_t n = len < kLanes ? len : kLanes, p = produced;
            x.each([&](uint32_t l) {
                if (l < n) {
                    const uint32_t back = dist >= kLanes ? l : l % dist;
                    const uint8_t v = mm->window[(p - dist + back) & (kWindow - 1)];
                    mm->window[(p + l) & (kWindow - 1)] = v;
                }
            });
            x.sync();
            produced += n;
            len -= n;
        }
        return true;
    }

    LSPPNG_HD bool stored()
    {
        take(bitcnt & 7);
        const uint32_t len = take(16), nlen = take(16);
        if (bad || (len ^ 0xffffu) != nlen) return false;
        pos -= bitcnt >> 3;                                                    // whole bytes go back to the stream
        bitbuf = 0;
        bitcnt = 0;
        if (!room(len) || len > end - pos) return false;
        InflateMem *mm = m;
        uint32_t left = len;
        while (left) {
            const uint32_t n = left < kLanes ? left : kLanes, p = produced;
            ensure();
            const uint64_t from = pos;
            x.each([&](uint32_t l) {
                if (l < n) mm->window[(p + l) & (kWindow - 1)] = mm->inring[(from + l) & (kInRing - 1)];
            });
            produced += n;
            pos += n;
            left -= n;
            flush_full();
        }
        return true;
    }

    LSPPNG_HD bool fixed_codes()
    {
        InflateMem *mm = m;
        x.sync();
        x.each([&](uint32_t lane) {
            for (uint32_t s = lane; s < 320; s += kLanes) mm->lens[s] = (uint16_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
        });
        return build(m->lit, 0, 288, CODE_LITLEN) && build(m->dist, 288, 32, CODE_DIST);
    }

    LSPPNG_HD bool dynamic_codes()
    {
        const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        InflateMem *mm = m;
        const uint32_t nlen = take(5) + 257, ndist = take(5) + 1, ncode = take(4) + 4;
        if (bad || nlen > 286 || ndist > 30) return false;
        x.sync();
        x.one([&]() {
            for (int k = 0; k < 19; ++k) mm->lens[k] = 0;
        });
        for (uint32_t k = 0; k < ncode; ++k) {
            need();
            const uint32_t v = take(3);
            const uint32_t slot = order[k];
            x.one([&]() { mm->lens[slot] = (uint16_t)v; });
        }
        if (bad || !build(m->lit, 0, 19, CODE_LENGTHS)) return false;
        uint32_t i = 0, last = 0;
        while (i < nlen + ndist) {
            need();
            const int sym = decode(m->lit);
            if (sym < 0) return false;
            uint32_t value = 0, rep = 1;
            if (sym < 16) {
                value = last = (uint32_t)sym;
            } else if (sym == 16) {
                if (i == 0) return false;
                value = last;
                rep = 3 + take(2);
            } else if (sym == 17) {
                last = 0;
                rep = 3 + take(3);
            } else {
                last = 0;
                rep = 11 + take(7);
            }
            if (bad || i + rep > nlen + ndist) return false;
            const uint32_t from = i;
            x.one([&]() {
                for (uint32_t k = 0; k < rep; ++k) mm->lens[from + k] = (uint16_t)value;
            });
            i += rep;
        }
        x.sync();
        if (m->lens[256] == 0) return false;
        return build(m->lit, 0, nlen, CODE_LITLEN) && build(m->dist, nlen, ndist, CODE_DIST);
    }

    LSPPNG_HD bool coded_block()
    {
        const uint16_t lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
        const uint8_t lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
        const uint16_t dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
        const uint8_t dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
        InflateMem *mm = m;
        for (;;) {
            need();
            int sym = decode(m->lit);
            if (sym < 0) return false;
            if (sym < 256) {
                if (!room(1)) return false;
                const uint32_t p = produced;
                x.one([&]() { mm->window[p & (kWindow - 1)] = (uint8_t)sym; });
                ++produced;
            } else if (sym == 256) {
                return true;
            } else {
                sym -= 257;
                if (sym >= 29) return false;
                const uint32_t len = lbase[sym] + take(lext[sym]);
                const int ds = decode(m->dist);
                if (ds < 0 || ds >= 30) return false;
                const uint32_t dist = dbase[ds] + take(dext[ds]);
                if (bad || !match(len, dist)) return false;
            }
            flush_full();
        }
    }

    // the whole stream behind the zlib header: ST_OK when it inflates to exactly `limit` bytes, its Adler-32 matches and nothing is left over
    LSPPNG_HD uint32_t run()
    {
        for (;;) {
            need();
            const uint32_t final = take(1), type = take(2);
            if (bad) return ST_CORRUPT;
            bool ok;
            if (type == 0)
                ok = stored();
            else if (type == 1)
                ok = fixed_codes() && coded_block();
            else if (type == 2)
                ok = dynamic_codes() && coded_block();
            else
                ok = false;
            if (!ok) return ST_CORRUPT;
            if (final) break;
        }
        while (flushed < produced) flush_some();
        if (produced != limit) return ST_CORRUPT;
        need();
        take(bitcnt & 7);
        uint32_t adler = 0;
        for (int k = 0; k < 4; ++k) adler = (adler << 8) | take(8);
        if (bad || adler != ((a2 << 16) | a1)) return ST_CORRUPT;
        refill();
        if (bitcnt != 0 || pos != end) return ST_CORRUPT;
        return ST_OK;
    }
};

// ---- unfilter: the PNG specification's reconstruction.  a = the byte bpp to the left (0 before the row's start), b = the byte above (0 above the
// first row), c = the byte above a; all of them reconstructed bytes.
LSPPNG_HD inline uint32_t paeth(uint32_t a, uint32_t b, uint32_t c)
{
    const int p = (int)a + (int)b - (int)c;
    const int pa = p > (int)a ? p - (int)a : (int)a - p, pb = p > (int)b ? p - (int)b : (int)b - p, pc = p > (int)c ? p - (int)c : (int)c - p;
    return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;                        // ties in the order a, b, c
}

LSPPNG_HD inline uint32_t reconstruct(uint32_t filter, uint32_t raw, uint32_t a, uint32_t b, uint32_t c)
{
    const uint32_t pred = filter == 0 ? 0u : filter == 1 ? a : filter == 2 ? b : filter == 3 ? (a + b) >> 1 : paeth(a, b, c);     // Average: floor of the 9-bit sum
    return (raw + pred) & 255u;
}

// byte `at` of a reconstructed row of a palette file holds an index at or past the PLTE entry count (the padding bits of the row's last byte are
// no pixels)
LSPPNG_HD inline bool index_bad(const FileDesc &f, uint32_t at, uint32_t byte)
{
    if (f.color_type != 3 || f.npal >= (1u << f.depth)) return false;
    const uint32_t per = 8 / f.depth;
    for (uint32_t k = 0; k < per; ++k) {
        if (at * per + k >= f.width) break;
        if (((byte >> (8 - f.depth * (k + 1))) & ((1u << f.depth) - 1)) >= f.npal) return true;
    }
    return false;
}

// the pixel x of a reconstructed row (behind its filter byte): palette lookup, alpha dropped
LSPPNG_HD inline void pixel_of(const FileDesc &f, const uint8_t *row, uint32_t x, uint32_t px[3])
{
    if (f.color_type == 3) {
        const uint32_t bit = x * f.depth, byte = row[bit >> 3];
        const uint32_t idx = (byte >> (8 - f.depth - (bit & 7))) & ((1u << f.depth) - 1);
        px[0] = f.palette[idx * 3];
        px[1] = f.palette[idx * 3 + 1];
        px[2] = f.palette[idx * 3 + 2];
    } else if (f.ncomp == 3) {
        px[0] = row[x * f.channels];
        px[1] = row[x * f.channels + 1];
        px[2] = row[x * f.channels + 2];
    } else {
        px[0] = px[1] = px[2] = row[x * f.channels];
    }
}

// stage 2 on the host: rows top to bottom, in place.  ST_CORRUPT: a filter byte above 4, or a palette index past the PLTE entries.
inline uint32_t unfilter_host(const FileDesc &f, uint8_t *raw)
{
    const uint32_t stride = 1 + f.rowbytes;
    for (uint32_t y = 0; y < f.height; ++y) {
        uint8_t *row = raw + (size_t)y * stride + 1;
        const uint8_t *up = y ? row - stride : nullptr;
        const uint32_t ft = row[-1];
        if (ft > 4) return ST_CORRUPT;
        for (uint32_t i = 0; i < f.rowbytes; ++i) {
            const uint32_t a = i >= f.bpp ? row[i - f.bpp] : 0, b = up ? up[i] : 0, c = up && i >= f.bpp ? up[i - f.bpp] : 0;
            row[i] = (uint8_t)reconstruct(ft, row[i], a, b, c);
        }
    }
    for (uint32_t y = 0; y < f.height; ++y)
        for (uint32_t i = 0; i < f.rowbytes; ++i)
            if (index_bad(f, i, raw[(size_t)y * stride + 1 + i])) return ST_CORRUPT;
    return ST_OK;
}

}  // namespace lsppng
#endif
