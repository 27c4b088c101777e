// pngenc_core.h -- the host/device half of the PNG encoder (include/lsppngenc.h): the five filters and the row heuristic, the matcher, the greedy
// token choice, the length-limited code builder, the block choice, the bit writer and the pieces of CRC-32 and Adler-32 with their combination.
// Plain C++ with no allocation and no library calls.  The chunk encoder is written once over a "lanes" policy, as pngdec_core.h's inflater is: on
// the device the kThreads threads of one workgroup run it (pngenc.hip BlockLanes), on the host the lanes are loops (HostLanes), so the file the
// stand-alone checker (pngenc_check.cpp, built with sanitizers) has made is the file the kernels make, bit for bit and within the same bounds.
//
// One chunk = kChunk bytes of the filtered scanline stream (the last one of a frame may be shorter).  Its payload is ONE deflate block (stored, fixed
// or dynamic, the cheapest in bytes; ties to the lower form) and an empty stored block, which ends it on a byte (zlib's sync flush; BFINAL is set in
// the last chunk's).  Phases, a sync between any two:
//   hash     every position's 3-byte hash; the positions of the up to kWindow bytes before the chunk enter the table: table[h] = the LAST position
//            with hash h (a maximum, so the order of arrival decides nothing);
//   look up  kStep positions per step read table[h] and older[h], then enter the table themselves (the same maximum) and move what they read from
//            table[h] to older[h] (every lane with that hash read the same value).  A step sees the steps before it only, so the steps are a chain;
//            they touch LDS only and leave two candidates per position;
//   match    every position, all at once: its two candidates and kNear fixed distances (the bytes just before it, and one row above with its two
//            neighbours) are extended; the longest match wins, of equal ones the nearest.  A lane walks kSeg consecutive positions and carries
//            what each fixed distance matched at the position before, so the bytes of a long match are compared once;
//   choose   greedy: from position 0, a match of 3 or more is taken whole, else a literal.  Thread t resolves, backwards over its kSeg positions, where
//            the walk leaves its segment from each of them; one lane then hops over the segments (kThreads hops at most) and every thread walks its own;
//   codes    histograms (integer adds), a rank sort, the two-queue Huffman merge, the length limit by the counting method of JPEG's Annex K.3 (as
//            jpegenc_core.h's), canonical codes, the run-length form of the dynamic header; the three forms' sizes, computed, not tried;
//   write    the bits of every thread's tokens at the offsets a prefix sum gives, ORed into a zeroed buffer (an OR: again no order);
//   sums     CRC-32 of the IDAT chunk and the Adler-32 sums of the chunk's input, in kThreads pieces each, combined in GF(2) / modulo 65521.
// Bounds: a match never reads at or past the chunk's end nor before position 0 of the frame; a distance is at most kWindow; the payload of a Huffman
// form is taken only when it is smaller than the stored one, kChunk + kStoredOverhead bytes, which is the size of the staging buffer.
#ifndef LSPPNGENC_CORE_H
#define LSPPNGENC_CORE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define LSPPE_HD __host__ __device__
#else
#define LSPPE_HD
#endif

namespace lsppngenc {

constexpr uint32_t kChunk = 16384;                   // PNGENC_CHUNK: bytes of the filtered stream per independently compressed piece
constexpr uint32_t kWindow = 32768;                  // deflate's largest distance: how far a match reaches back into the chunks before
constexpr uint32_t kThreads = 256;                   // lanes of one chunk
constexpr uint32_t kSeg = kChunk / kThreads;         // positions one lane owns in the token choice
constexpr uint32_t kHashBits = 12;
constexpr uint32_t kStep = 64;                       // positions per look-up step: what a step cannot see is the step itself
constexpr uint32_t kNear = 11;                       // fixed distances tried at every position
constexpr uint32_t kMinMatch = 3, kMaxMatch = 258;
constexpr uint32_t kFarDist = 4096;                  // a match of 3 from further away costs more than three literals (zlib's TOO_FAR)
constexpr uint32_t kStoredOverhead = 10;             // 1 + 4: header, LEN, NLEN of the stored block; 1 + 4: the empty stored block behind every chunk
constexpr uint32_t kIdatOverhead = 12;               // length, "IDAT", CRC
constexpr uint32_t kTailBytes = 2 + 16 + 12;         // zlib header (in the first IDAT); an IDAT of its own with the Adler-32; IEND
constexpr uint32_t kOutWords = (kChunk + kStoredOverhead + 3) / 4 + 1;
constexpr uint32_t kSlotBytes = kOutWords * 4;       // of a chunk's payload in the workspace
constexpr uint32_t kHeaderBytes = 33;                // signature + IHDR
constexpr uint32_t kNone = 0xffff;
constexpr uint32_t kFilterHeuristic = 5;
constexpr uint32_t kAdlerMod = 65521;
constexpr uint32_t kCrcPoly = 0xedb88320u;
enum : uint32_t { FORM_STORED = 0, FORM_FIXED = 1, FORM_DYNAMIC = 2 };
static_assert(kSeg * kThreads == kChunk && kChunk <= 32768 && kChunk + kWindow < 65536, "positions and exits are kept in 16 bits");

struct Geom {
    uint32_t width, height, comps;
    uint32_t stride;           // 1 + width * comps: one filtered scanline
    uint32_t raw;              // height * stride: the filtered stream
    uint32_t nchunks;          // ceil(raw / kChunk)
    uint32_t level;            // 0: stored blocks only; 1: matcher + Huffman coding
    uint32_t filter;           // 0..4, or kFilterHeuristic
    uint64_t cap;              // capacity_bound()
};

// what one chunk leaves for the scan and the gather
struct ChunkRec {
    uint32_t payload;          // bytes of its deflate blocks
    uint32_t crc;              // of its IDAT chunk
    uint32_t s1, s2;           // Adler-32 pieces of its input, modulo 65521: the sum of the bytes, and of (end - i) * byte[i]
};

// ---- sizes ------------------------------------------------------------------------------------------------------------------------------
LSPPE_HD inline uint32_t chunk_count(uint64_t raw) { return (uint32_t)((raw + kChunk - 1) / kChunk); }
// per frame behind the 33 header bytes: every chunk stored (its bytes + kStoredOverhead) in an IDAT of its own (kIdatOverhead), and kTailBytes.
// It is the exact size of a level 0 file's part, and nothing the encoder writes can pass it: a Huffman form is taken only when it is smaller.
LSPPE_HD inline uint64_t capacity_bound(uint64_t raw)
{
    return raw + (uint64_t)chunk_count(raw) * (kStoredOverhead + kIdatOverhead) + kTailBytes;
}

// ---- filters (PNG specification, section 9) -----------------------------------------------------------------------------------------------------
LSPPE_HD inline uint32_t paeth(uint32_t a, uint32_t b, uint32_t c)
{
    const int p = (int)a + (int)b - (int)c;
    const int pa = p > (int)a ? p - (int)a : (int)a - p, pb = p > (int)b ? p - (int)b : (int)b - p, pc = p > (int)c ? p - (int)c : (int)c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
LSPPE_HD inline uint32_t filter_byte(uint32_t type, uint32_t x, uint32_t a, uint32_t b, uint32_t c)
{
    const uint32_t pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : paeth(a, b, c);
    return (x - pred) & 255u;
}
// the heuristic's measure: the filtered byte read as signed
LSPPE_HD inline uint32_t sad(uint32_t v) { return v < 128 ? v : 256 - v; }

// byte j of row y filtered with `type`; px = the frame's pixels, rowbytes = width * comps, bpp = comps
LSPPE_HD inline uint32_t filtered_at(const uint8_t *px, uint32_t rowbytes, uint32_t bpp, uint32_t y, uint32_t j, uint32_t type)
{
    const uint8_t *row = px + (size_t)y * rowbytes;
    const uint32_t x = row[j], a = j >= bpp ? row[j - bpp] : 0, b = y ? row[j - (size_t)rowbytes] : 0, c = (y && j >= bpp) ? row[j - (size_t)rowbytes - bpp] : 0;
    return filter_byte(type, x, a, b, c);
}
// lane `lane` of `nlanes`: its share of the five sums of row y
LSPPE_HD inline void filter_sums(const uint8_t *px, uint32_t rowbytes, uint32_t bpp, uint32_t y, uint32_t lane, uint32_t nlanes, uint32_t sums[5])
{
    for (int f = 0; f < 5; ++f) sums[f] = 0;
    const uint8_t *row = px + (size_t)y * rowbytes;
    for (uint32_t j = lane; j < rowbytes; j += nlanes) {
        const uint32_t x = row[j], a = j >= bpp ? row[j - bpp] : 0, b = y ? row[j - (size_t)rowbytes] : 0, c = (y && j >= bpp) ? row[j - (size_t)rowbytes - bpp] : 0;
        for (uint32_t f = 0; f < 5; ++f) sums[f] += sad(filter_byte(f, x, a, b, c));
    }
}
// the smallest sum, ties to the lowest filter number
LSPPE_HD inline uint32_t filter_choice(const uint32_t sums[5])
{
    uint32_t best = 0;
    for (uint32_t f = 1; f < 5; ++f)
        if (sums[f] < sums[best]) best = f;
    return best;
}
// lane's share of the filtered scanline: the filter byte and the row
LSPPE_HD inline void filter_write(const uint8_t *px, uint32_t rowbytes, uint32_t bpp, uint32_t y, uint32_t type, uint32_t lane, uint32_t nlanes, uint8_t *line)
{
    if (lane == 0) line[0] = (uint8_t)type;
    for (uint32_t j = lane; j < rowbytes; j += nlanes) line[1 + j] = (uint8_t)filtered_at(px, rowbytes, bpp, y, j, type);
}

// ---- CRC-32 in pieces: x^k modulo the polynomial, reflected (bit 31 is x^0) ------------------------------------------------------------------------
LSPPE_HD inline uint32_t gf_mul(uint32_t a, uint32_t b)          // a must not be 0
{
    uint32_t m = 0x80000000u, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) break;
        }
        m >>= 1;
        b = (b & 1) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}
LSPPE_HD inline uint32_t gf_xpow_bytes(uint32_t nbytes)          // x^(8 * nbytes)
{
    uint32_t p = 0x80000000u, sq = 0x00800000u;
    for (uint32_t n = nbytes; n; n >>= 1) {
        if (n & 1) p = gf_mul(sq, p);
        sq = gf_mul(sq, sq);
    }
    return p;
}
// one byte through the register (no initial value, no final complement: linear, so pieces combine as raw(A || B) = raw(A) * x^(8 |B|) + raw(B),
// and zeros in front of a piece change nothing)
LSPPE_HD inline uint32_t crc_step(uint32_t r, uint32_t byte)
{
    r ^= byte;
    for (int k = 0; k < 8; ++k) r = (r & 1) ? (r >> 1) ^ kCrcPoly : r >> 1;
    return r;
}
inline uint32_t crc_bytes(const uint8_t *p, size_t n)             // the usual CRC-32, for the header and the tail
{
    uint32_t r = 0xffffffffu;
    for (size_t i = 0; i < n; ++i) r = crc_step(r, p[i]);
    return ~r;
}
LSPPE_HD inline void put_be32(uint8_t *p, uint32_t v)
{
    p[0] = (uint8_t)(v >> 24);
    p[1] = (uint8_t)(v >> 16);
    p[2] = (uint8_t)(v >> 8);
    p[3] = (uint8_t)v;
}

// ---- deflate's symbols -------------------------------------------------------------------------------------------------------------------------
LSPPE_HD inline uint32_t log2_floor(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }
// length 3..258 -> index 0..28 of symbol 257 + index, extra bits and their value
LSPPE_HD inline uint32_t length_symbol(uint32_t len, uint32_t *ebits, uint32_t *eval)
{
    const uint32_t l = len - 3;
    if (l < 8 || len == 258) {
        *ebits = 0;
        *eval = 0;
        return len == 258 ? 28 : l;
    }
    const uint32_t e = log2_floor(l) - 2;
    *ebits = e;
    *eval = l & ((1u << e) - 1);
    return 4 * e + 4 + ((l >> e) & 3);
}
LSPPE_HD inline uint32_t length_extra_bits(uint32_t index) { return (index < 8 || index == 28) ? 0 : (index - 4) >> 2; }
// distance 1..32768 -> symbol 0..29
LSPPE_HD inline uint32_t dist_symbol(uint32_t dist, uint32_t *ebits, uint32_t *eval)
{
    const uint32_t d = dist - 1;
    if (d < 4) {
        *ebits = 0;
        *eval = 0;
        return d;
    }
    const uint32_t lg = log2_floor(d), e = lg - 1;
    *ebits = e;
    *eval = d & ((1u << e) - 1);
    return 2 * lg + ((d >> e) & 1);
}
LSPPE_HD inline uint32_t dist_extra_bits(uint32_t sym) { return sym < 4 ? 0 : (sym >> 1) - 1; }
LSPPE_HD inline uint32_t fixed_length(uint32_t sym) { return sym < 144 ? 8 : sym < 256 ? 9 : sym < 280 ? 7 : 8; }

// ---- code lengths ------------------------------------------------------------------------------------------------------------------------------
struct CodeScratch {
    uint16_t order[288];       // the used symbols, by rising (frequency, symbol)
    uint32_t weight[576];
    uint16_t parent[576];
    uint8_t depth[576];
    uint16_t bits[64];         // symbols per length (the sum of the frequencies is below 2^32: no tree is deeper than 46)
};

// the place of symbol s among the used ones; any lane may do any symbol
LSPPE_HD inline void rank_symbol(const uint32_t *freq, uint32_t n, uint32_t s, uint16_t *order)
{
    if (!freq[s]) return;
    uint32_t rank = 0;
    for (uint32_t j = 0; j < n; ++j) rank += freq[j] && (freq[j] < freq[s] || (freq[j] == freq[s] && j < s));
    order[rank] = (uint16_t)s;
}

// freq[n] -> lengths[n]: 0 for an unused symbol, 1..limit for a used one, Kraft sum exactly 1; a single used symbol gets length 1 (the one
// incomplete code zlib's inftrees.c admits).  sc.order is sorted (rank_symbol of every symbol).  One lane.
LSPPE_HD inline void build_lengths(const uint32_t *freq, uint32_t n, uint32_t limit, CodeScratch &sc, uint8_t *lengths)
{
    uint32_t used = 0;
    for (uint32_t s = 0; s < n; ++s) {
        lengths[s] = 0;
        used += freq[s] != 0;
    }
    if (used == 0) return;
    if (used == 1) {
        lengths[sc.order[0]] = 1;
        return;
    }
    // the two-queue merge: the leaves wait sorted, the inner nodes are made in rising weight
    for (uint32_t i = 0; i < used; ++i) sc.weight[i] = freq[sc.order[i]];
    uint32_t leaf = 0, inner = used, made = used;
    while (made < 2 * used - 1) {
        uint32_t pick[2];
        for (int k = 0; k < 2; ++k) pick[k] = (leaf < used && (inner >= made || sc.weight[leaf] <= sc.weight[inner])) ? leaf++ : inner++;
        sc.weight[made] = sc.weight[pick[0]] + sc.weight[pick[1]];
        sc.parent[pick[0]] = sc.parent[pick[1]] = (uint16_t)made;
        ++made;
    }
    for (uint32_t l = 0; l < 64; ++l) sc.bits[l] = 0;
    sc.depth[made - 1] = 0;
    uint32_t deepest = 0;
    for (uint32_t i = made - 1; i-- > 0;) {
        const uint32_t d = sc.depth[sc.parent[i]] + 1u;
        sc.depth[i] = (uint8_t)d;
        if (i < used) {
            const uint32_t dd = d < 63 ? d : 63;
            ++sc.bits[dd];
            deepest = dd > deepest ? dd : deepest;
        }
    }
    // Annex K.3 of the JPEG specification: a pair of the longest codes goes one level up, under a shorter code that moves one level down
    for (uint32_t i = deepest; i > limit; --i)
        while (sc.bits[i] > 0) {
            uint32_t j = i - 2;
            while (sc.bits[j] == 0) --j;
            sc.bits[i] -= 2;
            sc.bits[i - 1] += 1;
            sc.bits[j + 1] += 2;
            sc.bits[j] -= 1;
        }
    uint32_t at = 0;                                  // the rarest symbols take the longest codes
    for (uint32_t l = deepest < limit ? deepest : limit; l >= 1; --l)
        for (uint32_t k = 0; k < sc.bits[l]; ++k) lengths[sc.order[at++]] = (uint8_t)l;
}

// canonical codes (RFC 1951 3.2.2), stored bit-reversed: deflate sends Huffman codes from their most significant bit, the writer from the least
LSPPE_HD inline void make_codes(const uint8_t *lengths, uint32_t n, uint16_t *codes)
{
    uint32_t count[16] = {0}, next[16];
    for (uint32_t s = 0; s < n; ++s) ++count[lengths[s]];
    count[0] = 0;
    uint32_t code = 0;
    for (uint32_t l = 1; l < 16; ++l) {
        code = (code + count[l - 1]) << 1;
        next[l] = code;
    }
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t l = lengths[s];
        if (!l) {
            codes[s] = 0;
            continue;
        }
        uint32_t c = next[l]++, r = 0;
        for (uint32_t k = 0; k < l; ++k) r |= ((c >> k) & 1u) << (l - 1 - k);
        codes[s] = (uint16_t)r;
    }
}

// ---- the working memory of one chunk: LDS on the device --------------------------------------------------------------------------------------------
struct ChunkMem {
    union {
        uint32_t table[1u << kHashBits];              // hash -> 1 + the last position with it (0: none); dead once the candidates are known
        uint32_t out[kOutWords];                      // the payload being written
    };
    uint32_t older[1u << kHashBits];                  // what table[h] held before the last step that changed it
    uint16_t dist[kChunk];                            // per position: the distance of its first candidate, then of the match found there; 0 = none
    union {
        uint16_t hash[kChunk];                        // per position, for the look-up steps (kNone: fewer than 3 bytes left)
        uint8_t mlen[kChunk];                         // the match's length - 3
    };
    union {
        uint16_t cand2[kChunk];                       // the distance of the second candidate
        uint16_t exit_[kChunk];                       // where the greedy walk leaves the position's segment when it passes the position
    };
    uint16_t entry[kThreads];                         // where it enters segment t (kNone: it hops over it)
    uint32_t part[kThreads];                          // bits per segment and their prefix sums; then the CRC pieces
    uint32_t lfreq[288], dfreq[32], cfreq[19];
    uint8_t llen[288], dlen[32], clen[19];
    uint16_t lcode[288], dcode[32], ccode[19];
    CodeScratch lit, dst;
    uint8_t hsym[320], hext[320];                     // the dynamic header's code-length symbols and the values of their extra bits
    uint32_t nh, hlit, hdist, hclen;
    uint32_t form, bits, payload;                     // bits of the chosen block, EOB included, without the empty stored block
    uint32_t s1, s2;
};

LSPPE_HD inline uint32_t hash3(const uint8_t *p)
{
    return (((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16)) * 0x9e3779b1u) >> (32 - kHashBits);
}

// bytes that f[p ..] and f[q ..] share, at most maxlen; the first `known` (<= maxlen) are known to be equal
LSPPE_HD inline uint32_t match_length(const uint8_t *f, uint32_t p, uint32_t q, uint32_t maxlen, uint32_t known)
{
    uint32_t l = known;
    while (l + 8 <= maxlen) {
        uint64_t x, y;
        __builtin_memcpy(&x, f + p + l, 8);
        __builtin_memcpy(&y, f + q + l, 8);
        if (x != y) return l + ((uint32_t)__builtin_ctzll(x ^ y) >> 3);
        l += 8;
    }
    while (l < maxlen && f[p + l] == f[q + l]) ++l;
    return l;
}

// the match of position p (of the frame's stream f): candidates are the kNear fixed distances and the table's two; the longest wins, of equal ones
// the nearest.  Returns length << 16 | distance, or 0.  near[k] carries what fixed distance k matched at position p - 1 (0: unknown), one byte of
// which was that position's own: the rest is known to match here, so a lane that walks consecutive positions compares each byte of a long match once.
LSPPE_HD inline uint32_t find_match(const uint8_t *f, uint32_t p, uint32_t end, uint32_t bpp, uint32_t stride, uint32_t d1, uint32_t d2, uint32_t near[kNear])
{
    const uint32_t maxlen = end - p < kMaxMatch ? end - p : kMaxMatch;
    if (maxlen < kMinMatch) {
        for (uint32_t k = 0; k < kNear; ++k) near[k] = 0;
        return 0;
    }
    const uint32_t cand[kNear + 2] = {1, 2, 3, 4, 5, 6, 9, 12, stride - bpp, stride, stride + bpp, d1, d2};
    uint32_t best = 0, bdist = 0;
    for (uint32_t k = 0; k < kNear + 2; ++k) {
        const uint32_t d = cand[k];
        uint32_t known = 0;
        if (k < kNear) {
            known = near[k] ? near[k] - 1 : 0;
            known = known < maxlen ? known : maxlen;
            near[k] = 0;
        }
        if (d == 0 || d > kWindow || d > p) continue;
        if (best == maxlen && d >= bdist) continue;
        const uint32_t l = match_length(f, p, p - d, maxlen, known);
        if (k < kNear) near[k] = l;
        if (l > best || (l == best && d < bdist)) {
            best = l;
            bdist = d;
        }
    }
    if (best < kMinMatch || (best == kMinMatch && bdist > kFarDist)) return 0;
    return best << 16 | bdist;
}

// ---- bits ----------------------------------------------------------------------------------------------------------------------------------------
template <class X> LSPPE_HD inline void put_bits(const X &lanes, uint32_t *out, uint32_t at, uint32_t value, uint32_t nbits)
{
    if (!nbits) return;
    const uint32_t w = at >> 5, sh = at & 31;
    lanes.bit_or(&out[w], value << sh);
    if (sh + nbits > 32) lanes.bit_or(&out[w + 1], value >> (32 - sh));
}

// the lanes as loops: the host twin
struct HostLanes {
    template <class F> void each(F f) const
    {
        for (uint32_t t = 0; t < kThreads; ++t) f(t);
    }
    template <class F> void one(F f) const { f(); }
    void sync() const {}
    void maximum(uint32_t *a, uint32_t v) const { *a = *a < v ? v : *a; }
    void add(uint32_t *a, uint32_t v) const { *a += v; }
    void bit_or(uint32_t *a, uint32_t v) const { *a |= v; }
};

// the tokens of segment t, in order: lit(byte) or match(length, distance)
template <class Lit, class Match>
LSPPE_HD inline void walk_segment(const ChunkMem &m, const uint8_t *in, uint32_t n, uint32_t t, Lit lit, Match match)
{
    uint32_t p = m.entry[t];
    if (p == kNone) return;
    const uint32_t segend = (t + 1) * kSeg < n ? (t + 1) * kSeg : n;
    while (p < segend) {
        const uint32_t d = m.dist[p];
        if (d) {
            const uint32_t len = m.mlen[p] + kMinMatch;
            match(len, d);
            p += len;
        } else {
            lit((uint32_t)in[p]);
            ++p;
        }
    }
}

// the run-length form of the code lengths (RFC 1951 3.2.7) into m.hsym / m.hext, counting m.cfreq.  One lane.
LSPPE_HD inline void header_symbols(ChunkMem &m)
{
    const uint32_t total = m.hlit + m.hdist;
    const auto at = [&](uint32_t i) -> uint32_t { return i < m.hlit ? m.llen[i] : m.dlen[i - m.hlit]; };
    const auto emit = [&](uint32_t sym, uint32_t ext) {
        m.hsym[m.nh] = (uint8_t)sym;
        m.hext[m.nh] = (uint8_t)ext;
        ++m.nh;
        ++m.cfreq[sym];
    };
    m.nh = 0;
    for (uint32_t s = 0; s < 19; ++s) m.cfreq[s] = 0;
    uint32_t i = 0;
    while (i < total) {
        const uint32_t v = at(i);
        uint32_t run = 1;
        while (i + run < total && at(i + run) == v) ++run;
        i += run;
        if (v == 0) {
            while (run >= 11) {
                const uint32_t r = run < 138 ? run : 138;
                emit(18, r - 11);
                run -= r;
            }
            if (run >= 3) {
                emit(17, run - 3);
                run = 0;
            }
        } else {
            emit(v, 0);
            --run;
            while (run >= 3) {
                const uint32_t r = run < 6 ? run : 6;
                emit(16, r - 3);
                run -= r;
            }
        }
        for (; run; --run) emit(v, 0);
    }
}

LSPPE_HD inline uint32_t cl_order(uint32_t i)
{
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return order[i];
}

// One chunk: in = the frame's filtered stream, [base, base + n) the chunk.  Leaves the payload in m.out and its record in *rec.
// first / last: the chunk opens (the zlib header goes into its IDAT, and into its CRC) / closes the frame's stream (BFINAL).
template <class X>
LSPPE_HD inline void encode_chunk(const X &lanes, ChunkMem &m, const uint8_t *f, const Geom &g, uint32_t chunk, ChunkRec *rec, uint32_t *forms)
{
    const uint32_t base = chunk * kChunk, n = g.raw - base < kChunk ? g.raw - base : kChunk, end = base + n;
    const uint32_t lo = base > kWindow ? base - kWindow : 0;
    const bool first = chunk == 0, last = chunk + 1 == g.nchunks;
    const uint8_t *in = f + base;
    const uint32_t nseg = (n + kSeg - 1) / kSeg;

    lanes.each([&](uint32_t t) {
        for (uint32_t i = t; i < (1u << kHashBits); i += kThreads) m.table[i] = m.older[i] = 0;
        for (uint32_t i = t; i < 288; i += kThreads) m.lfreq[i] = 0;
        if (t < 32) m.dfreq[t] = 0;
        if (t == 0) m.s1 = m.s2 = 0;
    });
    lanes.sync();

    if (g.level > 0) {
        // hash: every position's, and the window before the chunk into the table
        lanes.each([&](uint32_t t) {
            for (uint32_t i = t; i < n; i += kThreads) m.hash[i] = (uint16_t)(base + i + kMinMatch <= g.raw ? hash3(in + i) : kNone);
            for (uint32_t p = lo + t; p < base; p += kThreads)
                if (p + kMinMatch <= g.raw) lanes.maximum(&m.table[hash3(f + p)], p + 1);
        });
        lanes.sync();
        // look up: kStep positions per step, LDS only.  A candidate further away than kWindow is none.
        for (uint32_t step = 0; step < n; step += kStep) {
            lanes.each([&](uint32_t t) {
                const uint32_t i = step + t;
                if (t >= kStep || i >= n) return;
                const uint32_t h = m.hash[i], e1 = h == kNone ? 0 : m.table[h], e2 = h == kNone ? 0 : m.older[h];
                m.dist[i] = (uint16_t)(e1 && base + i + 1 - e1 <= kWindow ? base + i + 1 - e1 : 0);
                m.cand2[i] = (uint16_t)(e2 && base + i + 1 - e2 <= kWindow ? base + i + 1 - e2 : 0);
            });
            lanes.sync();
            lanes.each([&](uint32_t t) {
                const uint32_t i = step + t;
                if (t >= kStep || i >= n || m.hash[i] == kNone) return;
                if (m.dist[i]) m.older[m.hash[i]] = base + i + 1 - m.dist[i];
                lanes.maximum(&m.table[m.hash[i]], base + i + 1);
            });
            lanes.sync();
        }
        // match: every position; a lane walks the kSeg positions of its segment in turn
        lanes.each([&](uint32_t t) {
            uint32_t near[kNear] = {0};
            for (uint32_t i = t * kSeg; i < (t + 1) * kSeg && i < n; ++i) {
                const uint32_t found = find_match(f, base + i, end, g.comps, g.stride, m.dist[i], m.cand2[i], near);
                m.dist[i] = (uint16_t)(found & 0xffff);
                m.mlen[i] = (uint8_t)(found ? (found >> 16) - kMinMatch : 0);
            }
        });
        lanes.sync();
        // choose: where the walk leaves segment t from each of its positions, last position first
        lanes.each([&](uint32_t t) {
            if (t >= nseg) return;
            const uint32_t segend = (t + 1) * kSeg < n ? (t + 1) * kSeg : n;
            for (uint32_t i = segend; i-- > t * kSeg;) {
                const uint32_t nx = i + (m.dist[i] ? m.mlen[i] + kMinMatch : 1);
                m.exit_[i] = (uint16_t)(nx < segend ? m.exit_[nx] : nx);
            }
        });
        lanes.sync();
        lanes.one([&]() {
            uint32_t e = 0;
            for (uint32_t s = 0; s < kThreads; ++s) {
                const uint32_t segend = (s + 1) * kSeg < n ? (s + 1) * kSeg : n;
                if (s < nseg && e < segend) {
                    m.entry[s] = (uint16_t)e;
                    e = m.exit_[e];
                } else {
                    m.entry[s] = (uint16_t)kNone;
                }
            }
        });
        lanes.sync();
        // codes: the histograms
        lanes.each([&](uint32_t t) {
            walk_segment(
                m, in, n, t, [&](uint32_t byte) { lanes.add(&m.lfreq[byte], 1); },
                [&](uint32_t len, uint32_t d) {
                    uint32_t eb, ev;
                    lanes.add(&m.lfreq[257 + length_symbol(len, &eb, &ev)], 1);
                    lanes.add(&m.dfreq[dist_symbol(d, &eb, &ev)], 1);
                });
            if (t == 0) lanes.add(&m.lfreq[256], 1);
        });
        lanes.sync();
        lanes.each([&](uint32_t t) {
            for (uint32_t s = t; s < 286; s += kThreads) rank_symbol(m.lfreq, 286, s, m.lit.order);
            if (t < 30) rank_symbol(m.dfreq, 30, t, m.dst.order);
        });
        lanes.sync();
        lanes.each([&](uint32_t t) {
            if (t == 0) {
                build_lengths(m.lfreq, 286, 15, m.lit, m.llen);
                m.llen[286] = m.llen[287] = 0;
            }
            if (t == 64 % kThreads) {
                build_lengths(m.dfreq, 30, 15, m.dst, m.dlen);
                m.dlen[30] = m.dlen[31] = 0;
            }
        });
        lanes.sync();
        // the dynamic header and the three sizes
        lanes.one([&]() {
            m.hlit = 286;
            while (m.hlit > 257 && m.llen[m.hlit - 1] == 0) --m.hlit;
            m.hdist = 30;
            while (m.hdist > 1 && m.dlen[m.hdist - 1] == 0) --m.hdist;
            header_symbols(m);
            for (uint32_t s = 0; s < 19; ++s) rank_symbol(m.cfreq, 19, s, m.lit.order);
            build_lengths(m.cfreq, 19, 7, m.lit, m.clen);
            uint32_t used = 0, only = 0;
            for (uint32_t s = 0; s < 19; ++s)
                if (m.clen[s]) {
                    ++used;
                    only = s;
                }
            if (used == 1) m.clen[only ? 0 : 1] = 1;              // the code-length code must be complete: a second code of one bit, never sent
            make_codes(m.clen, 19, m.ccode);
            m.hclen = 19;
            while (m.hclen > 4 && m.clen[cl_order(m.hclen - 1)] == 0) --m.hclen;
            uint32_t dyn = 3 + 5 + 5 + 4 + 3 * m.hclen, fix = 3;
            for (uint32_t k = 0; k < m.nh; ++k) {
                const uint32_t s = m.hsym[k];
                dyn += m.clen[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0);
            }
            for (uint32_t s = 0; s < 286; ++s) {
                const uint32_t eb = s > 256 ? length_extra_bits(s - 257) : 0;
                dyn += m.lfreq[s] * (m.llen[s] + eb);
                fix += m.lfreq[s] * (fixed_length(s) + eb);
            }
            for (uint32_t s = 0; s < 30; ++s) {
                dyn += m.dfreq[s] * (m.dlen[s] + dist_extra_bits(s));
                fix += m.dfreq[s] * (5 + dist_extra_bits(s));
            }
            const uint32_t stored_bytes = n + kStoredOverhead, fix_bytes = (fix + 3 + 7) / 8 + 4, dyn_bytes = (dyn + 3 + 7) / 8 + 4;
            m.form = FORM_STORED;
            m.payload = stored_bytes;
            m.bits = 0;
            if (fix_bytes < m.payload) {
                m.form = FORM_FIXED;
                m.payload = fix_bytes;
                m.bits = fix;
            }
            if (dyn_bytes < m.payload) {
                m.form = FORM_DYNAMIC;
                m.payload = dyn_bytes;
                m.bits = dyn;
            }
            if (m.form == FORM_FIXED) {
                for (uint32_t s = 0; s < 288; ++s) m.llen[s] = (uint8_t)fixed_length(s);
                for (uint32_t s = 0; s < 32; ++s) m.dlen[s] = 5;
            }
            if (m.form != FORM_STORED) {
                make_codes(m.llen, 288, m.lcode);
                make_codes(m.dlen, 32, m.dcode);
            }
        });
    } else {
        lanes.one([&]() {
            m.form = FORM_STORED;
            m.payload = n + kStoredOverhead;
            m.bits = 0;
        });
    }
    lanes.sync();

    const uint32_t form = m.form, payload = m.payload;
    uint8_t *bytes = reinterpret_cast<uint8_t *>(m.out);
    // write: into a zeroed buffer
    lanes.each([&](uint32_t t) {
        for (uint32_t w = t; w < (payload + 3) / 4; w += kThreads) m.out[w] = 0;
    });
    lanes.sync();
    if (form == FORM_STORED) {
        lanes.each([&](uint32_t t) {
            for (uint32_t i = t; i < n; i += kThreads) bytes[5 + i] = in[i];
            if (t == 0) {
                bytes[1] = (uint8_t)n;
                bytes[2] = (uint8_t)(n >> 8);
                bytes[3] = (uint8_t)~n;
                bytes[4] = (uint8_t)(~n >> 8);
                bytes[5 + n] = last ? 1 : 0;
                bytes[5 + n + 3] = bytes[5 + n + 4] = 0xff;
            }
        });
    } else {
        // the bits of every segment, their prefix sums, and the tokens at their places
        const auto token_bits = [&](uint32_t t) {
            uint32_t b = 0;
            walk_segment(
                m, in, n, t, [&](uint32_t byte) { b += m.llen[byte]; },
                [&](uint32_t len, uint32_t d) {
                    uint32_t eb, ev;
                    b += m.llen[257 + length_symbol(len, &eb, &ev)] + eb;
                    b += m.dlen[dist_symbol(d, &eb, &ev)];
                    b += eb;
                });
            return b;
        };
        lanes.each([&](uint32_t t) { m.part[t] = token_bits(t); });
        lanes.sync();
        lanes.one([&]() {
            // the block's header, then where every segment starts
            uint32_t at = 0;
            put_bits(lanes, m.out, at, form == FORM_FIXED ? 2u : 4u, 3);        // BFINAL 0, BTYPE 01 / 10 (sent from the least significant bit)
            at += 3;
            if (form == FORM_DYNAMIC) {
                put_bits(lanes, m.out, at, m.hlit - 257, 5);
                put_bits(lanes, m.out, at + 5, m.hdist - 1, 5);
                put_bits(lanes, m.out, at + 10, m.hclen - 4, 4);
                at += 14;
                for (uint32_t k = 0; k < m.hclen; ++k, at += 3) put_bits(lanes, m.out, at, m.clen[cl_order(k)], 3);
                for (uint32_t k = 0; k < m.nh; ++k) {
                    const uint32_t s = m.hsym[k], eb = s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0;
                    put_bits(lanes, m.out, at, m.ccode[s], m.clen[s]);
                    put_bits(lanes, m.out, at + m.clen[s], m.hext[k], eb);
                    at += m.clen[s] + eb;
                }
            }
            for (uint32_t t = 0; t < kThreads; ++t) {
                const uint32_t b = m.part[t];
                m.part[t] = at;
                at += b;
            }
            put_bits(lanes, m.out, at, m.lcode[256], m.llen[256]);
            at += m.llen[256];
            // the empty stored block: BFINAL, BTYPE 00, zeros up to the byte, LEN 0, NLEN ffff
            put_bits(lanes, m.out, at, last ? 1u : 0u, 3);
            const uint32_t byte = (at + 3 + 7) / 8;
            bytes[byte + 2] = bytes[byte + 3] = 0xff;
        });
        lanes.sync();
        lanes.each([&](uint32_t t) {
            uint32_t at = m.part[t];
            walk_segment(
                m, in, n, t,
                [&](uint32_t byte) {
                    put_bits(lanes, m.out, at, m.lcode[byte], m.llen[byte]);
                    at += m.llen[byte];
                },
                [&](uint32_t len, uint32_t d) {
                    uint32_t eb, ev;
                    const uint32_t ls = 257 + length_symbol(len, &eb, &ev);
                    put_bits(lanes, m.out, at, m.lcode[ls] | (ev << m.llen[ls]), m.llen[ls] + eb);
                    at += m.llen[ls] + eb;
                    const uint32_t ds = dist_symbol(d, &eb, &ev);
                    put_bits(lanes, m.out, at, m.dcode[ds] | (ev << m.dlen[ds]), m.dlen[ds] + eb);
                    at += m.dlen[ds] + eb;
                });
        });
    }
    lanes.sync();

    // sums: CRC-32 of "IDAT" [78 01] payload in kThreads pieces, the first ones short or empty; Adler-32 of the input per segment
    const uint32_t piece = (payload + kThreads - 1) / kThreads;
    lanes.each([&](uint32_t t) {
        const uint32_t back = (kThreads - t) * piece;                     // the piece is [payload - back, payload - back + piece), cut at 0
        const uint32_t from = back > payload ? 0 : payload - back, to = back - piece > payload ? 0 : payload - (back - piece);
        uint32_t r = 0;
        for (uint32_t i = from; i < to; ++i) r = crc_step(r, bytes[i]);
        m.part[t] = r;
        if (t < nseg) {
            const uint32_t a = t * kSeg, b = (t + 1) * kSeg < n ? (t + 1) * kSeg : n;
            uint32_t s1 = 0, s2 = 0;
            for (uint32_t i = a; i < b; ++i) {
                s1 += in[i];
                s2 += (b - i) * in[i];
            }
            lanes.add(&m.s1, s1);
            lanes.add(&m.s2, (s2 + (n - b) * s1) % kAdlerMod);
        }
    });
    lanes.sync();
    uint32_t xp = gf_xpow_bytes(piece ? piece : 1);
    for (uint32_t stride = 1; stride < kThreads; stride <<= 1) {
        lanes.each([&](uint32_t t) {
            if (t % (2 * stride) == 0) m.part[t] = gf_mul(xp, m.part[t]) ^ m.part[t + stride];
        });
        lanes.sync();
        xp = gf_mul(xp, xp);
    }
    lanes.one([&]() {
        uint32_t r = 0xffffffffu;
        const uint8_t type[6] = {'I', 'D', 'A', 'T', 0x78, 0x01};
        for (uint32_t i = 0; i < (first ? 6u : 4u); ++i) r = crc_step(r, type[i]);
        rec->payload = payload;
        rec->crc = ~(gf_mul(gf_xpow_bytes(payload), r) ^ m.part[0]);
        rec->s1 = m.s1 % kAdlerMod;
        rec->s2 = m.s2 % kAdlerMod;
        if (forms) ++forms[form];
    });
    lanes.sync();
}

// ---- the frame around the chunks ---------------------------------------------------------------------------------------------------------------------
// bytes of chunk c in the file
LSPPE_HD inline uint32_t chunk_file_bytes(const ChunkRec &r, uint32_t c) { return kIdatOverhead + r.payload + (c == 0 ? 2u : 0u); }
// what chunk c adds to the frame's second Adler sum: its own, and its byte sum once for every byte behind it
LSPPE_HD inline uint32_t adler_s2_share(const ChunkRec &r, uint32_t c, const Geom &g)
{
    const uint64_t end = (uint64_t)(c + 1) * kChunk < g.raw ? (uint64_t)(c + 1) * kChunk : g.raw;
    return (uint32_t)((r.s2 + ((g.raw - end) % kAdlerMod) * r.s1) % kAdlerMod);
}
// the 28 bytes behind the last chunk: an IDAT with the Adler-32, and IEND.  s1, s2: the sums over all chunks modulo 65521.
LSPPE_HD inline void write_tail(uint8_t *dst, uint32_t s1, uint32_t s2, const Geom &g)
{
    const uint32_t a = (1 + s1) % kAdlerMod, b = (g.raw % kAdlerMod + s2) % kAdlerMod;
    const uint8_t type[4] = {'I', 'D', 'A', 'T'}, iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xae, 0x42, 0x60, 0x82};
    put_be32(dst, 4);
    for (int i = 0; i < 4; ++i) dst[4 + i] = type[i];
    put_be32(dst + 8, b << 16 | a);
    uint32_t r = 0xffffffffu;
    for (int i = 4; i < 12; ++i) r = crc_step(r, dst[i]);
    put_be32(dst + 12, ~r);
    for (int i = 0; i < 12; ++i) dst[16 + i] = iend[i];
}
// byte i of chunk c's IDAT chunk in the file (i < chunk_file_bytes)
LSPPE_HD inline uint8_t chunk_file_byte(const ChunkRec &r, uint32_t c, const uint8_t *payload, uint32_t i)
{
    const uint32_t head = c == 0 ? 10 : 8, data = r.payload + (c == 0 ? 2u : 0u);
    if (i < 4) return (uint8_t)(data >> (24 - 8 * i));
    if (i < 8) return (uint8_t)("IDAT"[i - 4]);
    if (i < head) return i == 8 ? 0x78 : 0x01;
    if (i < head + r.payload) return payload[i - head];
    return (uint8_t)(r.crc >> (24 - 8 * (i - head - r.payload)));
}

// signature + IHDR
inline void write_header(const Geom &g, uint8_t *dst)
{
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    for (int i = 0; i < 8; ++i) dst[i] = sig[i];
    put_be32(dst + 8, 13);
    dst[12] = 'I', dst[13] = 'H', dst[14] = 'D', dst[15] = 'R';
    put_be32(dst + 16, g.width);
    put_be32(dst + 20, g.height);
    dst[24] = 8;
    dst[25] = g.comps == 3 ? 2 : 0;
    dst[26] = dst[27] = dst[28] = 0;
    put_be32(dst + 29, crc_bytes(dst + 12, 17));
}

inline bool make_geom(int width, int height, int comps, int level, int filter, int max_side, Geom *g)
{
    if (width < 1 || height < 1 || width > max_side || height > max_side || (comps != 1 && comps != 3)) return false;
    if (level < 0 || level > 1 || filter < -1 || filter > 4) return false;
    g->width = (uint32_t)width;
    g->height = (uint32_t)height;
    g->comps = (uint32_t)comps;
    g->stride = 1 + g->width * g->comps;
    g->raw = g->height * g->stride;
    g->nchunks = chunk_count(g->raw);
    g->level = (uint32_t)level;
    g->filter = filter < 0 ? kFilterHeuristic : (uint32_t)filter;
    g->cap = capacity_bound(g->raw);
    return true;
}

// the whole file on the host, with the code the kernels run: lines = raw bytes of scratch, slots = nchunks * kSlotBytes, recs = nchunks records,
// file = kHeaderBytes + cap bytes.  forms (may be null) counts the chunks per block form; rows (may be null) the rows per filter.  Returns the size.
inline size_t encode_host(const Geom &g, const uint8_t *px, ChunkMem &m, uint8_t *lines, uint8_t *slots, ChunkRec *recs, uint8_t *file, uint32_t *forms,
                          uint32_t *rows)
{
    const uint32_t rowbytes = g.width * g.comps;
    for (uint32_t y = 0; y < g.height; ++y) {
        uint32_t type = g.filter;
        if (type == kFilterHeuristic) {
            uint32_t sums[5];
            filter_sums(px, rowbytes, g.comps, y, 0, 1, sums);
            type = filter_choice(sums);
        }
        if (rows) ++rows[type];
        filter_write(px, rowbytes, g.comps, y, type, 0, 1, lines + (size_t)y * g.stride);
    }
    const HostLanes lanes;
    for (uint32_t c = 0; c < g.nchunks; ++c) {
        encode_chunk(lanes, m, lines, g, c, &recs[c], forms);
        const uint8_t *out = reinterpret_cast<const uint8_t *>(m.out);
        for (uint32_t i = 0; i < recs[c].payload; ++i) slots[(size_t)c * kSlotBytes + i] = out[i];
    }
    write_header(g, file);
    size_t at = kHeaderBytes;
    uint32_t s1 = 0, s2 = 0;
    for (uint32_t c = 0; c < g.nchunks; ++c) {
        const uint32_t nb = chunk_file_bytes(recs[c], c);
        for (uint32_t i = 0; i < nb; ++i) file[at + i] = chunk_file_byte(recs[c], c, slots + (size_t)c * kSlotBytes, i);
        at += nb;
        s1 = (s1 + recs[c].s1) % kAdlerMod;
        s2 = (s2 + adler_s2_share(recs[c], c, g)) % kAdlerMod;
    }
    write_tail(file + at, s1, s2, g);
    return at + 28;
}

}  // namespace lsppngenc
#endif
