// jpegdec.hip -- the JPEG decoder of include/lspjpegdec.h: three stages on the device (entropy decode, dequantise + IDCT, upsample +
// colour + store) behind a host planner; stage 1 has a second kernel for complete progressive files (LSPJPEG_DEC_FLAG_PROGRESSIVE) and a third that decodes inside a restart interval in parallel (LSPJPEG_DEC_FLAG_PARALLEL).  The arithmetic is libjpeg's integer arithmetic step by step (jdhuff.c, jidctint.c, jdsample.c,
// jdcolor.c): for a file Pillow can open the output equals Pillow's pixels.  The parser and the segment decoder live in jpegdec_core.h, which is
// also built for the host alone and run under sanitizers (make check-jpegdec).
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/lspjpeg.h"
#include "../../include/lspjpegdec.h"
#include "jpegdec_plan.h"

namespace {

using namespace lspdec;

thread_local std::string g_err;
thread_local ParStats g_par_stats;           // of this thread's last lspjpeg_dec_host_coefficients
int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

struct Params {
    unsigned char *blob;                    // the descriptor block on the device
    const FileDesc *files;
    const SegDesc *segs;
    const HuffTable *tables;
    unsigned *status;                       // [nfiles]
    short *coef;                            // [total blocks][64] natural order, MCU order per file
    unsigned char *planes;
    unsigned nfiles, nsegs;
    unsigned long long bytes;               // of the block: no load reaches past it
    const ScanDesc *scans;                  // progressive files: their scans, those scans' restart intervals and table snapshots
    const SegDesc *psegs;
    const HuffTable *ptables;
};

constexpr int kWave = 64;
constexpr unsigned kRing = 8192;            // bytes of the stream window in LDS: > kMcuBytesBound + one refill of kWave * 16 bytes
static_assert(kRing >= kMcuBytesBound + 2 * kWave * 16 && (kRing & (kRing - 1)) == 0, "the window holds one MCU's worst case behind a refill");

// the byte source of BitReader on the device: the window, indexed by the offset inside the block
struct RingSrc {
    const unsigned char *ring;
    __device__ uint8_t at(uint64_t pos) const { return ring[pos & (kRing - 1)]; }
};

// ---- stage 1: one wave per restart interval.  All lanes stage the stream (16 bytes per lane and refill) and move finished MCUs to memory
// (16 bytes per lane); lane 0 walks the Huffman codes out of LDS.  Reads are bounded by the segment's end (BitReader) and by the block's end
// (the refill); writes by the segment's MCU count, which the planner derived from the file's geometry.
__global__ __launch_bounds__(kWave) void jpegdec_entropy(Params p)
{
    __shared__ uint4 s_tab[4 * sizeof(HuffTable) / 16];
    __shared__ uint4 s_ring[kRing / 16];
    __shared__ uint4 s_mcu[kMaxBlocksPerMcu * 8];
    __shared__ unsigned long long s_pos;
    __shared__ unsigned s_st;
    if (blockIdx.x >= p.nsegs) return;
    const SegDesc sg = p.segs[blockIdx.x];
    const FileDesc &f = p.files[sg.file];
    const int lane = threadIdx.x;
    const uint4 *tab = reinterpret_cast<const uint4 *>(p.tables + f.table0);
    for (unsigned k = lane; k < 4 * sizeof(HuffTable) / 16; k += kWave) s_tab[k] = tab[k];
    if (lane < kMaxBlocksPerMcu * 8) s_mcu[lane] = make_uint4(0, 0, 0, 0);
    uint8_t comp_of[kMaxBlocksPerMcu];
    int bpm;
    block_components(f.ncomp, f.hs, f.vs, comp_of, &bpm);
    const RingSrc src{reinterpret_cast<const unsigned char *>(s_ring)};
    BitReader<RingSrc> br(src, sg.begin, sg.end);
    int pred[3] = {0, 0, 0};
    unsigned long long filled = sg.begin & ~15ull, pos = sg.begin;
    uint4 *dst = reinterpret_cast<uint4 *>(p.coef + (f.coef_off + (unsigned long long)sg.mcu0 * bpm) * 64);
    unsigned st = ST_OK;
    for (unsigned m = 0; m < sg.nmcu; ++m) {
        unsigned long long want = pos + kMcuBytesBound;
        if (want > sg.end) want = sg.end;
        while (filled < want) {
            const unsigned long long off = filled + (unsigned long long)lane * 16;
            if (off + 16 <= p.bytes) s_ring[(off >> 4) & (kRing / 16 - 1)] = *reinterpret_cast<const uint4 *>(p.blob + off);
            filled += kWave * 16;
        }
        __syncthreads();
        if (lane == 0) {
            unsigned r = decode_mcu(br, reinterpret_cast<const HuffTable *>(s_tab), f.dc_sel, f.ac_sel, comp_of, bpm, pred, reinterpret_cast<int16_t *>(s_mcu));
            if (r == ST_OK && m + 1 == sg.nmcu && !br.drained()) r = ST_CORRUPT;
            s_st = r;
            s_pos = br.pos;
        }
        __syncthreads();
        st = s_st;
        pos = s_pos;
        if (st != ST_OK) break;
        if (lane < bpm * 8) {
            dst[(size_t)m * bpm * 8 + lane] = s_mcu[lane];
            s_mcu[lane] = make_uint4(0, 0, 0, 0);
        }
    }
    if (st != ST_OK && lane == 0) atomicCAS(p.status + sg.file, 0u, st);
}

// ---- stage 1 on the parallel route (LSPJPEG_DEC_FLAG_PARALLEL): one workgroup of kParLanes lanes per restart interval, decoding INSIDE the
// interval in parallel (jpegdec_core.h: decode_subsequence and the fixed point it serves; jpegdec_plan.h host_parallel_segment is this kernel with
// the lanes as loops).  The interval is walked in chunks of kParLanes subsequences.  Per chunk: the stream bytes are staged into LDS in 16-byte
// loads (with 16 bytes in front for the stuffed-pair test and 32 behind for the code that runs past the last boundary); every lane decodes its
// subsequence from its entry state without writing and the lanes hand their exit states on through LDS until no entry changes (a lane behind a
// dead exit keeps its own guess); an exclusive scan over blocks started, DC sums and dead exits gives each lane its block index and DC
// predictions and says whether its entry is true (no dead exit in front of it); each such lane decodes once more and writes coefficients.  The last exit state, the block count and the predictions carry over to the next chunk in LDS: no host loop, no
// global scratch.  Nothing is capped: a stream that never resynchronises costs one round per subsequence, the serial decode.
// Reads are bounded by the interval's end (BitReader) and the block's end (the staging); writes by the interval's block count nmcu * bpm, which
// decode_subsequence checks before every block it enters.
// Hazards.  (1) The interval's coefficient range is zeroed with 16-byte stores by all waves, and the write pass later stores 2-byte values to the
// same addresses from OTHER waves: a device-scope fence (__threadfence) after the zeroing and the workgroup barrier behind it order the two
// (each wave's zero stores are complete and visible device-wide before any wave passes the barrier).  Stage 2 reads the coefficients behind a
// kernel boundary.  (2) LDS: every exchange (window, exit states, scan inputs, carry, failure word) has a barrier between its writers and
// its readers, and one more before the words are written again.  (3) Two lanes never write the same coefficient: a block belongs to the lanes
// its codes start in, each code to one lane.
constexpr unsigned kParWindow = kParLanes * kSubseqBytes + 64;
static_assert(kParWindow % 16 == 0 && kParLanes % kWave == 0 && kParLanes <= 1024, "the window is staged in 16-byte loads by whole waves");

struct WindowSrc {
    const unsigned char *win;
    unsigned long long base;                // offset inside the block of win[0]
    __device__ uint8_t at(uint64_t pos) const { return win[pos - base]; }
};

__global__ __launch_bounds__(kParLanes) void jpegdec_entropy_parallel(Params p)
{
    __shared__ uint4 s_tab[4 * sizeof(HuffTable) / 16];
    __shared__ uint4 s_win[kParWindow / 16];
    __shared__ ParState s_exit[kParLanes];
    __shared__ unsigned s_blocks[kParLanes];
    __shared__ int s_dc[3][kParLanes];
    __shared__ unsigned s_dead[kParLanes];
    __shared__ unsigned s_wave_blocks[kParLanes / kWave], s_wave_dead[kParLanes / kWave];
    __shared__ int s_wave_dc[3][kParLanes / kWave];
    __shared__ ParState s_carry;
    __shared__ unsigned s_carry_blocks;
    __shared__ int s_carry_pred[3];
    __shared__ unsigned s_fail, s_done;
    if (blockIdx.x >= p.nsegs) return;
    const SegDesc sg = p.segs[blockIdx.x];
    const ParGeom g = par_geom(p.files[sg.file]);                              // the geometry in registers: the stores below may alias nothing of it
    const unsigned table0 = p.files[sg.file].table0;
    const unsigned long long coef_off = p.files[sg.file].coef_off;
    const unsigned lane = threadIdx.x;
    const uint4 *tab = reinterpret_cast<const uint4 *>(p.tables + table0);
    for (unsigned k = lane; k < 4 * sizeof(HuffTable) / 16; k += kParLanes) s_tab[k] = tab[k];
    const unsigned total = sg.nmcu * g.bpm;
    short *coef = p.coef + (coef_off + (unsigned long long)sg.mcu0 * g.bpm) * 64;
    for (unsigned long long k = lane; k < (unsigned long long)total * 8; k += kParLanes) reinterpret_cast<uint4 *>(coef)[k] = make_uint4(0, 0, 0, 0);
    if (lane == 0) {
        s_carry = ParState{sg.begin * 8, 0, 0, 0};
        s_carry_blocks = 0;
        s_carry_pred[0] = s_carry_pred[1] = s_carry_pred[2] = 0;
        s_fail = ~0u;
        s_done = 0;
    }
    __threadfence();                                                           // hazard (1)
    __syncthreads();
    const HuffTable *tables = reinterpret_cast<const HuffTable *>(s_tab);
    const unsigned nsub = subsequences_of(sg.begin, sg.end);
    for (unsigned c0 = 0; c0 < nsub; c0 += kParLanes) {
        const unsigned nl = nsub - c0 < kParLanes ? nsub - c0 : kParLanes;
        const unsigned long long cb = sg.begin + (unsigned long long)c0 * kSubseqBytes;
        const WindowSrc src{reinterpret_cast<const unsigned char *>(s_win), (cb - 16) & ~15ull};
        for (unsigned k = lane; k < kParWindow / 16; k += kParLanes) {
            const unsigned long long off = src.base + (unsigned long long)k * 16;
            if (off + 16 <= p.bytes) s_win[k] = *reinterpret_cast<const uint4 *>(p.blob + off);
        }
        __syncthreads();                                                       // the window, and the carry of the chunk before
        const bool active = lane < nl;
        unsigned long long limit = cb + (unsigned long long)(lane + 1) * kSubseqBytes;
        if (limit > sg.end) limit = sg.end;
        const ParState guess = guess_state(src, sg.begin, sg.end, cb + (unsigned long long)lane * kSubseqBytes);
        ParState entry = lane ? guess : s_carry;
        ParResult res;
        bool changed = active;
        for (;;) {                                                             // the fixed point
            if (changed) {
                decode_subsequence<false>(src, sg.begin, sg.end, limit, entry, tables, g, 0, 0, nullptr, nullptr, false, &res);
                s_exit[lane] = res.exit;
            }
            __syncthreads();
            changed = false;
            if (active && lane) {
                const ParState before = s_exit[lane - 1], want = before.dead ? guess : before;     // behind a dead exit the lane's own guess stands again
                if (!same_state(want, entry)) {
                    entry = want;
                    changed = true;
                }
            }
            if (!__syncthreads_or(changed)) break;                             // also: every exit state is read before one is written again
        }
        // the exclusive scan, in two levels: per wave, then over the waves
        s_blocks[lane] = active ? res.blocks : 0u;
        s_dead[lane] = active && res.exit.dead ? 1u : 0u;
        for (int c = 0; c < 3; ++c) s_dc[c][lane] = active ? res.dc[c] : 0;
        __syncthreads();
        if (lane < kParLanes / kWave) {
            unsigned nb = 0, nd = 0;
            int dc[3] = {0, 0, 0};
            for (unsigned j = lane * kWave; j < (lane + 1) * kWave; ++j) {
                nb += s_blocks[j];
                nd += s_dead[j];
                for (int c = 0; c < 3; ++c) dc[c] += s_dc[c][j];
            }
            s_wave_blocks[lane] = nb;
            s_wave_dead[lane] = nd;
            for (int c = 0; c < 3; ++c) s_wave_dc[c][lane] = dc[c];
        }
        __syncthreads();
        unsigned blocks = s_carry_blocks, dead = 0;                            // dead exits in front of this lane: its entry is true when there is none
        int pred[3] = {s_carry_pred[0], s_carry_pred[1], s_carry_pred[2]};
        for (unsigned w = 0; w < lane / kWave; ++w) {
            blocks += s_wave_blocks[w];
            dead += s_wave_dead[w];
            for (int c = 0; c < 3; ++c) pred[c] += s_wave_dc[c][w];
        }
        for (unsigned j = lane / kWave * kWave; j < lane; ++j) {
            blocks += s_blocks[j];
            dead += s_dead[j];
            for (int c = 0; c < 3; ++c) pred[c] += s_dc[c][j];
        }
        // the write pass, from the true entries
        if (active && !dead && !entry.dead && (entry.k == 0 || blocks > 0)) {
            ParResult w;
            decode_subsequence<true>(src, sg.begin, sg.end, limit, entry, tables, g, entry.k ? blocks - 1 : blocks, total, pred, coef, c0 + lane + 1 == nsub, &w);
            if (w.status != ST_OK) atomicMin(&s_fail, (lane << 2) | w.status);  // the lowest lane is the earliest failure in stream order
            if (w.done) s_done = 1;
        }
        __syncthreads();                                                       // the carry has been read by every lane
        if (lane == nl - 1) {
            s_carry = res.exit;
            s_carry_blocks = blocks + res.blocks;
            for (int c = 0; c < 3; ++c) s_carry_pred[c] = pred[c] + res.dc[c];
        }
        __syncthreads();
        if (s_fail != ~0u || s_done) break;                                    // behind a failure or the last block nothing is a state of the file
    }
    // neither a failure nor the last block: unreachable (a true entry with a dead exit fails or finishes in the write pass, and the interval's
    // last lane reports data that ends early); CORRUPT, as host_parallel_segment answers
    if (lane == 0 && (s_fail != ~0u || !s_done)) atomicCAS(p.status + sg.file, 0u, s_fail != ~0u ? s_fail & 3u : (unsigned)ST_CORRUPT);
}

// ---- stage 1 of the progressive files: one wave per file, every scan of the file in file order over the same coefficients (a refinement reads
// what the earlier scans left, so a file is one serial walk; files run beside each other).  The wave zeroes the file's coefficients, then for each
// restart interval of each scan stages the stream through the LDS window as above and moves kStage blocks at a time between the workspace and LDS,
// 16 bytes per lane, turning each block into zigzag order on the way in and back on the way out, so that lane 0, which runs the four procedures
// (prog_units) on the staged blocks, indexes LDS by the band position and looks nothing up.  A scan of one component walks
// that component's own raster, so each staged block's place comes from prog_block_index().  Reads are bounded by the interval's end (BitReader) and
// the block's end (the refill); writes by the file's block count.  Every store of a block is separated from the next load of it by a barrier of the
// (single-wave) workgroup, which also orders the zeroing before the first scan's loads.
constexpr unsigned kStage = 64;             // blocks per barrier pair: 8 KiB of LDS
constexpr unsigned kProgRing = 32768;       // the stream window: one stage's worst case behind a refill
static_assert(kProgRing >= kStage * kBlockBytesBound + 2 * kWave * 16 && (kProgRing & (kProgRing - 1)) == 0, "the window holds one stage's worst case behind a refill");
static_assert(kStage >= kMaxBlocksPerMcu && kStage * 8 % kWave == 0, "a stage holds at least one MCU, and the lanes move it in whole rounds");

struct ProgRingSrc {
    const unsigned char *ring;
    __device__ uint8_t at(uint64_t pos) const { return ring[pos & (kProgRing - 1)]; }
};

__global__ __launch_bounds__(kWave) void jpegdec_progressive(Params p)
{
    __shared__ uint4 s_tab[4 * sizeof(HuffTable) / 16];
    __shared__ uint4 s_ring[kProgRing / 16];
    __shared__ short s_blk[kStage * 64];                                       // zigzag order inside a block
    __shared__ unsigned long long s_pos;
    __shared__ unsigned s_st;
    const unsigned fi = blockIdx.x;
    if (fi >= p.nfiles) return;
    const FileDesc &gf = p.files[fi];
    if (!gf.progressive || gf.status != ST_OK) return;
    FileDesc f{};                                                              // the geometry in registers: the stores below may alias nothing of it
    f.ncomp = gf.ncomp;
    f.hs = gf.hs;
    f.vs = gf.vs;
    f.mcux = gf.mcux;
    f.bpm = gf.bpm;
    f.nblk = gf.nblk;
    f.scan0 = gf.scan0;
    f.nscan = gf.nscan;
    const int lane = threadIdx.x;
    uint4 *coef = reinterpret_cast<uint4 *>(p.coef + gf.coef_off * 64);
    const unsigned nblk = f.nblk;
    for (unsigned k = lane; k < nblk * 8; k += kWave) coef[k] = make_uint4(0, 0, 0, 0);
    uint8_t comp_of[kMaxBlocksPerMcu];
    int bpm;
    block_components(f.ncomp, f.hs, f.vs, comp_of, &bpm);
    const ProgRingSrc src{reinterpret_cast<const unsigned char *>(s_ring)};
    int zz[8];                                                                 // a lane always moves the same eighth of a block: where its coefficients stand in LDS
#pragma unroll
    for (int i = 0; i < 8; ++i) zz[i] = natural_to_zigzag((lane & 7) * 8 + i);
    unsigned st = ST_OK;
    for (unsigned s = 0; s < f.nscan && st == ST_OK; ++s) {
        const ScanDesc sc = p.scans[f.scan0 + s];
        __syncthreads();                                                       // lane 0 is done with the last scan's tables; the zeroing has landed
        const unsigned ntab = sc.ntab < 4 ? sc.ntab : 4;
        const uint4 *tab = reinterpret_cast<const uint4 *>(p.ptables + sc.table0);
        for (unsigned k = lane; k < ntab * (sizeof(HuffTable) / 16); k += kWave) s_tab[k] = tab[k];
        const unsigned bpu = sc.ncomp > 1 ? (unsigned)bpm : 1u, per_stage = kStage / bpu;
        unsigned long long filled = sc.begin & ~15ull;
        ScanState state{};
        for (unsigned g = 0; g < sc.nseg && st == ST_OK; ++g) {
            const SegDesc sg = p.psegs[sc.seg0 + g];
            BitReader<ProgRingSrc> br(src, sg.begin, sg.end);
            state = ScanState{};
            unsigned long long pos = sg.begin;
            for (unsigned u0 = 0; u0 < sg.nmcu; u0 += per_stage) {
                const unsigned nu = sg.nmcu - u0 < per_stage ? sg.nmcu - u0 : per_stage, nb = nu * bpu;
                unsigned long long want = pos + (unsigned long long)nb * kBlockBytesBound;
                if (want > sg.end) want = sg.end;
                while (filled < want) {
                    const unsigned long long off = filled + (unsigned long long)lane * 16;
                    if (off + 16 <= p.bytes) s_ring[(off >> 4) & (kProgRing / 16 - 1)] = *reinterpret_cast<const uint4 *>(p.blob + off);
                    filled += kWave * 16;
                }
                const unsigned first = (sg.mcu0 + u0) * bpu;
                for (unsigned k = lane; k < nb * 8; k += kWave) {
                    const unsigned at = prog_block_index(f, sc, first + (k >> 3));
                    if (at < nblk) {
                        const uint4 v = coef[(size_t)at * 8 + (k & 7)];
                        const unsigned w[4] = {v.x, v.y, v.z, v.w};
                        short *blk = s_blk + (k >> 3) * 64;
#pragma unroll
                        for (int i = 0; i < 8; ++i) blk[zz[i]] = (short)(w[i >> 1] >> (16 * (i & 1)));
                    }
                }
                __syncthreads();
                if (lane == 0) {
                    unsigned r = prog_units<ZigzagOrder>(br, sc, reinterpret_cast<const HuffTable *>(s_tab), comp_of, (int)bpu, state, s_blk, nu);
                    if (r == ST_OK && u0 + nu == sg.nmcu) {
                        if (!br.drained()) r = ST_CORRUPT;
                        else if (g + 1 == sc.nseg && state.eobrun) r = ST_CORRUPT;     // a run that reaches past the scan's last block
                    }
                    s_st = r;
                    s_pos = br.pos;
                }
                __syncthreads();
                st = s_st;
                pos = s_pos;
                if (st != ST_OK) break;
                for (unsigned k = lane; k < nb * 8; k += kWave) {
                    const unsigned at = prog_block_index(f, sc, first + (k >> 3));
                    if (at < nblk) {
                        const short *blk = s_blk + (k >> 3) * 64;
                        unsigned w[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) w[i] = (unsigned)(unsigned short)blk[zz[2 * i]] | ((unsigned)(unsigned short)blk[zz[2 * i + 1]] << 16);
                        coef[(size_t)at * 8 + (k & 7)] = make_uint4(w[0], w[1], w[2], w[3]);
                    }
                }
            }
        }
    }
    if (st != ST_OK && lane == 0) atomicCAS(p.status + fi, 0u, st);
}

// ---- stage 2: jidctint.c jpeg_idct_islow on one block per thread.
// The library Pillow ships runs this transform in 16-bit SIMD lanes (jidctint-sse2 / -avx2): in0 +- in4, in7 + in3 and in5 + in1 are 16-bit adds,
// each pass packs its output to int16 with saturation, and the final pack to bytes saturates where the C code's range table wraps (|x| >= 512).
// Inside those lanes the SIMD code and the C code give the same samples, and no file an encoder writes leaves them; a block that does is the
// RANGE status (`wide`), like a dequantised product outside int16: it is refused, not given pixels that differ from Pillow's.
constexpr int kIdctThreads = 128;

__device__ __forceinline__ bool fits16(long long v) { return v >= -32768 && v <= 32767; }

__device__ __forceinline__ void idct_1d(const long long in[8], long long out[8], int shift, bool &wide)
{
    wide |= !(fits16(in[0] + in[4]) && fits16(in[0] - in[4]) && fits16(in[7] + in[3]) && fits16(in[5] + in[1]));
    long long z2 = in[2], z3 = in[6];
    long long z1 = (z2 + z3) * 4433;
    long long tmp2 = z1 + z3 * (-15137);
    long long tmp3 = z1 + z2 * 6270;
    z2 = in[0];
    z3 = in[4];
    long long tmp0 = (z2 + z3) * 8192;
    long long tmp1 = (z2 - z3) * 8192;
    const long long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7];
    tmp1 = in[5];
    tmp2 = in[3];
    tmp3 = in[1];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    long long z4 = tmp1 + tmp3;
    const long long z5 = (z3 + z4) * 9633;
    tmp0 *= 2446;
    tmp1 *= 16819;
    tmp2 *= 25172;
    tmp3 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * (-16069) + z5;
    z4 = z4 * (-3196) + z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    const long long r = 1ll << (shift - 1);
    out[0] = (tmp10 + tmp3 + r) >> shift;
    out[7] = (tmp10 - tmp3 + r) >> shift;
    out[1] = (tmp11 + tmp2 + r) >> shift;
    out[6] = (tmp11 - tmp2 + r) >> shift;
    out[2] = (tmp12 + tmp1 + r) >> shift;
    out[5] = (tmp12 - tmp1 + r) >> shift;
    out[3] = (tmp13 + tmp0 + r) >> shift;
    out[4] = (tmp13 - tmp0 + r) >> shift;
}

// libjpeg's range table (jdmaster.c prepare_range_limit_table), indexed by x & 1023
__device__ __forceinline__ unsigned range_limit(long long v)
{
    const unsigned x = (unsigned)v & 1023u;
    return x < 128 ? x + 128 : x < 512 ? 255u : x < 896 ? 0u : x - 896;
}

__global__ __launch_bounds__(kIdctThreads) void jpegdec_idct(Params p)
{
    const unsigned fi = blockIdx.y;
    const FileDesc &f = p.files[fi];
    const unsigned g = blockIdx.x * kIdctThreads + threadIdx.x;
    if (g >= f.nblk || p.status[fi] != ST_OK) return;
    const unsigned mcu = g / f.bpm, k = g - mcu * f.bpm;
    const unsigned mx = mcu % f.mcux, my = mcu / f.mcux;
    unsigned c, bx, by;
    if (f.ncomp == 1 || k >= f.hs * f.vs) {
        c = f.ncomp == 1 ? 0 : 1 + (k - f.hs * f.vs);
        bx = mx;
        by = my;
    } else {
        c = 0;
        bx = mx * f.hs + k % f.hs;
        by = my * f.vs + k / f.hs;
    }
    const uint4 *src = reinterpret_cast<const uint4 *>(p.coef + (f.coef_off + g) * 64);
    int v[64];
    bool range = false;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const uint4 w = src[r];
        const unsigned ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int coef = (short)(ww[j >> 1] >> (16 * (j & 1)));
            const int d = coef * (int)f.q[c][r * 8 + j];
            range |= d < -32768 || d > 32767;
            v[r * 8 + j] = d;
        }
    }
    long long ws[64];
#pragma unroll
    for (int x = 0; x < 8; ++x) {                                              // pass 1: columns, descaled by CONST_BITS - PASS1_BITS
        long long in[8], out[8];
#pragma unroll
        for (int y = 0; y < 8; ++y) in[y] = v[y * 8 + x];
        idct_1d(in, out, 11, range);
#pragma unroll
        for (int y = 0; y < 8; ++y) {
            range |= !fits16(out[y]);
            ws[y * 8 + x] = out[y];
        }
    }
    unsigned char *dst = p.planes + f.plane_off[c] + ((size_t)by * 8) * f.plane_w[c] + (size_t)bx * 8;
#pragma unroll
    for (int y = 0; y < 8; ++y) {                                              // pass 2: rows, descaled by CONST_BITS + PASS1_BITS + 3
        long long out[8];
        idct_1d(ws + y * 8, out, 18, range);
        unsigned lo = 0, hi = 0;
#pragma unroll
        for (int x = 0; x < 8; ++x) range |= out[x] < -512 || out[x] > 511;
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            lo |= range_limit(out[x]) << (8 * x);
            hi |= range_limit(out[x + 4]) << (8 * x);
        }
        *reinterpret_cast<uint2 *>(dst + (size_t)y * f.plane_w[c]) = make_uint2(lo, hi);
    }
    if (range) atomicCAS(p.status + fi, 0u, (unsigned)ST_RANGE);           // stage 3 then leaves the file's output alone
}

// ---- stage 3: jdsample.c + jdcolor.c, one thread per pixel
constexpr int kStoreThreads = 256;

// the chroma sample of output pixel (x, y): plane cropped to dw x dh, mode by the luma sampling factors
__device__ __forceinline__ int chroma_at(const unsigned char *pl, unsigned stride, unsigned hs, unsigned vs, int dw, int dh, int x, int y)
{
    if (hs == 1) return pl[(size_t)y * stride + x];
    const int cx = x >> 1;
    if (vs == 1) {                                                             // h2v1
        const unsigned char *row = pl + (size_t)y * stride;
        const int s = row[cx];
        if (dw <= 2) return s;                                                 // the narrow-image rule: h2v1_upsample
        if (x & 1) return cx == dw - 1 ? s : (3 * s + row[cx + 1] + 2) >> 2;
        return cx == 0 ? s : (3 * s + row[cx - 1] + 1) >> 2;
    }
    const int cy = y >> 1;                                                     // h2v2
    const unsigned char *near = pl + (size_t)cy * stride;
    if (dw <= 2) return near[cx];                                              // h2v2_upsample
    int fy = (y & 1) ? cy + 1 : cy - 1;
    fy = fy < 0 ? 0 : fy > dh - 1 ? dh - 1 : fy;
    const unsigned char *far = pl + (size_t)fy * stride;
    const int s = 3 * near[cx] + far[cx];
    if (x & 1) return cx == dw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * near[cx + 1] + far[cx + 1] + 7) >> 4;
    return cx == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * near[cx - 1] + far[cx - 1] + 8) >> 4;
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

__global__ __launch_bounds__(kStoreThreads) void jpegdec_store(Params p)
{
    const unsigned fi = blockIdx.y;
    const FileDesc &f = p.files[fi];
    const unsigned g = blockIdx.x * kStoreThreads + threadIdx.x;
    if (g >= f.width * f.height || p.status[fi] != ST_OK) return;
    const int x = g % f.width, y = g / f.width;
    int px[3];
    px[0] = p.planes[f.plane_off[0] + (size_t)y * f.plane_w[0] + x];
    if (f.ncomp == 3) {
        const int dw = (f.width + f.hs - 1) / f.hs, dh = (f.height + f.vs - 1) / f.vs;
        const int cb = chroma_at(p.planes + f.plane_off[1], f.plane_w[1], f.hs, f.vs, dw, dh, x, y) - 128;
        const int cr = chroma_at(p.planes + f.plane_off[2], f.plane_w[2], f.hs, f.vs, dw, dh, x, y) - 128;
        const int yy = px[0];
        // FIX(1.402) = 91881, FIX(1.772) = 116130, FIX(0.34414) = 22554, FIX(0.71414) = 46802
        px[0] = clamp255(yy + ((91881 * cr + 32768) >> 16));
        px[1] = clamp255(yy + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
        px[2] = clamp255(yy + ((116130 * cb + 32768) >> 16));
    }
    lspout::store_pixel(f.form, f.out_ptr, f.table_ptr, f.plane_stride, f.ncomp, g, px);
}

void fill_info(const Parsed &f, uint32_t status, uint32_t nseg, uint64_t scan_end, lspjpeg_dec_info *info)
{
    *info = lspjpeg_dec_info{};
    info->status = (int32_t)status;
    info->width = (int32_t)f.width;
    info->height = (int32_t)f.height;
    info->components = (int32_t)f.ncomp;
    info->hsamp = (int32_t)f.hs;
    info->vsamp = (int32_t)f.vs;
    info->restart_interval = (int32_t)f.restart;
    if (status != ST_OK) return;
    info->mcus = (int32_t)mcu_count(f);
    info->segments = (int32_t)nseg;
    for (uint32_t c = 0; c < f.ncomp; ++c) {
        if (!f.huff_seen[0][f.dc_sel[c]]) info->default_tables |= 1 << (2 * f.dc_sel[c]);
        if (!f.huff_seen[1][f.ac_sel[c]]) info->default_tables |= 1 << (2 * f.ac_sel[c] + 1);
    }
    info->scan_offset = f.scan_begin;
    info->scan_bytes = scan_end - f.scan_begin;
}

void fill_info_progressive(const ProgFile &f, uint32_t status, lspjpeg_dec_info *info)
{
    *info = lspjpeg_dec_info{};
    info->status = (int32_t)status;
    info->width = (int32_t)f.width;
    info->height = (int32_t)f.height;
    info->components = (int32_t)f.ncomp;
    info->hsamp = (int32_t)f.hs;
    info->vsamp = (int32_t)f.vs;
    info->restart_interval = (int32_t)f.restart0;
    if (status != ST_OK) return;
    info->mcus = (int32_t)(((f.width + 8 * f.hs - 1) / (8 * f.hs)) * ((f.height + 8 * f.vs - 1) / (8 * f.vs)));
    info->segments = (int32_t)f.nseg;
    info->scan_offset = f.data_begin;
    info->scan_bytes = f.data_end - f.data_begin;
}

}  // namespace

extern "C" {

const char *lspjpeg_dec_last_error(void) { return g_err.c_str(); }

int lspjpeg_dec_probe(const unsigned char *bytes, size_t len, lspjpeg_dec_info *info) { return lspjpeg_dec_probe_flags(bytes, len, 0u, info); }

int lspjpeg_dec_probe_flags(const unsigned char *bytes, size_t len, unsigned flags, lspjpeg_dec_info *info)
{
    if (!bytes || !info) return fail(LSPJPEG_DEC_ERR_INVALID_ARGUMENT, "null argument");
    if (flags & ~(LSPJPEG_DEC_FLAG_PROGRESSIVE | LSPJPEG_DEC_FLAG_PARALLEL)) return fail(LSPJPEG_DEC_ERR_INVALID_ARGUMENT, "unknown flag");
    Parsed f;
    ProgFile pf;
    uint32_t nseg;
    uint64_t end;
    bool prog;
    const uint32_t st = examine_flags(bytes, len, LSPJPEG_MAX_SIDE, flags, &f, &nseg, &end, &pf, &prog);
    if (prog)
        fill_info_progressive(pf, st, info);
    else
        fill_info(f, st, nseg, end, info);
    return LSPJPEG_DEC_OK;
}

int64_t lspjpeg_dec_plan(const unsigned char *const *files, const size_t *lens, const lspjpeg_dec_output *outs, int n, int max_side, void *blob,
                         size_t cap)
{
    return lspjpeg_dec_plan_flags(files, lens, outs, n, max_side, 0u, blob, cap);
}

int64_t lspjpeg_dec_plan_flags(const unsigned char *const *files, const size_t *lens, const lspjpeg_dec_output *outs, int n, int max_side, unsigned flags,
                               void *blob, size_t cap)
{
    if (flags & ~(LSPJPEG_DEC_FLAG_PROGRESSIVE | LSPJPEG_DEC_FLAG_PARALLEL)) return fail(LSPJPEG_DEC_ERR_INVALID_ARGUMENT, "unknown flag");
    if (!files || !lens || n < 1 || n > 65535) return fail(LSPJPEG_DEC_ERR_INVALID_ARGUMENT, "files, lens and 1..65535 files are required");
    if (max_side < 1 || max_side > LSPJPEG_MAX_SIDE) return fail(LSPJPEG_DEC_ERR_INVALID_ARGUMENT, "max_side must be in 1.." + std::to_string(LSPJPEG_MAX_SIDE));
    for (int i = 0; i < n; ++i)
        if (!files[i]) return fail(LSPJPEG_DEC_ERR_INVALID_ARGUMENT, "file " + std::to_string(i) + " is null");
    const int64_t need = plan(files, lens, nullptr, n, (uint32_t)max_side, nullptr, flags);
    if (need < 0) return fail(LSPJPEG_DEC_ERR_INVALID_ARGUMENT, "the batch needs a descriptor block of 4 GiB or more: split it");
    if (!blob) return need;
    if (cap < (size_t)need || reinterpret_cast<uintptr_t>(blob) % 16)
        return fail(LSPJPEG_DEC_ERR_INVALID_ARGUMENT, "blob must be 16-byte aligned and hold " + std::to_string(need) + " bytes");
    std::vector<OutputDesc> od(outs ? (size_t)n : 0);
    if (outs) lspout::describe_outputs(outs, n, od.data());
    const int64_t got = plan(files, lens, outs ? od.data() : nullptr, n, (uint32_t)max_side, blob, flags);
    if (got == -1) return fail(LSPJPEG_DEC_ERR_INVALID_ARGUMENT, lspout::kOutputRefusal);
    return got;
}

int lspjpeg_dec_summary_of(const void *blob, lspjpeg_dec_summary *out)
{
    const BlobHeader *h = header_of(blob);
    if (!h || !out) return fail(LSPJPEG_DEC_ERR_INVALID_ARGUMENT, "not a descriptor block of lspjpeg_dec_plan");
    out->files = h->nfiles;
    out->segments = h->nsegs;
    out->max_blocks = h->max_blocks;
    out->max_pixels = h->max_pixels;
    out->total_blocks = h->total_blocks;
    out->bytes = h->bytes;
    out->workspace_bytes = h->workspace_bytes;
    out->status_offset = h->status_off;
    return LSPJPEG_DEC_OK;
}

int lspjpeg_dec_plan_file(const void *blob, int i, lspjpeg_dec_info *info)
{
    const BlobHeader *h = header_of(blob);
    if (!h || !info || i < 0 || (uint32_t)i >= h->nfiles) return fail(LSPJPEG_DEC_ERR_INVALID_ARGUMENT, "no such file in the block");
    const FileDesc &d = files_of(blob)[i];
    *info = lspjpeg_dec_info{};
    info->status = (int32_t)d.status;
    if (d.status != ST_OK) return LSPJPEG_DEC_OK;
    info->width = (int32_t)d.width;
    info->height = (int32_t)d.height;
    info->components = (int32_t)d.ncomp;
    info->hsamp = (int32_t)d.hs;
    info->vsamp = (int32_t)d.vs;
    info->restart_interval = (int32_t)d.restart;
    info->mcus = (int32_t)(d.mcux * d.mcuy);
    if (d.progressive) {                                                       // every restart interval of every scan; the data from the first scan's up to the EOI
        const ScanDesc *sc = scans_of(blob) + d.scan0;
        for (uint32_t k = 0; k < d.nscan; ++k) info->segments += (int32_t)sc[k].nseg;
        info->scan_offset = sc[0].begin;
        info->scan_bytes = sc[d.nscan - 1].end - sc[0].begin;
        return LSPJPEG_DEC_OK;
    }
    info->segments = (int32_t)d.nseg;
    const SegDesc *s = segs_of(blob) + d.seg0;
    info->scan_offset = s[0].begin;
    info->scan_bytes = s[d.nseg - 1].end - s[0].begin;
    return LSPJPEG_DEC_OK;
}

int lspjpeg_dec_plan_scans(const void *blob, int i)
{
    const BlobHeader *h = header_of(blob);
    if (!h || i < 0 || (uint32_t)i >= h->nfiles) return fail(LSPJPEG_DEC_ERR_INVALID_ARGUMENT, "no such file in the block");
    const FileDesc &d = files_of(blob)[i];
    return d.status == ST_OK && d.progressive ? (int)d.nscan : 0;
}

int lspjpeg_dec_plan_scan(const void *blob, int i, int s, lspjpeg_dec_scan *out)
{
    const BlobHeader *h = header_of(blob);
    if (!h || !out || i < 0 || (uint32_t)i >= h->nfiles) return fail(LSPJPEG_DEC_ERR_INVALID_ARGUMENT, "no such file in the block");
    const FileDesc &d = files_of(blob)[i];
    if (d.status != ST_OK || !d.progressive || s < 0 || (uint32_t)s >= d.nscan) return fail(LSPJPEG_DEC_ERR_INVALID_ARGUMENT, "no such scan of the file");
    const ScanDesc &sc = scans_of(blob)[d.scan0 + s];
    *out = lspjpeg_dec_scan{};
    out->components = sc.ncomp;
    for (int j = 0; j < 4; ++j) {
        out->component[j] = sc.comp[j];
        out->dc_table[j] = sc.td[j];
        out->ac_table[j] = sc.ta[j];
    }
    out->ss = sc.ss;
    out->se = sc.se;
    out->ah = sc.ah;
    out->al = sc.al;
    out->restart_interval = (int32_t)sc.restart;
    out->units = (int32_t)sc.units;
    out->segments = (int32_t)sc.nseg;
    out->begin = sc.begin;
    out->end = sc.end;
    return LSPJPEG_DEC_OK;
}

int lspjpeg_dec_plan_qtable(const void *blob, int i, int c, uint16_t out[64])
{
    const BlobHeader *h = header_of(blob);
    if (!h || !out || i < 0 || (uint32_t)i >= h->nfiles || c < 0 || c > 2) return fail(LSPJPEG_DEC_ERR_INVALID_ARGUMENT, "no such table in the block");
    for (int k = 0; k < 64; ++k) out[k] = files_of(blob)[i].q[c][k];
    return LSPJPEG_DEC_OK;
}

int lspjpeg_dec_plan_segment(const void *blob, int k, uint32_t *file, uint32_t *mcu0, uint32_t *nmcu, uint64_t *begin, uint64_t *end)
{
    const BlobHeader *h = header_of(blob);
    if (!h || k < 0 || (uint32_t)k >= h->nsegs || !file || !mcu0 || !nmcu || !begin || !end)
        return fail(LSPJPEG_DEC_ERR_INVALID_ARGUMENT, "no such segment in the block");
    const SegDesc &s = segs_of(blob)[k];
    *file = s.file;
    *mcu0 = s.mcu0;
    *nmcu = s.nmcu;
    *begin = s.begin;
    *end = s.end;
    return LSPJPEG_DEC_OK;
}

int lspjpeg_dec_host_coefficients(const void *blob, int i, int16_t *out, size_t cap_values)
{
    const BlobHeader *h = header_of(blob);
    if (!h || !out || i < 0 || (uint32_t)i >= h->nfiles) return fail(LSPJPEG_DEC_ERR_INVALID_ARGUMENT, "no such file in the block");
    if (cap_values < (size_t)files_of(blob)[i].nblk * 64) return fail(LSPJPEG_DEC_ERR_INVALID_ARGUMENT, "out is too small for the file's blocks");
    g_par_stats = ParStats{};
    return (int)host_coefficients(blob, i, out, &g_par_stats);
}

int lspjpeg_dec_plan_parallel(const void *blob, int k, uint32_t *subseq_bytes, uint32_t *subsequences)
{
    const BlobHeader *h = header_of(blob);
    if (!h || k < 0 || (uint32_t)k >= h->nsegs || !subseq_bytes || !subsequences) return fail(LSPJPEG_DEC_ERR_INVALID_ARGUMENT, "no such segment in the block");
    if (!h->parallel) return fail(LSPJPEG_DEC_ERR_INVALID_ARGUMENT, "the block was planned without LSPJPEG_DEC_FLAG_PARALLEL");
    const SegDesc &s = segs_of(blob)[k];
    *subseq_bytes = kSubseqBytes;
    *subsequences = subsequences_of(s.begin, s.end);
    return LSPJPEG_DEC_OK;
}

int lspjpeg_dec_host_parallel_stats(uint32_t *rounds, uint32_t *midblock_entries)
{
    if (!rounds || !midblock_entries) return fail(LSPJPEG_DEC_ERR_INVALID_ARGUMENT, "null argument");
    *rounds = g_par_stats.rounds;
    *midblock_entries = g_par_stats.midblock;
    return LSPJPEG_DEC_OK;
}

int lspjpeg_dec_decode(const void *blob_host, void *blob_dev, void *workspace_dev, size_t workspace_bytes, void *hip_stream)
{
    const BlobHeader *h = header_of(blob_host);
    if (!h || !blob_dev || !workspace_dev) return fail(LSPJPEG_DEC_ERR_INVALID_ARGUMENT, "a planned block, its device copy and a workspace are required");
    if (!h->has_outputs) return fail(LSPJPEG_DEC_ERR_INVALID_ARGUMENT, "the block was planned without outputs (host only)");
    if (reinterpret_cast<uintptr_t>(blob_dev) % 16 || reinterpret_cast<uintptr_t>(workspace_dev) % 256)
        return fail(LSPJPEG_DEC_ERR_INVALID_ARGUMENT, "blob_dev must be 16-byte aligned and workspace_dev 256-byte aligned");
    if (workspace_bytes < h->workspace_bytes) return fail(LSPJPEG_DEC_ERR_INVALID_ARGUMENT, "workspace needs " + std::to_string(h->workspace_bytes) + " bytes");
    unsigned char *b = static_cast<unsigned char *>(blob_dev);
    Params p{};
    p.blob = b;
    p.files = reinterpret_cast<const FileDesc *>(b + h->files_off);
    p.segs = reinterpret_cast<const SegDesc *>(b + h->segs_off);
    p.tables = reinterpret_cast<const HuffTable *>(b + h->tables_off);
    p.status = reinterpret_cast<unsigned *>(b + h->status_off);
    p.coef = static_cast<short *>(workspace_dev);
    p.planes = static_cast<unsigned char *>(workspace_dev) + h->planes_ws_off;
    p.nfiles = h->nfiles;
    p.nsegs = h->nsegs;
    p.bytes = h->bytes;
    p.scans = reinterpret_cast<const ScanDesc *>(b + h->scans_off);
    p.psegs = reinterpret_cast<const SegDesc *>(b + h->psegs_off);
    p.ptables = reinterpret_cast<const HuffTable *>(b + h->ptables_off);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const auto grid = [](unsigned items, unsigned per) { return items ? (items + per - 1) / per : 1u; };     // a batch of refused files still launches
    if (h->parallel)
        hipLaunchKernelGGL(jpegdec_entropy_parallel, dim3(grid(h->nsegs, 1)), dim3(kParLanes), 0, st, p);
    else
        hipLaunchKernelGGL(jpegdec_entropy, dim3(grid(h->nsegs, 1)), dim3(kWave), 0, st, p);
    if (h->nprog) hipLaunchKernelGGL(jpegdec_progressive, dim3(h->nfiles), dim3(kWave), 0, st, p);     // the files of the two kinds are disjoint
    hipLaunchKernelGGL(jpegdec_idct, dim3(grid(h->max_blocks, kIdctThreads), h->nfiles), dim3(kIdctThreads), 0, st, p);
    hipLaunchKernelGGL(jpegdec_store, dim3(grid(h->max_pixels, kStoreThreads), h->nfiles), dim3(kStoreThreads), 0, st, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(LSPJPEG_DEC_ERR_HIP, std::string("jpeg decode launch: ") + hipGetErrorString(e));
    return LSPJPEG_DEC_OK;
}

}  // extern "C"
