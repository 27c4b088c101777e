// Static execution plan of the feature2face generator: the residual U-Net unrolled into a flat
// list of fused conv launches, the expected state-dict tensors, the packed-weight blob layout
// and the liveness-based workspace layout.  Host-only C++ (no HIP types).
//
// Reference structure restated: models/networks.py:554-572 (large) / 458-476 (normal) build the
// nest; :592-640 (and :496-544) order each level's nn.Sequential; :650-675 ResidualBlock.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

namespace lspf2f {

enum LayerKind { kFirstConv = 0, kIgemm = 1, kLastConv = 2 };
// InstanceNorm plans, per layer and batch: kInFused = sums in the igemm epilogue (wave shuffles), kInReduce = a streaming pass
// that also folds the split-K partials, kInSmall = one workgroup per (frame, 32 channels) does statistics + normalisation
enum InRoute { kInNone = 0, kInFused = 1, kInReduce = 2, kInSmall = 3, kInWino = 4 };   // kInWino: sums in the Winograd kernel's epilogue (per tile-block of 128 pixels)

struct TensorDesc {        // an activation tensor in the workspace (NHWC)
    std::string name;
    int c = 0, h = 0;      // channels, spatial extent (square)
    int def = -1;          // index of the producing layer
    int last_use = -1;     // index of the last consuming layer
    size_t offset = 0;     // byte offset in the workspace for the planned batch
};

// which kernel runs a conv layer of the net body (LayerKind kIgemm) at the planned batch.  Exactly one per layer: choose_route() (plan.cpp) is
// the only place that decides, run_layer / kernel_name (api.cpp) and route_form() switch on it
enum ConvRoute { kRouteIgemm, kRouteSmallM, kRouteFullK, kRouteFullK16, kRouteWino, kRouteWino4, kRouteWinoUp,
                 kRouteRowUp, kRouteRowConv, kRouteBand, kRoutePatch16, kRoutePatchUp16 };
// the layouts a layer's weights can be packed in; the values are the ids of lspf2f_layer_form_offset() (include/lspf2f.h, _native.FORM_IDS)
enum WeightForm {
    kFormRows = 0,      // [co][tap][ci] rows of the implicit GEMM (sub-pixel rows for up4 / the last conv, [ci][tap][co] for the first conv)
    kFormFullK = 1,     // the tile-blocked layout of the full-K kernels (fullk.hip fp32, fullk16.hip 16-bit)
    kFormFullK2 = 2,    // fp32: the same with a single source packed as two half-sources (the K-split form and the stride-2 convs)
    kFormWino = 3,      // G g G^T in the fragment order of wino.hip
    kFormWino4 = 4,     // the 6x6 G g G^T in the order of the F(4x4,3x3) kernel (wino4.hip)
    kFormWinoUp = 5,    // the 9 transformed taps in the fragment order of winoup.hip
    kFormRowUp = 6,     // 16-bit: fragment order of rowup256 (rowconv.hip)
    kFormBand = 7,      // 16-bit: fragment order of bandconv.hip
    kFormRow = 8,       // 16-bit: fragment order of the weights-stationary kernels (rowconv.hip)
    kFormGemmLast = 9,  // 16-bit, last conv: the sub-pixel weights as a 9-tap [4*cout][3][3][cin] GEMM operand
    kFormRowLast = 10,  // 16-bit, last conv over two 64-channel sources: that operand in the fragment order of rowlast128 (rowconv.hip)
    kNumForms
};

struct LayerDesc {
    std::string name;
    LayerKind kind = kIgemm;
    int src0 = -1, src1 = -1, res = -1, out = -1;   // TensorDesc ids (-1: none / API tensor)
    int cin = 0, c0 = 0, c1 = 0, cout = 0;
    int hs = 0;            // spatial extent of the tensor(s) read
    int ho = 0;            // spatial extent written
    int stride = 1;
    bool up = false, relu = false, tanh_out = false, concat = false, residual = false;
    bool up4 = false;      // upsample conv executed in sub-pixel form (4 parities x 2x2 taps)
    std::string wkey;      // state-dict key of the OIHW weight
    std::string bnkey;     // state-dict prefix of the following BatchNorm2d ("" = none)
    std::string biaskey;   // state-dict key of the conv bias ("" = none; InstanceNorm plans: the level convs, networks.py:590)
    bool inorm = false;    // an InstanceNorm2d (affine=False, eps 1e-5) follows the conv: per-(frame, channel) statistics at run time
    int in_route = 0;      // per-batch: how those statistics are gathered (kInFused / kInReduce / kInSmall)
    int64_t form_off[kNumForms] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};   // byte offsets in the packed blob (-1: this handle's blob does not carry the form)
    int64_t scale_off = -1, shift_off = -1;
    // per-batch decision (choose_route)
    ConvRoute route = kRouteIgemm;
    int route_arg = 0;     // SmallM 1 | FullK, FullK16: 16-pixel blocks per tile | Wino, WinoUp: 32-channel blocks per wave | Wino4 1 | RowUp: low-res rows per strip |
                           // RowConv: output rows per strip | Band 1 | Patch16, PatchUp16: tile width in pixels
    int bm = 0, bn = 0, splits = 1, group = 1;   // the route's tile; splits = its K splits; group = K-tiles per pipeline step
    bool fused_splitk = false;   // fp32 plans: 2..8 K-splits combined inside the igemm launch by the last-arriving workgroup (no splitk_reduce
                                 // launch): +1.0 % at fp32 batch 1, none at batch 8, -2.4 % on bf16 batch 8 (A-B-A-B, one session; restricted
                                 // to the <= 16x16 / <= 8x8 levels of a bf16 plan it still loses 0.7-0.9 %)
};
// the weight form the kernel of a (batch-planned) layer reads
inline WeightForm route_form(const LayerDesc &l)
{
    switch (l.route) {
    case kRouteFullK: return (l.stride == 2 || (l.splits == 2 && !l.c1)) ? kFormFullK2 : kFormFullK;
    case kRouteFullK16: return kFormFullK;
    case kRouteWino: return kFormWino;
    case kRouteWino4: return kFormWino4;
    case kRouteWinoUp: return kFormWinoUp;
    case kRouteRowUp: return kFormRowUp;
    case kRouteBand: return kFormBand;
    case kRouteRowConv: return kFormRow;
    case kRouteIgemm: case kRouteSmallM: case kRoutePatch16: case kRoutePatchUp16: break;
    }
    return kFormRows;
}

struct ParamDesc {         // an expected state-dict entry
    std::string key;
    std::vector<int64_t> dims;
    std::vector<float> data;
    bool set = false;
    size_t numel() const { size_t n = 1; for (auto d : dims) n *= (size_t)d; return n; }
};

struct Plan {
    int variant = 1, nres = 2, input_nc = 13, feat_nc = 1, output_nc = 3, ngf = 64, num_downs = 8, size = 512;
    bool keep_intermediates = false;
    int dtype = 0;             // 0: fp32 activations + weights; 1: bf16 storage (fp32 accumulate), first/last-layer weights fp32; 2: fp16 storage, likewise
                               // (the reference's opt.fp16 / autocast configuration; the row / band / up-conv kernels of the 16-bit plans are templated on
                               // the storage type, so an fp16 plan takes the same kernel per layer as the bf16 plan)
    int norm = 0;              // 0: BatchNorm2d in eval mode (folded, the shipped checkpoints); 1: InstanceNorm2d (norm_layer argument
                               // of the reference constructors, networks.py:555 / :459): conv biases on, statistics at run time, fp32 only
    int fullk16_levels = 3;    // 16-bit plans: which small levels run on the full-K kernel (fullk16.hip; tune key `fullk16`, bit mask as in fullk16_choice(), plan.cpp; 0 = none)
    int fullk16_min_frames = 2; // ... from this many frames up (tune key `fullk16_min_frames`)
    bool use_bandconv = true;  // bf16 plans: tune key `bandconv=0` puts the 16x16 / 8x8 layers back on the implicit GEMM (A-B runs)
    int bandconv_min_blocks = 128;  // (16x16 / 8x8 levels; the 4x4 / 2x2 levels, one tile per 2 / 8 frames, have their own bound below)
    int bandconv_min_frames_small = 1 << 30;   // 4x4 / 2x2 levels (a tile = 2 / 8 whole frames): never by default -- at 8 frames the 64 / 16
                                               // workgroups of such a launch lose to the igemm (normal 4460 -> 4388, large 2881 -> 2840 frames/s,
                                               // A-B-A-B); tune key `bandconv_min_frames` lowers it for measurements at larger batches   // ... and they only leave it when the launch has at least this many workgroups
    bool use_patch16 = true;   // 16-bit plans: tune key `patch16=0` keeps the stride-1 convs of the 64x64 / 32x32 levels on the implicit GEMM (A-B runs)
    bool use_patchup16 = true; // ... and `patchup16=0` the sub-pixel up-convs over 32x32 / 64x64 sources (conv3x3_patchup16)
    int patch16_deep = 1;      // ... and `patch16_deep=0` its 64-channel tiles in the first form (3-slot ring, copies in the load segment) instead of conv3x3_patch16d (A-B runs)
    int patch16_min_blocks = 192;   // ... which they only leave when the launch has at least this many workgroups (tune key `patch16_min_blocks`)
    bool use_rowup = true;     // bf16 plans: tune key `rowup=0` keeps L1.up on the implicit GEMM (A-B runs)
    bool rowlast_fused = true; // bf16 plans: rowlast128 applies pixel shuffle + tanh in its epilogue when only fp32 frames are wanted (tune key `rowlast_fused=0`: the two-launch form, A-B runs)
    bool use_rowlast = true;   // bf16 plans: tune key `rowlast=0` keeps the GEMM-form last conv on the implicit-GEMM kernel (A-B runs)
    int fullk_split_max_tiles = 128;   // tune key `fullk_split_tiles` (tools): 256 also splits the 16x16 layers at batch 1
    int use_fullk_s2 = 0;          // tune key `fullk_s2`: the stride-2 convs of the small levels at batch 1 on the K-split full-K kernel instead of the implicit
                                   // GEMM + split-K reduce: 1 = L4 / L5 / L6.down (16x16, 8x8, 4x4 outputs), 2 = only those writing <= 8x8 (L5 / L6.down).
                                   // Round 3 measured 1 as SLOWER for the whole forward although two of its three launches are shorter; round 4 found why
                                   // (tools/s2_layer_delta.py): L4.down itself loses 8 us and two far-away up-convs lose 9 us each
    bool use_fullk_split = true;   // the 8x8 layers at batch 1 run the full-K kernel with K in two halves over twice the workgroups (tune key `fullk_split=0` at
                                   // create: unsplit, A-B runs)
    bool use_wino = true;      // fp32 plans: stride-1 convs at >= 32x32 on the Winograd kernel (tune key `wino=0`: the implicit GEMM, A-B runs)
    bool use_wino4 = false;    // fp32 plans: ... and of those the layers choose_route() gives to the F(4x4,3x3) kernel (LSPF2F_FLAG_WINO4; measured slower at batch 1 and
                               // equal at batch 8, DESIGN.md 4.11, so off by default); decides whether the blob carries the 6x6 transformed weights
    int in_small_max_hw = 1024;  // `in_small_max_hw`: InstanceNorm plans take the one-launch route (in_small: one workgroup per (frame, 32 channels)) up to this many pixels per frame; above it
                                 // in_reduce_stats + in_finalize + in_apply spread the frame over the chip
    bool in_smallm_fused = true; // `in_smallm_fused`: InstanceNorm plans normalise in conv3x3_smallm's epilogue (a workgroup holds every pixel of its channels) instead of an in_small launch behind it
    bool in_wino_stats = true;   // `in_wino_stats`: InstanceNorm plans take a wino3x3 layer's statistics from its epilogue instead of a pass over its output
    int smallm_kb = 64;          // `smallm_kb`: largest input tensor (KB, fp32 in LDS) the tiny-M kernel takes.  64 until round 5; with LDS-DMA staging a 128-KB tensor (one workgroup per CU) is
                                 // one round of copies: L6.down (512 -> 512 at stride 2, 8x8 -> 4x4) leaves the 36-way split-K implicit GEMM + reduce launch at one frame
    int out_wt = 1;              // `out_wt`: wino3x3 / winoup3x3 write their output through (sc1 stores) instead of leaving it dirty in L2 for the end-of-kernel write-back: bit-identical, +0.6 % at batch 1, +0.3 % at batch 8, +1.0 % `normal` batch 1 (A-B-A-B x3, profiles/r05_outwt_ab.txt); 0 = plain stores
    bool fused_splitk16 = false; // `fused_splitk16`: 16-bit plans combine 2..8 K-splits inside the igemm launch like the fp32 plans do (off until measured: round 5)
    int wino_prio = 1;           // `wino_prio`: wino3x3<1>'s register form sets its wave priority by K-loop progress, the workgroup that is BEHIND leads (ProgressPrio, wino_common.h): bit-identical,
                                 // +0.7-0.85 % at batch 1 (two boxes, A-B-A-B x3 each), neutral at batch 8; 3 / 4..6 = the variants measured within 0.2 % of it (profiles/r05_wino_prio_ab.txt); 0 = off
    int wino_ureg = 1;           // `wino_ureg`: wino3x3<1> keeps its U fragments in registers (wino.hip UR form: three register sets, two steps ahead); 0 = through LDS
    bool wino_pre = true, wino_il = true, wino_rot = true;   // tools (`wino_pre` / `wino_il` / `wino_rot` of lspf2f_create_tuned): A-B switches of wino3x3
    int wino_xcd = -1, igemm_xcd = -1;                       // tools: forced block orders (-1 = by operand size)
    int winoup_nb = 0, winoup_target = 1024;   // tools (tune keys `winoup_nb` / `winoup_target`): force the channel blocks per wave / the workgroup count aimed at
    bool use_winoup = true;    // fp32 plans: sub-pixel up-convs on the up-conv Winograd kernel (tune key `winoup=0`: the implicit GEMM, A-B runs)
    bool use_rowconv = true;   // bf16 plans: 64 -> 64 layers on the weights-stationary kernel (tune key `rowconv=0`: the igemm, A-B runs)
    size_t elt() const { return dtype ? 2 : 4; }
    int ktile_channels() const { return dtype ? 64 : 32; }   // a K-tile is 128 B of channels
    bool layer_weights_typed(const LayerDesc &l) const { return l.kind == kIgemm; }   // else fp32
    // bf16: the last conv runs as an implicit GEMM on the low-res source (N = 4 parities x cout) + a pixel-shuffle/tanh pass
    bool last_as_gemm(const LayerDesc &l) const { return dtype != 0 && l.kind == kLastConv && l.cin % 64 == 0; }
    std::vector<LayerDesc> layers;
    std::vector<TensorDesc> tensors;
    std::vector<ParamDesc> params;
    std::map<std::string, int> param_index;
    size_t blob_bytes = 0;

    // per-batch state
    int planned_batch = 0;
    size_t act_bytes = 0;       // activation arena
    size_t partial_bytes = 0;   // split-K scratch
    size_t partial_offset = 0;
    size_t stats_bytes = 0;     // InstanceNorm plans: per-group sums and shifts [3][B][groups][C] + the finalised (mean, rstd) [2][B][C]
    size_t stats_offset = 0;
    int stats_groups_max = 0;
    // persistent region at workspace offset 0: pre-activation contribution of the candidate channels to the
    // first conv, [H/2][W/2][ngf] fp32 (constant per person: demo.py:89-95 builds img_candidates once)
    size_t cand_cache_bytes() const { return ((size_t)(size / 2) * (size / 2) * ngf * sizeof(float) + 255) / 256 * 256; }
    // head of the workspace: slot 0 = that per-person cache (lspf2f_set_candidates), slot 1 = the same quantity for a
    // candidate stack broadcast over ONE forward's batch (never aliases slot 0)
    // then kTileCounters arrival counters of the in-launch split-K combine (zero between launches; zeroed once per workspace binding)
    static const size_t kTileCounters = 16384;
    size_t counters_offset() const { return 2 * cand_cache_bytes(); }
    size_t persistent_bytes() const { return 2 * cand_cache_bytes() + kTileCounters * sizeof(unsigned); }

    // max_batch_forms > 0: the blob carries only the weight forms the plans of batch 1 .. max_batch_forms read (0: every form)
    std::string build(int variant, int input_nc, int feat_nc, int output_nc, int ngf, int num_downs,
                      int size, bool keep, int dtype = 0, int norm = 0, int max_batch_forms = 0);   // returns "" or an error message
    static unsigned forms_used(const LayerDesc &tiled, const Plan &p);   // bit mask (1u << WeightForm) of the forms the kernel(s) of a (batch-planned) layer read
    size_t form_bytes(const LayerDesc &l, WeightForm f) const;           // size of a layer's weights in that form
    void assign_offsets(const std::vector<unsigned> *used);               // lays the blob out with the forms of `used` (nullptr: every form)
    int blob_pad_kb = 0;           // tune key `blob_pad_kb` (tools): empty KB in front of the first layer's weights
    bool keep_all_forms = false;   // tune key `all_forms=1`: every form whatever the batch range (tests that look at forms other batches would use)
    void plan_batch(int batch);
    // the most frames one forward can run: every kernel addresses a tensor through 32-bit buffer offsets (top bit = out-of-range marker),
    // so the largest activation tensor of the plan must stay within 2 GiB - 1 at the batch (the implicit GEMM refuses its source past it,
    // igemm.hip launch_igemm; 8 MiB per frame at 512x512 in 16 bits: 255 frames).  `largest` (optional) receives that tensor's index.
    int max_frames(int *largest = nullptr) const;
    size_t workspace_bytes(int batch) const;   // without mutating the current plan
    std::string pack(void *blob, size_t bytes) const;   // "" or error
    int64_t layer_flops(const LayerDesc &l) const;
    int64_t layer_act_bytes(const LayerDesc &l) const;
};

// tile / split-K heuristic shared by the planner and lspf2f_conv3x3
void choose_tiling(int M, int N, int ktiles, int par, bool up9, int dtype, int *bm, int *bn, int *splits, int *group);
// InstanceNorm plans, implicit GEMM with epilogue sums (kInFused): the rows behind one wave's sums (32 per 32x32 tile row; bm / 2 for the
// 2x2-wave tiles) and the rule that lets a layer take that route -- a wave's rows must stay inside one frame, and the tiny levels do
// statistics + normalisation in one workgroup per channel slab instead.  rhw = pixels per frame of the GEMM's M space (the LOW-res frame of a
// sub-pixel up-conv).  Shared by the planner and lspf2f_conv3x3_instnorm.
inline int in_fused_wave_rows(int bm) { return bm == 32 ? 32 : bm / 2; }
inline bool in_fused_eligible(int bm, int splits, int rhw) { return splits == 1 && rhw >= 1024 && rhw % in_fused_wave_rows(bm) == 0; }

// Split-K scratch of one conv launch: fp32 partial slabs, then one arrival counter per tile the in-launch combine owns.  Each layout is stated here once:
// lspf2f_conv3x3_scratch_bytes sizes it, lspf2f_conv3x3 bounds-checks and binds it, and the planner's Winograd rules test the same tile-block counts against
// Plan::kTileCounters.
struct SplitKScratch {
    size_t slab_bytes, counters;
    size_t bytes() const { return slab_bytes + counters * sizeof(unsigned); }
};
inline size_t wino_tile_blocks(int batch, int h, int w) { return (size_t)batch * (h / 8) * (w / 16); }        // wino3x3: 8 x 16 output pixels
inline size_t wino4_tile_blocks(int batch, int h, int w) { return (size_t)batch * (h / 16) * (w / 32); }      // wino4_3x3: 16 x 32 output pixels
inline size_t winoup_tile_blocks(int batch, int hs, int ws) { return (size_t)batch * (hs / 4) * (ws / 8); }   // winoup3x3: 4 x 8 SOURCE pixels
// the Winograd kernels: [splits][pixels][cout] floats, a counter per (tile-block, 32 nb channels)
inline SplitKScratch wino_family_scratch(size_t tile_blocks, size_t pixels, int cout, int nb, int splits)
{
    return {splits > 1 ? (size_t)splits * pixels * cout * sizeof(float) : 0, tile_blocks * (cout / (32 * nb))};
}
inline SplitKScratch wino_scratch(int batch, int h, int w, int cout, int nb, int splits) { return wino_family_scratch(wino_tile_blocks(batch, h, w), (size_t)batch * h * w, cout, nb, splits); }
inline SplitKScratch wino4_scratch(int batch, int h, int w, int cout, int splits) { return wino_family_scratch(wino4_tile_blocks(batch, h, w), (size_t)batch * h * w, cout, 1, splits); }
inline SplitKScratch winoup_scratch(int batch, int hs, int ws, int cout, int nb, int splits) { return wino_family_scratch(winoup_tile_blocks(batch, hs, ws), (size_t)batch * 4 * hs * ws, cout, nb, splits); }
// K-split full-K kernel: [2][tiles][pb * 256] floats, a counter per tile of 16 pb pixels x 16 channels
inline SplitKScratch fullk_split_scratch(int batch, int ho, int cout, int pb)
{
    const size_t tiles = (size_t)batch * (ho * ho / (16 * pb)) * (cout / 16);
    return {2 * tiles * pb * 256 * sizeof(float), tiles};
}
// implicit GEMM: [splits][Mout][cout] floats; its in-launch combine (plans only) counts in the workspace's counters
inline SplitKScratch igemm_scratch(int mout, int cout, int splits) { return {splits > 1 ? (size_t)splits * mout * cout * sizeof(float) : 0, 0}; }

// Who gets a weight form at pack time: the batch-independent half of each kernel family's rule (the blob layout must not depend on the batch).
// Policy only -- which layers a family is FOR; extents, alignments and LDS bounds are the kernel's own *_supported() (kernels.h), asked here
// for one frame and by choose_route() for the batch.  Also used by lspf2f_conv3x3 on a LayerDesc filled from its arguments.
bool fullk_layer(const LayerDesc &l, int dtype);       // fp32 16x16 .. 2x2 stride-1 layers (incl. the nearest-upsampling up-convs below the sub-pixel extent)
bool fullk_s2_layer(const LayerDesc &l, int dtype);    // fp32 stride-2 convs writing 16x16 / 8x8 / 4x4 from one source of 256 | 512 channels (K-split form only)
bool fullk16_layer(const LayerDesc &l, int dtype);     // 16-bit 8x8 / 4x4 / 2x2 layers: stride 1, stride 2 (one source) or nearest x2 upsample in front
bool wino_layer(const LayerDesc &l, int dtype);        // fp32 stride-1 single-source convs at >= 16x16
bool wino4_layer(const LayerDesc &l, int dtype);       // ... of those the extents that are multiples of 32 (tile-blocks of 16 x 32 output pixels)
bool winoup_layer(const LayerDesc &l, int dtype);      // fp32 up-convs (either form) over one source or two equally wide ones
bool rowup_layer(const LayerDesc &l, int dtype);       // 16-bit sub-pixel up-conv over two 128-channel sources -> 64 channels (L1.up)
bool rowconv_layer(const LayerDesc &l, int dtype);     // 16-bit stride-1 single-source convs with as many channels out as in (64 | 128)
bool bandconv_layer(const LayerDesc &l, int dtype);    // 16-bit stride-1 512 -> Cout convs at 16x16 .. 2x2
// per batch: pixel blocks per tile of the fp32 full-K kernel for a fullk_layer (0 = another kernel keeps it); shared with lspf2f_conv3x3's tile 0x0
int fullk_choice(const LayerDesc &l, int batch, int dtype);
static const int kWinoMinExtent = 16;  // 16x16 only from 4 frames up (choose_route): below that the full-K kernel is as fast
static const int kUp4MinExtent = 32;   // up-convs writing >= 32x32 use the sub-pixel form

// THE kernel choice of a body layer at a batch: the route, its argument (LayerDesc::route_arg) and its tile
struct RouteChoice { ConvRoute route; int arg, bm, bn, splits, group; };
RouteChoice choose_route(const Plan &p, const LayerDesc &l, int batch);

}  // namespace lspf2f
