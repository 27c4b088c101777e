// C ABI of liblspf2f.so (include/lspf2f.h).  Host side: owns the plan, never owns device memory.
#include "../../include/lspf2f.h"

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "kernels.h"
#include "plan.h"

using namespace lspf2f;

struct GraphKey {
    const void *feat, *cand, *out, *out_u8, *ws, *blob;
    int cand_batch, batch;
    bool operator==(const GraphKey &o) const
    {
        return feat == o.feat && cand == o.cand && out == o.out && out_u8 == o.out_u8 && ws == o.ws && blob == o.blob &&
               cand_batch == o.cand_batch && batch == o.batch;
    }
};

struct CachedGraph {
    GraphKey key{};
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    void reset()
    {
        if (exec) (void)hipGraphExecDestroy(exec);
        if (graph) (void)hipGraphDestroy(graph);
        exec = nullptr; graph = nullptr;
    }
};
static const size_t kMaxCachedGraphs = 8;   // demo.py-style callers cycle through a few buffers

struct lspf2f_handle {
    Plan plan;
    lspf2f_config cfg{};
    const char *blob = nullptr;   // device, caller-owned
    size_t blob_size = 0;
    char *ws = nullptr;           // device, caller-owned
    size_t ws_size = 0;
    bool packed = false;
    bool use_graph = true;
    // (the next four: `tune` keys of lspf2f_create_tuned -- tools, tests, A-B runs)
    bool last_direct = false;     // lastconv_direct=1: 16-bit plans run the direct last-conv kernel instead of the GEMM form
    bool prefetch = true;         // prefetch=0: weight-streaming layers do not request the next launch's weights
    bool in_small_regs = true;    // in_small_regs=0: InstanceNorm plans run in_small in its three-pass form (re-reads the slab for the variance and the normalisation)
    bool smallm_dma = true;       // smallm_dma=0: conv3x3_smallm stages its input tensor through registers (the form of rounds 2-4) instead of LDS-DMA pieces
    bool smallm_static = true;    // smallm_static=0: conv3x3_smallm takes its geometry from its arguments at every shape (the only form until the static-geometry instances)
    bool fuse_splitk = true;      // fused_splitk=0: always combine split-K slabs with a separate launch
    bool counters_clean = false;  // the arrival counters at the head of the workspace were zeroed since it was bound
    int first_direct = 0;         // firstconv=1: vector-ALU first conv; 2: register-staged matrix-core kernel
    int timing_part = 3;          // lspf2f_subset_timed: 1 = main kernels only, 2 = split-K reduce only, 3 = everything (always 3 on the hot path)
    int last_route = 0;           // lastconv=<route>: forced direct last-conv kernel (LastConvParams::route; tests only)
    const void *cand_cached = nullptr;   // candidate stack whose first-conv contribution sits in the workspace cache
    hipStream_t cap_stream = nullptr;
    std::vector<CachedGraph> graphs;
    size_t next_victim = 0;
    void drop_graphs()
    {
        for (auto &g : graphs) g.reset();
        graphs.clear();
    }
    ~lspf2f_handle()
    {
        drop_graphs();
        if (cap_stream) (void)hipStreamDestroy(cap_stream);
    }
};

#ifdef LSPF2F_ABLATE
// tools/ablate.sh builds only: the ablation bits of the kernels (the shipped library never reads the process environment)
static int ablate_dbg() { const char *env = std::getenv("LSP_HIP_DBG"); return env ? std::atoi(env) : 0; }
#endif

static thread_local std::string g_err;
static int fail(int code, const std::string &msg) { g_err = msg; return code; }
static int hipfail(hipError_t e, const char *what)
{
    return fail(LSPF2F_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

extern "C" {

const char *lspf2f_last_error(void) { return g_err.c_str(); }
int lspf2f_abi_version(void) { return LSPF2F_ABI_VERSION; }

// "key=value,key=value" -> (key, integer value) pairs; "" / NULL = none.  Whitespace around tokens is ignored.
static bool parse_tune(const char *tune, std::vector<std::pair<std::string, int>> *out, std::string *bad)
{
    if (!tune) return true;
    std::string s(tune);
    size_t i = 0;
    while (i < s.size()) {
        size_t j = s.find(',', i);
        if (j == std::string::npos) j = s.size();
        std::string tok = s.substr(i, j - i);
        i = j + 1;
        const size_t a = tok.find_first_not_of(" \t"), b = tok.find_last_not_of(" \t");
        if (a == std::string::npos) continue;
        tok = tok.substr(a, b - a + 1);
        const size_t eq = tok.find('=');
        if (eq == std::string::npos || eq == 0 || eq + 1 >= tok.size()) { *bad = tok; return false; }
        char *endp = nullptr;
        const long v = std::strtol(tok.c_str() + eq + 1, &endp, 10);
        if (*endp) { *bad = tok; return false; }
        out->emplace_back(tok.substr(0, eq), (int)v);
    }
    return true;
}

int lspf2f_create(const lspf2f_config *cfg, lspf2f_handle **out) { return lspf2f_create_tuned(cfg, nullptr, out); }

int lspf2f_create_tuned(const lspf2f_config *cfg, const char *tune, lspf2f_handle **out)
{
    if (!cfg || !out) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "null argument");
    if (cfg->abi_version != LSPF2F_ABI_VERSION) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "ABI version mismatch");
    if (cfg->dtype != LSPF2F_DTYPE_F32 && cfg->dtype != LSPF2F_DTYPE_BF16 && cfg->dtype != LSPF2F_DTYPE_F16) return fail(LSPF2F_ERR_UNSUPPORTED, "unknown dtype");
    if (cfg->height != cfg->width) return fail(LSPF2F_ERR_UNSUPPORTED, "frames must be square (loadSize x loadSize)");
    if (cfg->max_batch < 1) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "max_batch must be >= 1");
    std::vector<std::pair<std::string, int>> kv;
    std::string bad;
    if (!parse_tune(tune, &kv, &bad)) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "tune: expected key=integer, got '" + bad + "'");
    lspf2f_handle *h = new (std::nothrow) lspf2f_handle();
    if (!h) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "out of host memory");
    h->cfg = *cfg;
    h->use_graph = (cfg->flags & LSPF2F_FLAG_NO_GRAPH) == 0;
    Plan &P = h->plan;
    P.use_wino4 = (cfg->flags & LSPF2F_FLAG_WINO4) != 0;
    // The switches of tools, tests and A-B runs: applied HERE, once per handle, before the plan is built (some decide what the packed blob
    // carries); nothing in this library reads the process environment.
    for (const auto &e : kv) {
        const std::string &k = e.first;
        const int v = e.second;
        if (k == "graph") h->use_graph = h->use_graph && v != 0;
        else if (k == "wino") P.use_wino = v != 0;
        else if (k == "wino4") P.use_wino4 = v != 0;
        else if (k == "wino_pre") P.wino_pre = v != 0;
        else if (k == "wino_xcd") P.wino_xcd = v;
        else if (k == "wino_il") P.wino_il = v != 0;
        else if (k == "wino_ureg") {
            if (v != 0 && v != 1) { delete h; return fail(LSPF2F_ERR_INVALID_ARGUMENT, "tune: wino_ureg takes 0 (U fragments through LDS) or 1 (in registers)"); }
            P.wino_ureg = v;
        }
        else if (k == "in_wino_stats") P.in_wino_stats = v != 0;
        else if (k == "wino_rot") P.wino_rot = v != 0;
        else if (k == "winoup") P.use_winoup = v != 0;
        else if (k == "winoup_nb") P.winoup_nb = v;
        else if (k == "winoup_target") P.winoup_target = v;
        else if (k == "igemm_xcd") P.igemm_xcd = v;
        else if (k == "bandconv") P.use_bandconv = v != 0;
        else if (k == "bandconv_min_blocks") P.bandconv_min_blocks = v;
        else if (k == "bandconv_min_frames") P.bandconv_min_frames_small = v;
        else if (k == "patch16") P.use_patch16 = v != 0;
        else if (k == "patchup16") P.use_patchup16 = v != 0;
        else if (k == "patch16_deep") P.patch16_deep = v != 0;
        else if (k == "patch16_min_blocks") P.patch16_min_blocks = v;
        else if (k == "rowup") P.use_rowup = v != 0;
        else if (k == "rowlast") P.use_rowlast = v != 0;
        else if (k == "rowlast_fused") P.rowlast_fused = v != 0;
        else if (k == "rowconv") P.use_rowconv = v != 0;
        else if (k == "fullk_split") P.use_fullk_split = v != 0;
        else if (k == "fullk_split_tiles") P.fullk_split_max_tiles = v;
        else if (k == "fullk_s2") P.use_fullk_s2 = v;
        else if (k == "all_forms") P.keep_all_forms = v != 0;
        else if (k == "blob_pad_kb") P.blob_pad_kb = v < 0 ? 0 : v;
        else if (k == "fused_splitk") h->fuse_splitk = v != 0;
        else if (k == "fused_splitk16") P.fused_splitk16 = v != 0;
        else if (k == "out_wt") P.out_wt = v;
        else if (k == "fullk16") P.fullk16_levels = v;
        else if (k == "fullk16_min_frames") P.fullk16_min_frames = v;
        else if (k == "wino_prio") P.wino_prio = v;
        else if (k == "prefetch") h->prefetch = v != 0;
        else if (k == "smallm_dma") h->smallm_dma = v != 0;
        else if (k == "smallm_kb") P.smallm_kb = v;
        else if (k == "smallm_static") {
            if (v != 0 && v != 1) { delete h; return fail(LSPF2F_ERR_INVALID_ARGUMENT, "tune: smallm_static takes 0 (run-time geometry) or 1 (static-geometry instances)"); }
            h->smallm_static = v != 0;
        }
        else if (k == "in_small_regs") h->in_small_regs = v != 0;
        else if (k == "in_smallm_fused") P.in_smallm_fused = v != 0;
        else if (k == "in_small_max_hw") P.in_small_max_hw = v;
        else if (k == "lastconv_direct") h->last_direct = v != 0;      // 16-bit plans: the direct last-conv kernel instead of the GEMM form
        else if (k == "lastconv") h->last_route = v;                   // LastConvParams::route (0 = by shape)
        else if (k == "firstconv") h->first_direct = v;                // FirstConvParams::force_direct (0 = by shape)
        else { delete h; return fail(LSPF2F_ERR_INVALID_ARGUMENT, "tune: unknown key '" + k + "'"); }
    }
    const std::string e = P.build(cfg->variant, cfg->input_nc, cfg->feat_nc, cfg->output_nc, cfg->ngf,
                                  cfg->num_downs, cfg->height,
                                  (cfg->flags & LSPF2F_FLAG_KEEP_INTERMEDIATES) != 0, cfg->dtype,
                                  (cfg->flags & LSPF2F_FLAG_INSTANCE_NORM) ? 1 : 0, cfg->max_batch);
    if (!e.empty()) { delete h; return fail(LSPF2F_ERR_UNSUPPORTED, e); }
    int largest = -1;
    const int frames = P.max_frames(&largest);
    if (cfg->max_batch > frames) {
        const TensorDesc &t = P.tensors[largest];
        const std::string msg = "max_batch " + std::to_string(cfg->max_batch) + " exceeds the limit of " + std::to_string(frames) + " frames: " + t.name + " (" +
                                std::to_string(t.h) + "x" + std::to_string(t.h) + "x" + std::to_string(t.c) + ", " + std::to_string((size_t)t.c * t.h * t.h * P.elt()) +
                                " bytes per frame) must stay within the kernels' 2 GiB tensor limit (32-bit buffer offsets)";
        delete h;
        return fail(LSPF2F_ERR_UNSUPPORTED, msg);
    }
    P.plan_batch(cfg->max_batch);
    *out = h;
    return LSPF2F_OK;
}

int lspf2f_destroy(lspf2f_handle *h)
{
    delete h;
    return LSPF2F_OK;
}

int lspf2f_num_tensors(const lspf2f_handle *h) { return h ? (int)h->plan.params.size() : fail(LSPF2F_ERR_INVALID_ARGUMENT, "null handle"); }

int lspf2f_tensor_info(const lspf2f_handle *h, int i, const char **name, int64_t dims[4], int *ndim)
{
    if (!h || i < 0 || i >= (int)h->plan.params.size()) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "bad tensor index");
    const ParamDesc &p = h->plan.params[i];
    if (name) *name = p.key.c_str();
    if (ndim) *ndim = (int)p.dims.size();
    if (dims) for (size_t d = 0; d < p.dims.size() && d < 4; ++d) dims[d] = p.dims[d];
    return LSPF2F_OK;
}

int lspf2f_set_tensor(lspf2f_handle *h, const char *key, const float *host, size_t numel)
{
    if (!h || !key || !host) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "null argument");
    auto it = h->plan.param_index.find(key);
    if (it == h->plan.param_index.end())
        return fail(LSPF2F_ERR_INVALID_ARGUMENT, std::string("unexpected state-dict key: ") + key);
    ParamDesc &p = h->plan.params[it->second];
    if (numel != p.numel())
        return fail(LSPF2F_ERR_SHAPE, std::string("size mismatch for ") + key + ": got " + std::to_string(numel) +
                                          ", expected " + std::to_string(p.numel()));
    p.data.assign(host, host + numel);
    p.set = true;
    h->packed = false;
    return LSPF2F_OK;
}

size_t lspf2f_packed_bytes(const lspf2f_handle *h) { return h ? h->plan.blob_bytes : 0; }

int lspf2f_pack_weights(lspf2f_handle *h, void *host_blob, size_t bytes)
{
    if (!h || !host_blob) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "null argument");
    const std::string e = h->plan.pack(host_blob, bytes);
    if (!e.empty())
        return fail(e.rfind("missing", 0) == 0 ? LSPF2F_ERR_MISSING_TENSOR : LSPF2F_ERR_INVALID_ARGUMENT, e);
    // the fp32 copies are no longer needed once packed; a second pack of the same handle needs the tensors set again (it answers MISSING_TENSOR, it used to crash)
    for (auto &p : h->plan.params) { std::vector<float>().swap(p.data); p.set = false; }
    h->packed = true;
    return LSPF2F_OK;
}

int lspf2f_bind_weights(lspf2f_handle *h, const void *dev_blob, size_t bytes)
{
    if (!h || !dev_blob) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "null argument");
    if (bytes < h->plan.blob_bytes) return fail(LSPF2F_ERR_SHAPE, "packed weight arena too small");
    if ((uintptr_t)dev_blob % 256) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "weight arena must be 256-byte aligned");
    h->drop_graphs();
    h->cand_cached = nullptr;
    h->blob = static_cast<const char *>(dev_blob);
    h->blob_size = bytes;
    return LSPF2F_OK;
}

size_t lspf2f_workspace_bytes(const lspf2f_handle *h, int batch)
{
    if (!h || batch < 1) return 0;
    // enough for EVERY batch of 1 .. batch frames: the plans of different batch sizes pick different kernels (split-K slabs come and go), so the need is
    // not monotonic in the batch -- a handle planned for 5 frames may need more for 3 of them than for 5
    size_t need = 0;
    for (int b = 1; b <= batch; ++b) need = std::max(need, h->plan.workspace_bytes(b));
    return need;
}

int lspf2f_bind_workspace(lspf2f_handle *h, void *dev_workspace, size_t bytes)
{
    if (!h || !dev_workspace) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "null argument");
    if ((uintptr_t)dev_workspace % 256) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "workspace must be 256-byte aligned");
    h->drop_graphs();
    h->cand_cached = nullptr;
    h->counters_clean = false;
    h->ws = static_cast<char *>(dev_workspace);
    h->ws_size = bytes;
    return LSPF2F_OK;
}

int lspf2f_num_layers(const lspf2f_handle *h) { return h ? (int)h->plan.layers.size() : fail(LSPF2F_ERR_INVALID_ARGUMENT, "null handle"); }

int lspf2f_plan_batch(lspf2f_handle *h, int batch)
{
    if (!h || batch < 1 || batch > h->cfg.max_batch) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "batch out of range");
    h->plan.plan_batch(batch);
    return LSPF2F_OK;
}

static const char *kernel_name(const LayerDesc &l, const Plan &P)
{
    if (l.kind == kFirstConv) return "first_conv";
    if (l.kind == kLastConv)
        return l.form_off[kFormGemmLast] < 0 ? "last_conv"
               : l.form_off[kFormRowLast] >= 0 && P.use_rowlast ? "last_conv (rowlast128 + pixel_shuffle_tanh)" : "last_conv (igemm3x3 + pixel_shuffle_tanh)";
    const bool two = l.route_arg == 2, split = l.splits > 1, small = l.in_route == kInSmall, stats = l.in_route == kInWino;
    switch (l.route) {
    case kRouteSmallM: return !l.inorm ? "conv3x3_smallm" : P.in_smallm_fused ? "conv3x3_smallm(in)" : "conv3x3_smallm+in_small";
    case kRouteWinoUp:
        if (!l.inorm) return two ? (split ? "winoup3x3<2> (split-K combined in the launch)" : "winoup3x3<2>") : (split ? "winoup3x3<1> (split-K combined in the launch)" : "winoup3x3<1>");
        if (stats) return two ? "winoup3x3<2>(stats)+in_finalize+in_apply" : "winoup3x3<1>(stats)+in_finalize+in_apply";
        return two ? (small ? "winoup3x3<2>+in_small" : "winoup3x3<2>+in_reduce_stats+in_finalize+in_apply")
                   : (small ? "winoup3x3<1>+in_small" : "winoup3x3<1>+in_reduce_stats+in_finalize+in_apply");
    case kRouteWino4:
        if (!l.inorm) return split ? "wino4_3x3 (split-K combined in the launch)" : "wino4_3x3";
        return small ? "wino4_3x3+in_small" : "wino4_3x3+in_reduce_stats+in_finalize+in_apply";
    case kRouteWino:
        if (!l.inorm) return two ? (split ? "wino3x3<2> (split-K combined in the launch)" : "wino3x3<2>") : (split ? "wino3x3<1> (split-K combined in the launch)" : "wino3x3<1>");
        if (stats) return two ? "wino3x3<2>(stats)+in_finalize+in_apply" : "wino3x3<1>(stats)+in_finalize+in_apply";
        return two ? (small ? "wino3x3<2>+in_small" : "wino3x3<2>+in_reduce_stats+in_finalize+in_apply")
                   : (small ? "wino3x3<1>+in_small" : "wino3x3<1>+in_reduce_stats+in_finalize+in_apply");
    case kRouteRowUp: return "rowup256";
    case kRoutePatchUp16: return "conv3x3_patchup16";
    case kRoutePatch16: return "conv3x3_patch16";
    case kRouteBand: return "bandconv512";
    case kRouteRowConv: return l.c0 == 64 ? "rowconv64" : "rowconv128";
    case kRouteFullK16: return "conv3x3_fullk16";
    case kRouteFullK: return l.inorm ? "conv3x3_fullk+in_small" : "conv3x3_fullk";
    case kRouteIgemm:
        if (l.inorm) return l.in_route == kInFused ? "igemm3x3(stats)+in_finalize+in_apply" : small ? "igemm3x3+in_small" : "igemm3x3+in_reduce_stats+in_finalize+in_apply";
        return !split ? "igemm3x3" : l.fused_splitk ? "igemm3x3 (split-K combined in the launch)" : "igemm3x3+splitk_reduce";
    }
    return "";
}

int lspf2f_layer_info_get(const lspf2f_handle *h, int i, lspf2f_layer_info *o)
{
    if (!h || !o || i < 0 || i >= (int)h->plan.layers.size()) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "bad layer index");
    const LayerDesc &l = h->plan.layers[i];
    o->name = l.name.c_str();
    o->kernel = kernel_name(l, h->plan);
    o->cin = l.cin; o->cout = l.cout; o->h_in = l.hs; o->h_out = l.ho; o->stride = l.stride;
    o->upsample = l.up || l.up4; o->concat = l.concat; o->residual = l.residual; o->relu = l.relu; o->tanh_out = l.tanh_out;
    o->tile_m = l.bm; o->tile_n = l.bn; o->split_k = l.splits; o->k_group = l.group;
    o->flops_per_frame = h->plan.layer_flops(l);
    o->act_bytes_per_frame = h->plan.layer_act_bytes(l);
    // what the layer's kernel reads and multiplies: the sub-pixel form does 16 multiplies per 2x2 outputs instead of 36, the up-conv Winograd form 9,
    // Winograd F(2x2, 3x3) 16, F(4x4, 3x3) 36 per 4x4 outputs instead of 144 (first / last conv: their rows, whatever the last conv's route)
    const bool body = l.kind == kIgemm;
    o->weight_bytes = (int64_t)h->plan.form_bytes(l, body ? route_form(l) : kFormRows);
    const bool quarter = body && (l.route == kRouteWinoUp || l.route == kRouteWino4);
    const bool four_ninths = l.up4 || l.kind == kLastConv || (body && l.route == kRouteWino);
    o->exec_flops_per_frame = quarter ? o->flops_per_frame / 4 : four_ninths ? o->flops_per_frame * 4 / 9 : o->flops_per_frame;
    o->w_offset = l.form_off[kFormRows]; o->scale_offset = l.scale_off; o->shift_offset = l.shift_off;
    o->out_offset = l.out >= 0 ? (int64_t)h->plan.tensors[l.out].offset : -1;
    return LSPF2F_OK;
}

int lspf2f_unet_prepare(const float *src_dev, int src_nchw, int batch, int h, int w, int c, float slope,
                        float *s2d_out_dev, int s2d_channels, float *relu_out_dev, void *hip_stream)
{
    if (!src_dev || (!s2d_out_dev && !relu_out_dev)) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "null argument");
    PrepareParams p{src_dev, src_nchw ? 1 : 0, batch, h, w, c, slope, s2d_out_dev, s2d_channels, relu_out_dev};
    const hipError_t e = launch_unet_prepare(p, static_cast<hipStream_t>(hip_stream));
    if (e == hipErrorInvalidValue) return fail(LSPF2F_ERR_SHAPE, "unet_prepare: h, w must be even and s2d_channels >= 4c, a multiple of 4");
    return e == hipSuccess ? LSPF2F_OK : hipfail(e, "unet_prepare launch");
}

int lspf2f_pixel_shuffle(const float *g_dev, int batch, int hs, int ws, int cout, int apply_tanh,
                         float *out_f32_dev, unsigned char *out_u8_dev, void *hip_stream)
{
    if (!g_dev || (!out_f32_dev && !out_u8_dev)) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "null argument");
    if (batch < 1 || hs < 1 || ws < 1 || cout < 1 || cout > 4) return fail(LSPF2F_ERR_SHAPE, "pixel_shuffle: cout must be in 1..4");
    ShuffleParams sp{g_dev, out_f32_dev, out_u8_dev, batch, hs, ws, cout, apply_tanh ? 1 : 0, 0, nullptr};
    const hipError_t e = launch_pixel_shuffle(sp, static_cast<hipStream_t>(hip_stream));
    return e == hipSuccess ? LSPF2F_OK : hipfail(e, "pixel_shuffle launch");
}

int64_t lspf2f_layer_form_offset(const lspf2f_handle *h, int layer, int form)
{
    if (!h || layer < 0 || layer >= (int)h->plan.layers.size() || form < 0 || form >= kNumForms) return -1;
    return h->plan.layers[layer].form_off[form];
}

int lspf2f_memcpy(void *dst, const void *src, size_t bytes, void *hip_stream)
{
    if (!dst || !src) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "null argument");
    const hipError_t e = launch_copy16(dst, src, bytes, static_cast<hipStream_t>(hip_stream));
    if (e == hipErrorInvalidValue) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "lspf2f_memcpy: pointers and size must be multiples of 16 bytes");
    return e == hipSuccess ? LSPF2F_OK : hipfail(e, "lspf2f_memcpy launch");
}

int lspf2f_clock_probe(unsigned long long *out_dev, unsigned duration_us, void *hip_stream)
{
    if (!out_dev || duration_us == 0 || duration_us > 2000000u) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "clock_probe: null output or duration outside 1..2 000 000 us");
    const hipError_t e = launch_clock_probe(out_dev, duration_us, static_cast<hipStream_t>(hip_stream));
    return e == hipSuccess ? LSPF2F_OK : hipfail(e, "clock_probe launch");
}

}  // extern "C"

// ---- InstanceNorm behind a conv: what run_layer and the per-layer entry points (lspf2f_instance_norm, lspf2f_conv3x3_instnorm) share ----
// statistics scratch of one layer: per-group (sum d, sum d^2, shift) [3][slab][C], then the finalised (mean, rstd) [2][B][C]; slab = B x the groups the scratch holds
static void in_bind_stats(InstNormParams &q, float *st, size_t slab)
{
    q.psum = st; q.psq = st + slab * q.C; q.pshift = st + 2 * slab * q.C;
    q.mean = st + 3 * slab * q.C; q.rstd = q.mean + (size_t)q.B * q.C;
}
// groups a statistics producer leaves per frame: the implicit GEMM's epilogue one per wave (x4 for the sub-pixel up-convs, per parity), the Winograd kernels one per
// tile-block of 128 output pixels
static void in_groups_igemm(InstNormParams &q, int bm, bool up4, int rhw)
{
    q.rows_per_group = in_fused_wave_rows(bm);
    q.groups = (up4 ? 4 : 1) * rhw / q.rows_per_group;
}
static void in_groups_wino(InstNormParams &q) { q.groups = q.hw / 128; q.rows_per_group = 128; }
static hipError_t in_finalize_apply(const InstNormParams &q, hipStream_t s)
{
    hipError_t r = launch_in_finalize(q, s);
    if (r == hipSuccess) r = launch_in_apply(q, s);
    return r;
}
// the standalone passes over a complete raw tensor (or over split-K partials + bias): one launch (`small`), or 64-row partial sums -> finalize -> apply
static hipError_t in_standalone(InstNormParams &q, bool small, float *st, size_t slab, hipStream_t s)
{
    if (small) return launch_in_small(q, s);
    in_bind_stats(q, st, slab);
    q.groups = (q.hw + 63) / 64; q.rows_per_group = 64;
    const hipError_t r = launch_in_reduce_stats(q, s);
    return r == hipSuccess ? in_finalize_apply(q, s) : r;
}

// ---- a body layer's kernel arguments, stated once per kernel family.  Both callers know a ConvIO and a LayerDesc: run_layer (a plan's layer: workspace tensors,
// blob offsets) and conv3x3_run (lspf2f_conv3x3's arguments; conv3x3_layer() + the decoded tile code).  The builders fill the pointers and the shape; what only one
// caller knows -- the plan's tune knobs, the tool builds' stamps, the statistics pointers of an InstanceNorm behind the conv -- that caller sets on the result ----
struct ConvIO {
    const void *src0, *src1, *w;          // src1 == nullptr when the layer has one source
    const float *scale, *shift;
    const void *residual;
    void *out;
    float *partial;                       // split-K slabs and, behind them, the arrival counters of an in-launch combine (bound when the layer's splits > 1;
    unsigned *tile_cnt;                   //   the implicit GEMM binds its own counters: plans only)
    int batch, dtype, relu;
    int kernel_order;                     // w is in the kernel's own (fragment / tile-blocked) order -- the plans' blob always -- not rows [cout][9][cin]
};
static const float *f32(const void *p) { return static_cast<const float *>(p); }

static SmallMParams smallm_params(const ConvIO &io, const LayerDesc &l)
{
    SmallMParams p{};
    p.src = io.src0; p.w = io.w; p.scale = io.scale; p.shift = io.shift; p.residual = io.residual; p.out = io.out;
    p.B = io.batch; p.Hs = p.Ws = l.hs; p.Ho = p.Wo = l.ho; p.Cin = l.cin; p.Cout = l.cout;
    p.stride = l.stride; p.up = l.up; p.relu = io.relu; p.M = io.batch * l.ho * l.ho; p.dtype = io.dtype;
    return p;
}
static WinoUpParams winoup_params(const ConvIO &io, const LayerDesc &l)
{
    WinoUpParams p{};
    p.src0 = f32(io.src0); p.src1 = f32(io.src1); p.u = f32(io.w); p.scale = io.scale; p.shift = io.shift; p.out = static_cast<float *>(io.out);
    p.B = io.batch; p.Hs = p.Ws = l.hs; p.C0 = l.c0; p.C1 = l.c1; p.N = l.cout; p.relu = io.relu; p.splits = l.splits;
    if (l.splits > 1) { p.partial = io.partial; p.tile_cnt = io.tile_cnt; }      // the counters must be zero on entry; every launch leaves them zero
    return p;
}
static WinoParams wino_params(const ConvIO &io, const LayerDesc &l)          // wino3x3 and wino4_3x3
{
    WinoParams p{};
    p.src = f32(io.src0); p.u = f32(io.w); p.scale = io.scale; p.shift = io.shift; p.residual = f32(io.residual); p.out = static_cast<float *>(io.out);
    p.B = io.batch; p.H = p.W = l.ho; p.C = l.cin; p.N = l.cout; p.relu = io.relu; p.splits = l.splits;
    if (l.splits > 1) { p.partial = io.partial; p.tile_cnt = io.tile_cnt; }
    return p;
}
static RowUpParams rowup_params(const ConvIO &io, const LayerDesc &l)
{
    RowUpParams p{};
    p.src0 = io.src0; p.src1 = io.src1; p.w = io.w; p.scale = io.scale; p.shift = io.shift; p.out = io.out;
    p.B = io.batch; p.H = p.W = l.hs; p.R = l.route_arg; p.relu = io.relu; p.dtype = io.dtype;
    return p;
}
static PatchConvParams patch_params(const ConvIO &io, const LayerDesc &l)    // conv3x3_patch16 (one source) and conv3x3_patchup16 (H x W = the LOW-res extent)
{
    PatchConvParams p{};
    p.src = io.src0; p.src1 = io.src1; p.w = io.w; p.scale = io.scale; p.shift = io.shift; p.residual = io.residual; p.out = io.out;
    p.B = io.batch; p.H = p.W = l.up4 ? l.hs : l.ho; p.C = l.c0; p.C1 = l.c1; p.Cout = l.cout; p.relu = io.relu; p.dtype = io.dtype;
    return p;
}
static BandConvParams band_params(const ConvIO &io, const LayerDesc &l)
{
    BandConvParams p{};
    p.src = io.src0; p.w = io.w; p.scale = io.scale; p.shift = io.shift; p.residual = io.residual; p.out = io.out;
    p.B = io.batch; p.W = l.ho; p.Cout = l.cout; p.relu = io.relu; p.dtype = io.dtype;
    return p;
}
static RowConvParams rowconv_params(const ConvIO &io, const LayerDesc &l)
{
    RowConvParams p{};
    p.src = io.src0; p.w = io.w; p.scale = io.scale; p.shift = io.shift; p.residual = io.residual; p.out = io.out;
    p.B = io.batch; p.H = p.W = l.ho; p.C = l.c0; p.R = l.route_arg; p.relu = io.relu; p.dtype = io.dtype; p.wfrag = io.kernel_order;
    return p;
}
static FullK16Params fullk16_params(const ConvIO &io, const LayerDesc &l)
{
    FullK16Params p{};
    p.src0 = io.src0; p.src1 = io.src1; p.w = io.w; p.scale = io.scale; p.shift = io.shift; p.residual = io.residual; p.out = io.out;
    p.B = io.batch; p.Hs = p.Ws = l.hs; p.Ho = p.Wo = l.ho; p.C0 = l.c0; p.C1 = l.c1; p.Cout = l.cout;
    p.up = l.up; p.relu = io.relu; p.stride = l.stride; p.dtype = io.dtype; p.wtile = io.kernel_order;
    return p;
}
static FullKParams fullk_params(const ConvIO &io, const LayerDesc &l)
{
    FullKParams p{};
    p.src0 = f32(io.src0); p.src1 = f32(io.src1); p.w = f32(io.w); p.scale = io.scale; p.shift = io.shift; p.residual = f32(io.residual); p.out = static_cast<float *>(io.out);
    p.B = io.batch; p.Hs = p.Ws = l.hs; p.Ho = p.Wo = l.ho; p.C0 = l.c0; p.C1 = l.c1; p.Cout = l.cout;
    p.up = l.up; p.relu = io.relu; p.stride = l.stride; p.wtile = io.kernel_order;
    if (l.splits == 2) {          // K in two halves, combined in the launch; a single source is then read (and its weights packed) as two half-sources: route_form
        p.split = 2; p.partial = io.partial; p.tile_cnt = io.tile_cnt;
    }
    return p;
}
static IgemmParams igemm_params(const ConvIO &io, const LayerDesc &l)
{
    IgemmParams p{};
    p.src0 = io.src0; p.src1 = io.src1; p.w = io.w; p.scale = io.scale; p.shift = io.shift; p.residual = io.residual; p.out = io.out;
    p.partial = io.partial;
    p.B = io.batch; p.Hs = p.Ws = l.hs; p.Ho = p.Wo = l.ho; p.C0 = l.c0; p.C1 = l.c1; p.Cin = l.cin; p.Cout = l.cout;
    p.stride = l.stride; p.up = l.up; p.up4 = l.up4; p.relu = io.relu; p.dtype = io.dtype;
    p.Mout = io.batch * l.ho * l.ho;
    p.M = l.up4 ? io.batch * l.hs * l.hs : p.Mout;
    p.ktiles_total = (l.up4 ? 4 : 9) * l.cin / (io.dtype ? 64 : 32);
    p.splits = l.splits;
    p.ktiles_per_split = (p.ktiles_total + l.splits - 1) / l.splits;
    return p;
}

static int run_layer(lspf2f_handle *h, const LayerDesc &l, const float *feat, const float *cand, int cand_batch,
                     float *out, unsigned char *out_u8, int batch, hipStream_t s)
{
    const Plan &P = h->plan;
    auto tptr = [&](int t) -> float * { return t < 0 ? nullptr : reinterpret_cast<float *>(h->ws + P.tensors[t].offset); };
    auto bptr = [&](int64_t off) -> const float * { return off < 0 ? nullptr : reinterpret_cast<const float *>(h->blob + off); };
    hipError_t e = hipSuccess;
    // InstanceNorm plans: the normalisation of this layer's output (+ residual, ReLU), and the statistics scratch
    float *const st = reinterpret_cast<float *>(h->ws + P.stats_offset);
    const size_t slab = (size_t)batch * P.stats_groups_max;            // [B][groups][C] with C <= the plan's widest layer
    auto in_of_output = [&]() {
        InstNormParams q{};
        q.three_pass = h->in_small_regs ? 0 : 1;
        q.x = tptr(l.out); q.residual = tptr(l.res); q.relu = l.relu; q.partial = nullptr; q.splits = 1; q.bias = nullptr;
        q.B = batch; q.hw = l.ho * l.ho; q.C = l.cout;
        return q;
    };
    // ... behind a kernel that has written the complete raw conv output (+ bias) itself (the Winograd kernels combine their split-K slabs in the launch; the
    // tiny-M and full-K kernels have none): statistics + normalisation as separate passes over that tensor -- one launch (`small`), or reduce, finalize, apply
    auto in_after_complete_output = [&](hipError_t prev, bool small) -> hipError_t {
        if (prev != hipSuccess) return prev;
        InstNormParams q = in_of_output();
        return in_standalone(q, small, st, slab, s);
    };
    // ... around a Winograd kernel (`launch` runs it on `p`).  kInWino: its epilogue (or its split-K combine) leaves the sums of every tile-block of 128 output
    // pixels at the pointers bound here, so only finalize + normalise follow; otherwise the passes above
    auto wino_with_in = [&](auto &p, auto &&launch) -> hipError_t {
        if (!l.inorm) return launch();
        if (l.in_route != kInWino) return in_after_complete_output(launch(), l.in_route == kInSmall);
        InstNormParams q = in_of_output();
        in_bind_stats(q, st, slab);
        in_groups_wino(q);
        p.psum = q.psum; p.psq = q.psq; p.pshift = q.pshift;
        const hipError_t r = launch();
        return r == hipSuccess ? in_finalize_apply(q, s) : r;
    };
    // A body layer's tensors, the blob address of the form its route reads, and the plan's split-K scratch.  InstanceNorm plans: the conv writes its raw output (+ bias);
    // the residual add and the ReLU move behind the normalisation -- except in the tiny-M kernel, whose workgroup holds every pixel of its channels and normalises in its
    // own epilogue (`in_smallm_fused`)
    const bool in_fused = l.inorm && l.route == kRouteSmallM && P.in_smallm_fused;
    const bool raw = l.inorm && !in_fused;
    const ConvIO io{tptr(l.src0), tptr(l.src1), l.kind == kIgemm ? bptr(l.form_off[route_form(l)]) : nullptr, bptr(l.scale_off), bptr(l.shift_off),
                    raw ? nullptr : tptr(l.res), tptr(l.out), reinterpret_cast<float *>(h->ws + P.partial_offset),
                    reinterpret_cast<unsigned *>(h->ws + P.counters_offset()), batch, P.dtype, raw ? 0 : (int)l.relu, 1};
    const bool main_part = (h->timing_part & 1) != 0;      // lspf2f_subset_timed may leave the main kernel out
    if (l.kind == kFirstConv) {
        FirstConvParams p{};
        p.feat = feat; p.cand = cand; p.w = bptr(l.form_off[kFormRows]); p.out = tptr(l.out);
        p.B = batch; p.H = l.hs; p.W = l.hs; p.feat_nc = P.feat_nc; p.cand_nc = P.input_nc - P.feat_nc;
        p.cand_batch = cand_batch; p.Cout = l.cout; p.dtype = P.dtype;
        p.ci_begin = 0; p.ci_end = P.input_nc; p.base = nullptr; p.relu = 1;
        p.bias = bptr(l.shift_off);          // InstanceNorm plans: the conv bias (scale is 1); nullptr otherwise
        // two slots at the head of the workspace: [0] lspf2f_set_candidates' per-person cache, [1] the per-forward share of a
        // broadcast stack -- separate, so a broadcast forward never overwrites what the cache holds
        float *cache = reinterpret_cast<float *>(cand != nullptr ? h->ws + P.cand_cache_bytes() : h->ws);
        p.force_direct = h->first_direct;
#ifdef LSPF2F_ABLATE
        p.dbg = ablate_dbg();
#endif
        // a candidate stack shared by a batch (cand_batch == 1, batch > 1): its 12-channel share is computed once (matrix-core kernel,
        // channel range) and every frame adds its feature-map channel in a streaming pass -- measured 77 us vs 150 us at batch 8 for
        // running the full 13-channel layer per frame
        const bool shared = p.cand_nc > 0 && P.feat_nc > 0 && (cand == nullptr || (cand_batch == 1 && batch > 1));
        if (shared) {
            // candidate stack shared by the whole batch: its contribution is computed once (or taken
            // from lspf2f_set_candidates' cache when cand == NULL), each frame then adds its own
            // feature-map channels
            if (cand != nullptr) {
                FirstConvParams c = p;
                c.B = 1; c.cand_batch = 1; c.ci_begin = P.feat_nc; c.out = cache; c.relu = 0; c.bias = nullptr;
                e = launch_first_conv(c, s);
            }
            p.ci_end = P.feat_nc; p.base = cache;
            if (e == hipSuccess) e = launch_first_conv(p, s);
        } else {
            e = launch_first_conv(p, s);
        }
    } else if (l.kind == kLastConv && P.last_as_gemm(l) && !h->last_direct) {
        // bf16: 3x3 conv on the low-res source with N = 4 parities x cout through the MFMA kernel, then shuffle + tanh
        if (l.form_off[kFormRowLast] >= 0 && P.use_rowlast) {
            RowLastParams q{};
            q.src0 = tptr(l.src0); q.src1 = tptr(l.src1); q.w = h->blob + l.form_off[kFormRowLast];
            q.out = reinterpret_cast<float *>(h->ws + P.partial_offset);
            q.B = batch; q.H = l.hs; q.W = l.hs; q.R = rowlast_rows(batch, l.hs, l.hs); q.dtype = P.dtype;
            // fp32 frames only: shuffle + tanh in the kernel's epilogue (no intermediate, no second launch); uint8 rows (tensor2im) keep the two-launch form
            const bool fused = P.rowlast_fused && out && !out_u8;
            if (fused) { q.out_nchw = out; q.cout = l.cout; q.apply_tanh = l.tanh_out ? 1 : 0; }
            e = launch_rowlast(q, s);
            if (e == hipSuccess && !fused) {
                ShuffleParams sp{reinterpret_cast<const float *>(h->ws + P.partial_offset), out, out_u8, batch, l.hs, l.hs, l.cout, l.tanh_out ? 1 : 0, 1, nullptr};
                e = launch_pixel_shuffle(sp, s);
            }
            if (e != hipSuccess) return hipfail(e, ("launch " + l.name).c_str());
            return LSPF2F_OK;
        }
        IgemmParams g{};
        g.src0 = tptr(l.src0); g.src1 = tptr(l.src1); g.w = h->blob + l.form_off[kFormGemmLast];
        g.out = h->ws + P.partial_offset; g.out_f32 = 1;
        g.B = batch; g.Hs = l.hs; g.Ws = l.hs; g.Ho = l.hs; g.Wo = l.hs;
        g.C0 = l.c0; g.C1 = l.c1; g.Cin = l.cin; g.Cout = 4 * l.cout;
        g.stride = 1; g.Mout = batch * l.hs * l.hs; g.M = g.Mout; g.dtype = P.dtype;
        g.ktiles_total = 9 * l.cin / P.ktile_channels(); g.splits = 1; g.ktiles_per_split = g.ktiles_total;
        e = launch_igemm(g, 128, 32, 1, s);
        if (e == hipSuccess) {
            ShuffleParams sp{reinterpret_cast<const float *>(h->ws + P.partial_offset), out, out_u8, batch, l.hs, l.hs, l.cout, l.tanh_out ? 1 : 0, 0, nullptr};
            e = launch_pixel_shuffle(sp, s);
        }
    } else if (l.kind == kLastConv) {
        LastConvParams p{};
        p.src0 = tptr(l.src0); p.src1 = tptr(l.src1); p.w = bptr(l.form_off[kFormRows]); p.out = out;
        p.B = batch; p.Hs = l.hs; p.Ws = l.hs; p.C0 = l.c0; p.C1 = l.c1; p.Cout = l.cout; p.apply_tanh = l.tanh_out; p.out_u8 = out_u8; p.dtype = P.dtype;
        p.route = h->last_route;
        p.bias = bptr(l.shift_off);
        e = launch_last_conv(p, s);
    } else switch (l.route) {
    case kRouteSmallM: {
        SmallMParams p = smallm_params(io, l);
        p.in_fused = in_fused ? 1 : 0;
        p.stage_regs = h->smallm_dma ? 0 : 1;
        p.runtime_geo = h->smallm_static ? 0 : 1;
        if (h->prefetch && P.dtype == 0 && !l.inorm) {
            // the next launch, if it is another weight-streaming layer: its weights (in the form its route reads) are requested from inside this one
            const size_t li = (size_t)(&l - P.layers.data());
            if (li + 1 < P.layers.size()) {
                const LayerDesc &n = P.layers[li + 1];
                const int64_t off = n.kind == kIgemm && (n.route == kRouteSmallM || n.route == kRouteFullK) ? n.form_off[route_form(n)] : -1;
                if (off >= 0) { p.pf = h->blob + off; p.pf_bytes = (unsigned)((size_t)n.cout * 9 * n.cin * sizeof(float)); }
            }
        }
        e = launch_smallm(p, s);
        if (l.inorm && !in_fused) e = in_after_complete_output(e, true);          // raw conv output (+ bias) -> statistics + normalisation (+ residual, ReLU) in one launch
        break;
    }
    case kRouteWinoUp: {
        WinoUpParams p = winoup_params(io, l);
        p.out_wt = P.out_wt; p.prio = P.wino_prio;
        e = wino_with_in(p, [&] { return main_part ? launch_winoup(p, l.route_arg, s) : hipSuccess; });
        break;
    }
    case kRouteWino4:
    case kRouteWino: {
        WinoParams p = wino_params(io, l);
        if (l.route == kRouteWino4) {          // (never kInWino: F(4x4,3x3) leaves no epilogue sums)
            e = wino_with_in(p, [&] { return main_part ? launch_wino4(p, s) : hipSuccess; });
            break;
        }
        p.nopre = P.wino_pre ? 0 : 1; p.xcd_force = P.wino_xcd + 1; p.no_il = P.wino_il ? 0 : 1; p.no_rot = P.wino_rot ? 0 : 1; p.ureg = P.wino_ureg; p.out_wt = P.out_wt; p.prio = P.wino_prio;
        e = wino_with_in(p, [&] { return main_part ? launch_wino(p, l.route_arg, s) : hipSuccess; });
        break;
    }
    case kRouteRowUp: e = launch_rowup(rowup_params(io, l), s); break;
    case kRoutePatchUp16: e = launch_patchup16(patch_params(io, l), l.route_arg, l.bn, s); break;
    case kRoutePatch16: {
        PatchConvParams p = patch_params(io, l);
        p.deep = P.patch16_deep;
        e = launch_patch16(p, l.route_arg, l.bn, s);
        break;
    }
    case kRouteBand: e = launch_bandconv(band_params(io, l), s); break;
    case kRouteRowConv: e = launch_rowconv(rowconv_params(io, l), s); break;
    case kRouteFullK16: e = launch_fullk16(fullk16_params(io, l), l.route_arg, s); break;
    case kRouteFullK:
        e = launch_fullk(fullk_params(io, l), l.route_arg, s);
        if (l.inorm) e = in_after_complete_output(e, true);          // InstanceNorm plans: H*W <= 256 here, the one-launch statistics route
        break;
    case kRouteIgemm: {
        IgemmParams p = igemm_params(io, l);
        if (l.inorm) {
            InstNormParams q = in_of_output();
            if (l.in_route == kInFused) {
                in_bind_stats(q, st, slab);
                in_groups_igemm(q, l.bm, l.up4, l.up4 ? l.hs * l.hs : l.ho * l.ho);      // one group per wave
                p.psum = q.psum; p.psq = q.psq; p.pshift = q.pshift; p.in_groups = q.groups;
                e = launch_igemm(p, l.bm, l.bn, l.group, s);
                if (e == hipSuccess) e = in_finalize_apply(q, s);
            } else {
                e = launch_igemm(p, l.bm, l.bn, l.group, s);
                q.splits = l.splits;
                q.partial = l.splits > 1 ? p.partial : nullptr;
                q.bias = bptr(l.shift_off);
                if (e == hipSuccess) e = in_standalone(q, l.in_route == kInSmall, st, slab, s);
            }
        } else {
            const bool fused = l.fused_splitk && h->fuse_splitk;
            if (fused) {
                p.tile_cnt = io.tile_cnt;
                p.slab_bytes = igemm_scratch(p.Mout, l.cout, l.splits).slab_bytes;
            }
            p.xcd_force = P.igemm_xcd + 1;
            if (main_part) e = launch_igemm(p, l.bm, l.bn, l.group, s);
            if (e == hipSuccess && l.splits > 1 && !fused && (h->timing_part & 2)) e = launch_splitk_reduce(p, s);
        }
        break;
    }
    }
    if (e != hipSuccess) return hipfail(e, ("launch " + l.name).c_str());
    return LSPF2F_OK;
}

// the arrival counters of the in-launch split-K combine must be zero before the first launch that uses them; every last arriver
// resets its own, so once per workspace binding is enough
static int clean_counters(lspf2f_handle *h, hipStream_t s)
{
    if (h->counters_clean) return LSPF2F_OK;
    const hipError_t e = hipMemsetAsync(h->ws + h->plan.counters_offset(), 0, Plan::kTileCounters * sizeof(unsigned), s);
    if (e != hipSuccess) return hipfail(e, "hipMemsetAsync (split-K arrival counters)");
    h->counters_clean = true;
    return LSPF2F_OK;
}

static int check_forward_args(lspf2f_handle *h, const float *feat, const float *cand, int cand_batch, float *out,
                              int batch)
{
    if (!h || !feat || !out) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "null argument");
    if (batch < 1 || batch > h->cfg.max_batch) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "batch out of range (max_batch)");
    const int cand_nc = h->plan.input_nc - h->plan.feat_nc;
    if (cand_nc > 0 && !cand && !h->cand_cached)
        return fail(LSPF2F_ERR_INVALID_ARGUMENT, "cand_image is required (input_nc > feat_nc) unless lspf2f_set_candidates() was called");
    if (cand_nc > 0 && cand && cand_batch != 1 && cand_batch != batch)
        return fail(LSPF2F_ERR_SHAPE, "cand_batch must be 1 (broadcast) or equal to batch");
    if (!h->blob) return fail(LSPF2F_ERR_STATE, "weights not bound (lspf2f_bind_weights)");
    if (!h->ws) return fail(LSPF2F_ERR_STATE, "workspace not bound (lspf2f_bind_workspace)");
    h->plan.plan_batch(batch);
    if (h->ws_size < h->plan.act_bytes + h->plan.partial_bytes + h->plan.stats_bytes)
        return fail(LSPF2F_ERR_STATE, "workspace too small for this batch (lspf2f_workspace_bytes)");
    return LSPF2F_OK;
}

extern "C" {

int lspf2f_forward(lspf2f_handle *h, const float *feat_dev, const float *cand_dev, int cand_batch, float *out_dev,
                   int batch, void *hip_stream)
{
    return lspf2f_forward_ex(h, feat_dev, cand_dev, cand_batch, out_dev, nullptr, batch, hip_stream);
}

int lspf2f_forward_ex(lspf2f_handle *h, const float *feat_dev, const float *cand_dev, int cand_batch, float *out_dev,
                      unsigned char *out_u8_dev, int batch, void *hip_stream)
{
    if (!out_dev && !out_u8_dev) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "at least one of out_dev / out_u8_dev is required");
    int rc = check_forward_args(h, feat_dev, cand_dev, cand_batch, out_dev ? out_dev : reinterpret_cast<float *>(out_u8_dev), batch);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    rc = clean_counters(h, s);
    if (rc) return rc;

    // The ~80-150 launches of one forward are replayed from a hipGraph (captured once per
    // distinct set of pointers on a private stream), which removes the per-launch host cost that
    // dominates the <= 16x16 levels at batch 1.  If the caller is itself capturing `s`, or graphs
    // are disabled, launch eagerly into `s` instead.
    bool eager = !h->use_graph;
    if (!eager) {
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        if (s != nullptr && hipStreamIsCapturing(s, &st) == hipSuccess && st != hipStreamCaptureStatusNone) eager = true;
    }
    if (eager) {
        for (const auto &l : h->plan.layers) {
            rc = run_layer(h, l, feat_dev, cand_dev, cand_batch, out_dev, out_u8_dev, batch, s);
            if (rc) return rc;
        }
        return LSPF2F_OK;
    }

    GraphKey key{feat_dev, cand_dev, out_dev, out_u8_dev, h->ws, h->blob, cand_batch, batch};
    CachedGraph *g = nullptr;
    for (auto &c : h->graphs)
        if (c.exec && c.key == key) { g = &c; break; }
    if (!g) {
        if (!h->cap_stream) {
            const hipError_t e = hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking);
            if (e != hipSuccess) return hipfail(e, "hipStreamCreateWithFlags");
        }
        if (h->graphs.size() < kMaxCachedGraphs) h->graphs.emplace_back();
        g = &h->graphs[h->next_victim++ % h->graphs.size()];
        g->reset();
        hipError_t e = hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeThreadLocal);
        if (e != hipSuccess) return hipfail(e, "hipStreamBeginCapture");
        for (const auto &l : h->plan.layers) {
            rc = run_layer(h, l, feat_dev, cand_dev, cand_batch, out_dev, out_u8_dev, batch, h->cap_stream);
            if (rc) break;
        }
        e = hipStreamEndCapture(h->cap_stream, &g->graph);
        if (rc) { g->reset(); return rc; }
        if (e != hipSuccess) { g->reset(); return hipfail(e, "hipStreamEndCapture"); }
        e = hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0);
        if (e != hipSuccess) { g->reset(); return hipfail(e, "hipGraphInstantiate"); }
        g->key = key;
    }
    const hipError_t e = hipGraphLaunch(g->exec, s);
    if (e != hipSuccess) return hipfail(e, "hipGraphLaunch");
    return LSPF2F_OK;
}

int lspf2f_debug_poison(lspf2f_handle *h, unsigned char byte, void *hip_stream, unsigned *nonzero_counters)
{
    if (!h) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "null handle");
    if (!h->ws) return fail(LSPF2F_ERR_STATE, "workspace not bound (lspf2f_bind_workspace)");
    const Plan &P = h->plan;
    if (h->ws_size < P.persistent_bytes()) return fail(LSPF2F_ERR_STATE, "workspace too small");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    hipError_t e = hipSuccess;
    // head of the workspace: [slot 0: per-person candidate cache][slot 1: per-forward candidate slot][arrival counters]; everything behind is scratch
    const size_t cc = P.cand_cache_bytes();
    if (!h->cand_cached) e = hipMemsetAsync(h->ws, byte, cc, s);
    if (e == hipSuccess) e = hipMemsetAsync(h->ws + cc, byte, cc, s);
    if (e == hipSuccess && h->ws_size > P.persistent_bytes()) e = hipMemsetAsync(h->ws + P.persistent_bytes(), byte, h->ws_size - P.persistent_bytes(), s);
    if (e != hipSuccess) return hipfail(e, "hipMemsetAsync (poison)");
    if (nonzero_counters) {
        *nonzero_counters = 0;
        if (h->counters_clean) {          // (before the first forward on this binding the counters are whatever the allocation held: nothing to check)
            std::vector<unsigned> host(Plan::kTileCounters);
            e = hipMemcpyAsync(host.data(), h->ws + P.counters_offset(), Plan::kTileCounters * sizeof(unsigned), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) return hipfail(e, "read-back of the split-K arrival counters");
            for (unsigned v : host) *nonzero_counters += v != 0;
            return LSPF2F_OK;
        }
    }
    e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hipfail(e, "hipStreamSynchronize (poison)");
    return LSPF2F_OK;
}

int lspf2f_set_candidates(lspf2f_handle *h, const float *cand_dev, void *hip_stream)
{
    if (!h) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "null handle");
    if (!cand_dev) { h->cand_cached = nullptr; return LSPF2F_OK; }
    const Plan &P = h->plan;
    if (P.input_nc == P.feat_nc || P.feat_nc == 0) return fail(LSPF2F_ERR_UNSUPPORTED, "no candidate channels to cache");
    if (!h->blob || !h->ws) return fail(LSPF2F_ERR_STATE, "bind weights and workspace first");
    if (h->ws_size < P.cand_cache_bytes()) return fail(LSPF2F_ERR_STATE, "workspace too small");
    const LayerDesc &l = P.layers[0];
    FirstConvParams c{};
    c.feat = nullptr; c.cand = cand_dev; c.w = reinterpret_cast<const float *>(h->blob + l.form_off[kFormRows]);
    c.out = reinterpret_cast<float *>(h->ws);
    c.B = 1; c.H = l.hs; c.W = l.hs; c.feat_nc = P.feat_nc; c.cand_nc = P.input_nc - P.feat_nc; c.cand_batch = 1;
    c.Cout = l.cout; c.ci_begin = P.feat_nc; c.ci_end = P.input_nc; c.base = nullptr; c.relu = 0;
    c.force_direct = h->first_direct;
    const hipError_t e = launch_first_conv(c, static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess) return hipfail(e, "lspf2f_set_candidates launch");
    h->cand_cached = cand_dev;
    return LSPF2F_OK;
}

// Duration of a SUBSET of the forward's launches without host gaps: the selected layers are captured, in network order, into one graph
// that is replayed `reps` times between two ordinary events on `hip_stream` (events recorded by graph nodes cannot be timed on ROCm 7.2,
// so a kernel cannot be bracketed inside the replay of the whole forward).  part[i]: 0 = skip layer i, 1 = its main kernel(s) only (a
// split-K layer without its reduce launch), 2 = only its split-K reduce launch, 3 = everything the layer launches.  The layers read
// what the last forward left in the workspace (run one first); results are not meaningful, durations are.
int lspf2f_subset_timed(lspf2f_handle *h, const float *feat_dev, const float *cand_dev, int cand_batch, float *out_dev, int batch,
                        void *hip_stream, const int *part, int reps, float *ms_per_replay, int *launches_per_replay)
{
    if (!part || !ms_per_replay || reps < 1) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "null part / ms_per_replay, or reps < 1");
    int rc = check_forward_args(h, feat_dev, cand_dev, cand_batch, out_dev, batch);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if ((rc = clean_counters(h, s)) != 0) return rc;
    const int n = (int)h->plan.layers.size();
    if (!h->cap_stream) {
        const hipError_t e = hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking);
        if (e != hipSuccess) return hipfail(e, "hipStreamCreateWithFlags");
    }
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int launches = 0;
    hipError_t e = hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeThreadLocal);
    for (int i = 0; i < n && !rc && e == hipSuccess; ++i) {
        if (!part[i]) continue;
        h->timing_part = part[i];
        rc = run_layer(h, h->plan.layers[i], feat_dev, cand_dev, cand_batch, out_dev, nullptr, batch, h->cap_stream);
        ++launches;
    }
    h->timing_part = 3;
    const hipError_t e2 = hipStreamEndCapture(h->cap_stream, &graph);
    if (!rc && e != hipSuccess) rc = hipfail(e, "hipStreamBeginCapture");
    if (!rc && e2 != hipSuccess) rc = hipfail(e2, "hipStreamEndCapture");
    if (!rc && !launches) rc = fail(LSPF2F_ERR_INVALID_ARGUMENT, "empty selection");
    if (!rc && (e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0)) != hipSuccess) rc = hipfail(e, "hipGraphInstantiate");
    if (!rc && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)) rc = fail(LSPF2F_ERR_HIP, "hipEventCreate failed");
    if (!rc && (e = hipGraphLaunch(exec, s)) != hipSuccess) rc = hipfail(e, "hipGraphLaunch");          // warm-up replay
    if (!rc) {
        (void)hipEventRecord(e0, s);
        for (int r = 0; r < reps && e == hipSuccess; ++r) e = hipGraphLaunch(exec, s);
        (void)hipEventRecord(e1, s);
        if (e != hipSuccess) rc = hipfail(e, "hipGraphLaunch");
    }
    if (!rc && (e = hipStreamSynchronize(s)) != hipSuccess) rc = hipfail(e, "hipStreamSynchronize");
    if (!rc) {
        float ms = 0.f;
        if ((e = hipEventElapsedTime(&ms, e0, e1)) != hipSuccess) rc = hipfail(e, "hipEventElapsedTime");
        *ms_per_replay = ms / (float)reps;
        if (launches_per_replay) *launches_per_replay = launches;
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (exec) (void)hipGraphExecDestroy(exec);
    if (graph) (void)hipGraphDestroy(graph);
    return rc;
}

int lspf2f_forward_timed(lspf2f_handle *h, const float *feat_dev, const float *cand_dev, int cand_batch,
                         float *out_dev, int batch, void *hip_stream, float *ms_per_layer)
{
    if (!ms_per_layer) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "null ms_per_layer");
    int rc = check_forward_args(h, feat_dev, cand_dev, cand_batch, out_dev, batch);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if ((rc = clean_counters(h, s)) != 0) return rc;
    const int n = (int)h->plan.layers.size();
    std::vector<hipEvent_t> ev(n + 1);
    for (auto &e : ev)
        if (hipEventCreate(&e) != hipSuccess) return fail(LSPF2F_ERR_HIP, "hipEventCreate failed");
    (void)hipEventRecord(ev[0], s);
    for (int i = 0; i < n && !rc; ++i) {
        rc = run_layer(h, h->plan.layers[i], feat_dev, cand_dev, cand_batch, out_dev, nullptr, batch, s);
        (void)hipEventRecord(ev[i + 1], s);
    }
    const hipError_t e = hipStreamSynchronize(s);
    if (!rc && e != hipSuccess) rc = hipfail(e, "hipStreamSynchronize");
    if (!rc)
        for (int i = 0; i < n; ++i) (void)hipEventElapsedTime(&ms_per_layer[i], ev[i], ev[i + 1]);
    for (auto &x : ev) (void)hipEventDestroy(x);
    return rc;
}

// ---- lspf2f_conv3x3: one conv on the kernel its tile code names (include/lspf2f.h) ----
// The code, decoded once for lspf2f_conv3x3_scratch_bytes, conv3x3_run and conv3x3_in_shape.  Precedence = the order of the lines of decode_tile().
struct TileCode {
    ConvRoute route;      // the kernel the code forces; kRouteIgemm = the implicit GEMM on tile_m x tile_n tiles (0 x 0: the planner's tiling)
    int arg;              // that kernel's LayerDesc::route_arg
    int bn;               // conv3x3_patch16: channels per workgroup = tile_n, with 65 = 64 in its FIRST form
    bool planner;         // tile 0 x 0 with split_k 0: the planner's rules may also give the call to the tiny-M or the full-K kernel
    bool kernel_order;    // k_group -1: w_packed is in the kernel's own (fragment / tile-blocked) order, not rows [cout][9][cin]
    bool k8;              // a Winograd code: the K step is 8 channels (checked by *_supported()), not a K-tile of 32 | 64
};
static TileCode decode_tile(int tile_m, int tile_n, int split_k, int k_group, int dtype)
{
    const bool own = k_group == -1;
    TileCode t{kRouteIgemm, 0, tile_n == 65 ? 64 : tile_n, false, own, own && ((tile_m >= 4001 && tile_m <= 4003) || tile_m == 5001 || tile_m == 5002 || tile_m == 6001)};
    auto is = [&t](ConvRoute r, int arg) { t.route = r; t.arg = arg; return t; };
    if (tile_m == 1 && tile_n == 1) return is(kRouteSmallM, 1);                                    // tiny-M single-launch kernel
    if (tile_m > 3000 && tile_n == 64 && own) return is(kRouteRowUp, tile_m - 3000);               // 3000 + R: sub-pixel up-conv row kernel, R low-res rows per strip
    if ((tile_m == 5001 || tile_m == 5002) && own) return is(kRouteWinoUp, tile_m - 5000);         // 5000 + nb: up-conv Winograd kernel; split_k = K splits (0: 1)
    if (tile_m == 6001 && own) return is(kRouteWino4, 1);                                          // Winograd F(4x4, 3x3), weights as pack_wino4_weights(); split_k likewise
    if (t.k8) return is(kRouteWino, tile_m == 4002 ? 2 : 1);                                       // 4000 + nb: Winograd F(2x2, 3x3); 4003 = nb 1 with the U fragments in registers
    if (tile_m == 7164 || tile_m == 7132 || tile_m == 7116) return is(kRoutePatchUp16, tile_m - 7100);   // 7100 + tile width: conv3x3_patchup16 (upsample 2, w_packed = [4][cout][2][2][c0 + c1])
    if (tile_m == 7064 || tile_m == 7032) return is(kRoutePatch16, tile_m - 7000);                 // 7000 + tile width: conv3x3_patch16, tile_n = 128 | 64 | 65 channels per workgroup; igemm weight rows
    if (tile_m == 2000 && own) return is(kRouteBand, 1);                                           // activation-stationary 16-bit kernel of the 16x16 / 8x8 levels
    if (tile_m > 1000 && (tile_n == 64 || tile_n == 128)) return is(kRouteRowConv, tile_m - 1000); // 1000 + R: weights-stationary 16-bit kernel, tile_n channels in and out, R output rows per strip
    if ((tile_m == 16 || tile_m == 32) && tile_n == 16) return is(dtype ? kRouteFullK16 : kRouteFullK, tile_m / 16);   // full-K single-launch kernels, tile_m / 16 pixel blocks per tile
    t.planner = tile_m == 0 && tile_n == 0 && split_k == 0 && k_group != -4;
    return t;
}

// the layer lspf2f_conv3x3's arguments describe, for the planner's predicates and the builders above (upsample 1 = nearest x2 in front of the 9 taps, 2 = the sub-pixel form)
static LayerDesc conv3x3_layer(int hs, int c0, int c1, int cout, int stride, int upsample)
{
    LayerDesc l;
    l.hs = hs; l.ho = upsample ? 2 * hs : (stride == 2 ? (hs + 1) / 2 : hs);
    l.c0 = c0; l.c1 = c1; l.cin = c0 + c1; l.cout = cout; l.stride = stride; l.up = upsample == 1; l.up4 = upsample == 2;
    return l;
}
// its tiling on the implicit GEMM (bm, bn, splits, group): tile 0 x 0, split_k 0 and k_group 0 each take the planner's value.  Returns the K-tiles: k_group -4 keeps
// the 16 live (tap, quarter) pairs of a space-to-depth 4x4 / s2 conv
static int conv3x3_tiling(LayerDesc &l, int batch, int tile_m, int tile_n, int split_k, int k_group, int dtype)
{
    const int ktc = dtype ? 64 : 32, ktiles = k_group == -4 ? 16 * (l.c0 / 4) / ktc : (l.up4 ? 4 : 9) * l.cin / ktc;
    l.bm = tile_m; l.bn = tile_n; l.splits = split_k; l.group = k_group == -4 ? 0 : k_group;
    if (!l.bm || !l.bn || !l.splits) {
        int bm, bn, splits, group;
        choose_tiling(l.up4 ? batch * l.hs * l.hs : batch * l.ho * l.ho, l.cout, ktiles, l.up4 ? 4 : 1, l.up, dtype, &bm, &bn, &splits, &group);
        if (!l.bm || !l.bn) { l.bm = bm; l.bn = bn; if (!l.group) l.group = group; }
        if (!l.splits) l.splits = splits;
    }
    if (!l.group) l.group = 1;
    return ktiles;
}

size_t lspf2f_conv3x3_scratch_bytes(int batch, int hs, int ws, int c0, int c1, int cout, int stride, int upsample,
                                    int tile_m, int tile_n, int split_k, int k_group, int dtype)
{
    const TileCode t = decode_tile(tile_m, tile_n, split_k, k_group, dtype);
    LayerDesc L = conv3x3_layer(hs, c0, c1, cout, stride, upsample);
    const int sp = split_k > 0 ? split_k : 1;
    switch (t.route) {
    case kRouteWinoUp: return sp > 1 ? winoup_scratch(batch, hs, hs, cout, t.arg, sp).bytes() : 0;      // (slabs at OUTPUT resolution)
    case kRouteWino4: return sp > 1 ? wino4_scratch(batch, hs, ws, cout, sp).bytes() : 0;
    case kRouteWino: return sp > 1 ? wino_scratch(batch, hs, ws, cout, t.arg, sp).bytes() : 0;
    case kRoutePatch16: case kRoutePatchUp16: return 0;
    case kRouteFullK: case kRouteFullK16:
        if (split_k == 2) return fullk_split_scratch(batch, L.ho, cout, t.arg).bytes();
        break;
    default: break;
    }
    // every other selection: the implicit GEMM's slabs for the K splits asked for (0: the planner's count) -- enough for whichever kernel then takes the call
    conv3x3_tiling(L, batch, tile_m, tile_n, split_k, k_group, dtype);
    return igemm_scratch(batch * L.ho * L.ho, cout, L.splits).bytes();
}

// lspf2f_conv3x3, and with `in` the conv of lspf2f_conv3x3_instnorm: the producer then also leaves the statistics InstanceNorm plans take from it -- per-group sums at
// in->psum / psq / pshift ([B][in->groups][cout], bound and sized by the caller) from the implicit GEMM and the Winograd kernels, the normalisation itself from the
// tiny-M kernel.  The caller has checked that (tile, k_group) names one of those producers.
static int conv3x3_run(const void *src0, const void *src1, const void *w_packed, const float *scale,
                       const float *shift, const void *residual, void *out, int batch, int hs, int ws, int c0,
                       int c1, int cout, int stride, int upsample, int relu, int tile_m, int tile_n, int split_k,
                       int k_group, int dtype, void *scratch, size_t scratch_bytes, void *hip_stream, const InstNormParams *in)
{
    if (dtype < 0 || dtype > 2) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "dtype must be 0 (fp32), 1 (bf16) or 2 (fp16)");
    const int ktc = dtype ? 64 : 32;
    if (!src0 || !w_packed || !out) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "null argument");
    if (hs != ws) return fail(LSPF2F_ERR_UNSUPPORTED, "square tensors only");
    const TileCode t = decode_tile(tile_m, tile_n, split_k, k_group, dtype);
    if (!t.k8 && ((c0 % ktc) || (c1 % ktc) || c0 <= 0 || c1 < 0 || (c1 > 0 && !src1)))
        return fail(LSPF2F_ERR_UNSUPPORTED, "channel counts must be multiples of 32 (fp32) / 64 (bf16, fp16)");
    if (cout % 4 && !(t.route == kRouteSmallM && cout % 2 == 0)) return fail(LSPF2F_ERR_UNSUPPORTED, "cout must be a multiple of 4");     // (the tiny-M kernel: channel pairs)
    if (stride != 1 && stride != 2) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "stride must be 1 or 2");
    if (upsample && stride != 1) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "upsample requires stride 1");
    if ((scale == nullptr) != (shift == nullptr)) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "scale and shift come together");
    if (k_group == -4) {
        // The masked 16-of-36 tap operand of a space-to-depth 4x4 / s2 conv ([cout][16][ci]) is an IMPLICIT-GEMM form only: checked here, before any other route
        // (Winograd, full-K, row / band kernels read w_packed as a dense 9-tap operand) can take the call
        if (dtype != 0 || stride != 1 || upsample || c1 || c0 % 4 || (c0 / 4) % ktc)
            return fail(LSPF2F_ERR_UNSUPPORTED, "k_group -4 (space-to-depth 4x4 / s2 taps): fp32, one source of 4 x ci channels, ci a multiple of 32");
        const bool gemm_tile = (tile_m == 0 && tile_n == 0) || ((tile_m == 32 || tile_m == 64 || tile_m == 128) && (tile_n == 64 || tile_n == 128));
        if (!gemm_tile) return fail(LSPF2F_ERR_UNSUPPORTED, "k_group -4 runs on the implicit GEMM only: tile 0x0 (planner's choice) or one of its tiles");
    }
    if (upsample < 0 || upsample > 2) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "upsample must be 0, 1 or 2");
    LayerDesc L = conv3x3_layer(hs, c0, c1, cout, stride, upsample);
    L.route = t.route; L.route_arg = t.arg; L.splits = split_k > 0 ? split_k : 1;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    ConvIO io{src0, c1 ? src1 : nullptr, w_packed, scale, shift, residual, out, nullptr, nullptr, batch, dtype, relu, t.kernel_order};
    // a route's split-K scratch: bounds-checked, then bound -- the slabs, and behind them the arrival counters (zero on entry; every launch leaves them zero)
    auto bind_scratch = [&](const SplitKScratch &k) {
        if (!scratch || scratch_bytes < k.bytes()) return false;
        io.partial = static_cast<float *>(scratch);
        io.tile_cnt = reinterpret_cast<unsigned *>(static_cast<char *>(scratch) + k.slab_bytes);
        return true;
    };
    auto launched = [](hipError_t e, const char *what) { return e == hipSuccess ? (int)LSPF2F_OK : hipfail(e, what); };
    if (t.route == kRouteSmallM || t.planner) {
        SmallMParams q = smallm_params(io, L);
        q.in_fused = in ? 1 : 0;
        if (t.route == kRouteSmallM && k_group > 0) {           // the forms of the tile 1 x 1 code (include/lspf2f.h)
            q.runtime_geo = k_group & 1;
            if ((k_group & 2) && dtype == 0 && !in) { q.pf = w_packed; q.pf_bytes = (unsigned)((size_t)cout * 9 * c0 * sizeof(float)); }
        }
        if (c1 == 0 && upsample != 2 && smallm_supported(q)) return launched(launch_smallm(q, s), "lspf2f_conv3x3 (tiny-M) launch");
        if (!t.planner) return fail(LSPF2F_ERR_UNSUPPORTED, "tiny-M kernel does not support this shape");
    }
    switch (t.route) {
    case kRouteRowUp: {
        const RowUpParams q = rowup_params(io, L);
        if (!rowup_layer(L, dtype) || residual || !rowup_supported(q) || (q.R & 1))
            return fail(LSPF2F_ERR_UNSUPPORTED, "the bf16 up-conv row kernel does not support this shape");
        return launched(launch_rowup(q, s), "lspf2f_conv3x3 (rowup) launch");
    }
    case kRouteWinoUp: {
        if (L.splits > 1 && !bind_scratch(winoup_scratch(batch, hs, ws, cout, t.arg, L.splits))) return fail(LSPF2F_ERR_STATE, "split-K scratch missing or too small");
        WinoUpParams q = winoup_params(io, L);
        if (in) { q.psum = in->psum; q.psq = in->psq; q.pshift = in->pshift; }
        if (dtype != 0 || stride != 1 || !upsample || residual || !winoup_supported(q, t.arg))
            return fail(LSPF2F_ERR_UNSUPPORTED, "the up-conv Winograd kernel does not support this shape");
        return launched(launch_winoup(q, t.arg, s), "lspf2f_conv3x3 (winoup) launch");
    }
    case kRouteWino4:
    case kRouteWino: {
        const bool f4 = t.route == kRouteWino4;
        const SplitKScratch k = f4 ? wino4_scratch(batch, hs, ws, cout, L.splits) : wino_scratch(batch, hs, ws, cout, t.arg, L.splits);
        if (L.splits > 1 && !bind_scratch(k)) return fail(LSPF2F_ERR_STATE, "split-K scratch missing or too small");
        WinoParams q = wino_params(io, L);
        q.ureg = tile_m == 4003;      // 4003: nb = 1 with the U fragments in registers (the form the plans take), 4001: through LDS
#ifdef LSPF2F_WINO_STAMPS
        {   // stamps live behind slabs and counters when the caller's scratch has room for them
            const size_t used = (k.bytes() + 255) / 256 * 256;
            const size_t blocks = k.counters * (size_t)L.splits;
            if (scratch && scratch_bytes >= used + blocks * 4 * 8 * 8) q.stamps = reinterpret_cast<unsigned long long *>(static_cast<char *>(scratch) + used);
        }
#endif
        if (in) { q.psum = in->psum; q.psq = in->psq; q.pshift = in->pshift; }
        if (dtype != 0 || c1 != 0 || stride != 1 || upsample != 0 || !(f4 ? wino4_supported(q) : wino_supported(q, t.arg)))
            return fail(LSPF2F_ERR_UNSUPPORTED, f4 ? "the Winograd F(4x4,3x3) kernel does not support this shape" : "the Winograd kernel does not support this shape");
        return f4 ? launched(launch_wino4(q, s), "lspf2f_conv3x3 (wino4) launch") : launched(launch_wino(q, t.arg, s), "lspf2f_conv3x3 (wino) launch");
    }
    case kRoutePatchUp16: {
        const PatchConvParams q = patch_params(io, L);
        if (stride != 1 || upsample != 2 || !patchup16_supported(q, t.arg, tile_n))
            return fail(LSPF2F_ERR_UNSUPPORTED, "the patch-staged 16-bit up-conv kernel does not support this shape");
        return launched(launch_patchup16(q, t.arg, tile_n, s), "lspf2f_conv3x3 (patchup16) launch");
    }
    case kRoutePatch16: {
        PatchConvParams q = patch_params(io, L);
        q.deep = tile_n == 64;                  // tile_n 65 = 64 channels per workgroup in the FIRST form (copies in the load segment, 3-slot ring; A-B runs, the ablation and stamp builds)
#ifdef LSPF2F_ABLATE
        q.dbg = ablate_dbg();
#endif
#ifdef LSPF2F_PATCH_STAMPS
        if (scratch && scratch_bytes >= (size_t)4096 * 8 * 8 * 8) q.stamps = static_cast<unsigned long long *>(scratch);
#endif
        if (c1 != 0 || stride != 1 || upsample != 0 || !patch16_supported(q, t.arg, t.bn))
            return fail(LSPF2F_ERR_UNSUPPORTED, "the patch-staged 16-bit kernel does not support this shape");
        return launched(launch_patch16(q, t.arg, t.bn, s), "lspf2f_conv3x3 (patch16) launch");
    }
    case kRouteBand: {
        const BandConvParams q = band_params(io, L);
        if (!bandconv_layer(L, dtype) || !bandconv_supported(q)) return fail(LSPF2F_ERR_UNSUPPORTED, "the bf16 band kernel does not support this shape");
        return launched(launch_bandconv(q, s), "lspf2f_conv3x3 (bandconv) launch");
    }
    case kRouteRowConv: {
        const RowConvParams q = rowconv_params(io, L);
        if (!rowconv_layer(L, dtype) || c0 != tile_n || !rowconv_supported(q)) return fail(LSPF2F_ERR_UNSUPPORTED, "the bf16 row kernel does not support this shape");
        return launched(launch_rowconv(q, s), "lspf2f_conv3x3 (rowconv) launch");
    }
    case kRouteFullK16: {
        const FullK16Params q = fullk16_params(io, L);
        if (upsample == 2 || !fullk16_supported(q, t.arg)) return fail(LSPF2F_ERR_UNSUPPORTED, "the 16-bit full-K kernel does not support this shape");
        return launched(launch_fullk16(q, t.arg, s), "lspf2f_conv3x3 (full-K, 16-bit) launch");
    }
    default: break;
    }
    // the fp32 full-K kernel: forced by its tile, or picked by the planner's rule (tile 0x0 + split 0).  split_k 2 = K halves; a single source's w_packed is then packed as two half-sources
    if (const int pb = t.route == kRouteFullK ? t.arg : t.planner ? fullk_choice(L, batch, dtype) : 0) {
        if (L.splits == 2 && !bind_scratch(fullk_split_scratch(batch, L.ho, cout, pb))) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "scratch too small for the K-split full-K kernel");
        FullKParams q = fullk_params(io, L);
#ifdef LSPF2F_FULLK_STAMPS
        q.stamps = scratch_bytes >= (size_t)512 * 4 * 16 * 8 ? static_cast<unsigned long long *>(scratch) : nullptr;
#endif
        if (dtype != 0 || (stride != 1 && !(stride == 2 && q.split == 2)) || upsample == 2 || !fullk_supported(q, pb))
            return fail(LSPF2F_ERR_UNSUPPORTED, "full-K kernel does not support this shape");
        return launched(launch_fullk(q, pb, s), "lspf2f_conv3x3 (full-K) launch");
    }
    // the implicit GEMM on the tiles asked for; 0 x 0, split_k 0 and k_group 0 each take the planner's value
    const int kt = conv3x3_tiling(L, batch, tile_m, tile_n, split_k, k_group, dtype);
    if (!igemm_group_supported(L.bm, L.bn, L.group, L.up)) return fail(LSPF2F_ERR_UNSUPPORTED, "tile shape / k_group not instantiated");
    if (L.splits < 1 || L.splits > kt) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "bad split_k");
    const int per = (kt + L.splits - 1) / L.splits, sp = L.splits = (kt + per - 1) / per;      // no empty slice
    if (in) {
        // epilogue sums: the planner's own precondition (a wave's rows inside one frame, one K slice), and the group count the caller sized the statistics for
        const int rhw = L.up4 ? hs * hs : L.ho * L.ho;
        if (!in_fused_eligible(L.bm, sp, rhw) || in->groups != (L.up4 ? 4 : 1) * rhw / in_fused_wave_rows(L.bm))
            return fail(LSPF2F_ERR_UNSUPPORTED, "the implicit GEMM gathers InstanceNorm statistics in its epilogue only with one K slice, >= 1024 pixels per frame and whole waves per frame");
    }
    if (sp > 1 && !bind_scratch(igemm_scratch(batch * L.ho * L.ho, cout, sp))) return fail(LSPF2F_ERR_STATE, "split-K scratch missing or too small");
    IgemmParams p = igemm_params(io, L);
    if (in) { p.psum = in->psum; p.psq = in->psq; p.pshift = in->pshift; p.in_groups = in->groups; }
    if (k_group == -4) {
        // Conv2d(k4, s2, p1) as a 3x3 conv on the space-to-depth image (c0 = 4 ci, channel = (dy * 2 + dx) * ci + c): tap row ty reads sub-rows {1}, {0, 1}, {0} for
        // ty = 0, 1, 2 (columns alike), so 16 of the 36 (tap, quarter) pairs carry weights; w_packed = [cout][those 16 in tap-major order][ci]
        static const unsigned sub[3] = {2u, 3u, 1u};          // live sub-rows of tap row 0, 1, 2 as a bit set over dy
        for (int ty = 0; ty < 3; ++ty)
            for (int tx = 0; tx < 3; ++tx)
                for (int dy = 0; dy < 2; ++dy)
                    for (int dx = 0; dx < 2; ++dx)
                        if (((sub[ty] >> dy) & 1u) && ((sub[tx] >> dx) & 1u)) p.kmask |= 1ull << ((ty * 3 + tx) * 4 + dy * 2 + dx);
        p.kblk = c0 / 4; p.ktiles_total = kt; p.ktiles_per_split = per;
    }
#ifdef LSPF2F_ABLATE
    p.dbg = ablate_dbg();   // tools/ablate.sh builds only
#endif
#ifdef LSPF2F_IGEMM_STAMPS
    if (sp == 1 && scratch && scratch_bytes >= (size_t)2048 * 4 * 16 * 8) p.stamps = static_cast<unsigned long long *>(scratch);
#endif
    hipError_t e = launch_igemm(p, L.bm, L.bn, L.group, s);
    if (e == hipSuccess && sp > 1) e = launch_splitk_reduce(p, s);
    return launched(e, "lspf2f_conv3x3 launch");
}

int lspf2f_conv3x3(const void *src0, const void *src1, const void *w_packed, const float *scale,
                   const float *shift, const void *residual, void *out, int batch, int hs, int ws, int c0,
                   int c1, int cout, int stride, int upsample, int relu, int tile_m, int tile_n, int split_k,
                   int k_group, int dtype, void *scratch, size_t scratch_bytes, void *hip_stream)
{
    return conv3x3_run(src0, src1, w_packed, scale, shift, residual, out, batch, hs, ws, c0, c1, cout, stride, upsample, relu, tile_m, tile_n, split_k, k_group, dtype,
                       scratch, scratch_bytes, hip_stream, nullptr);
}

// ---- InstanceNorm, layer by layer (tests/test_gpu_instnorm_layer.py) ----

static size_t in_route_groups(int hw, int route) { return route == 1 ? (size_t)(hw + 63) / 64 : 0; }

size_t lspf2f_instance_norm_scratch_bytes(int batch, int hw, int c, int route)
{
    if (batch < 1 || hw < 1 || c < 1 || route != 1) return 0;                 // the one-launch route keeps nothing in memory
    return ((size_t)3 * in_route_groups(hw, route) + 2) * batch * c * sizeof(float);
}

int lspf2f_instance_norm(float *x, const float *partial, int splits, const float *bias, const float *residual, int relu, int batch, int hw, int c, int route,
                         int three_pass, float *mean_out, float *rstd_out, void *scratch, size_t scratch_bytes, void *hip_stream)
{
    if (!x) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "instance_norm: null x");
    if (route != 0 && route != 1) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "instance_norm: route must be 0 (small) or 1 (reduce)");
    if (splits < 1 || (splits > 1 && !partial)) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "instance_norm: splits >= 1, and partial slabs when splits > 1");
    if (route == 0 && (mean_out || rstd_out)) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "instance_norm: the one-launch route keeps its statistics in registers: mean_out / rstd_out must be null");
    if (batch < 1 || hw < 1) return fail(LSPF2F_ERR_UNSUPPORTED, "instance_norm: batch and hw must be >= 1");
    if (c < 4 || c % 4) return fail(LSPF2F_ERR_UNSUPPORTED, "instance_norm: the channel count must be a multiple of 4");
    if (route == 1 && c / 4 > 256) return fail(LSPF2F_ERR_UNSUPPORTED, "instance_norm: the reduce route takes at most 1024 channels (256 channel quads per workgroup)");
    const size_t need = lspf2f_instance_norm_scratch_bytes(batch, hw, c, route);
    if (need && (!scratch || scratch_bytes < need)) return fail(LSPF2F_ERR_STATE, "instance_norm: statistics scratch missing or smaller than lspf2f_instance_norm_scratch_bytes()");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    InstNormParams q{};
    q.three_pass = three_pass ? 1 : 0;
    q.x = x; q.residual = residual; q.relu = relu; q.partial = splits > 1 ? partial : nullptr; q.splits = splits; q.bias = bias;
    q.B = batch; q.hw = hw; q.C = c;
    hipError_t e = in_standalone(q, route == 0, static_cast<float *>(scratch), (size_t)batch * in_route_groups(hw, route), s);
    if (e == hipErrorInvalidValue) return fail(LSPF2F_ERR_UNSUPPORTED, "instance_norm: the launcher refused this shape");
    if (e == hipSuccess && mean_out) e = hipMemcpyAsync(mean_out, q.mean, (size_t)batch * c * sizeof(float), hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && rstd_out) e = hipMemcpyAsync(rstd_out, q.rstd, (size_t)batch * c * sizeof(float), hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return hipfail(e, "lspf2f_instance_norm launch");
    return LSPF2F_OK;
}

// B, hw, C, groups and rows_per_group of the InstanceNorm behind the conv a tile code of lspf2f_conv3x3 names, and the kernel that produces its statistics; "" or why
// the selection is refused
static const char *conv3x3_in_shape(int batch, int hs, int ws, int cout, int stride, int upsample, int tile_m, int tile_n, int split_k, int k_group, int dtype,
                                    ConvRoute *prod, InstNormParams *q)
{
    *prod = decode_tile(tile_m, tile_n, split_k, k_group, dtype).route;
    const bool gemm_stats = (tile_m == 128 || tile_m == 64 || tile_m == 32) && tile_n == 64 && k_group >= 0;      // (of the implicit GEMM's tiles, the 64-column ones)
    if (*prod != kRouteSmallM && *prod != kRouteWino && *prod != kRouteWinoUp && !(*prod == kRouteIgemm && gemm_stats))
        return "conv3x3_instnorm: the statistics producers are the implicit GEMM (tile 128 | 64 | 32 x 64), wino3x3 (4001 .. 4003), winoup3x3 (5001, 5002) and the tiny-M kernel (1 x 1)";
    if (dtype != 0) return "conv3x3_instnorm: InstanceNorm plans are fp32 only";
    if (batch < 1 || hs < 1 || hs != ws || cout < 4 || cout % 4 || (stride != 1 && stride != 2) || upsample < 0 || upsample > 2) return "conv3x3_instnorm: bad shape";
    const int ho = upsample ? 2 * hs : (stride == 2 ? (hs + 1) / 2 : hs);
    q->B = batch; q->hw = ho * ho; q->C = cout; q->groups = 0; q->rows_per_group = 0;
    if (*prod == kRouteIgemm) {
        const int rhw = upsample == 2 ? hs * hs : ho * ho;
        if (split_k != 1 || !in_fused_eligible(tile_m, split_k, rhw))
            return "conv3x3_instnorm: the implicit GEMM gathers InstanceNorm statistics in its epilogue only with split_k 1, >= 1024 pixels per frame and whole waves per frame";
        in_groups_igemm(*q, tile_m, upsample == 2, rhw);
    } else if (*prod != kRouteSmallM) {
        if (q->hw % 128) return "conv3x3_instnorm: the Winograd kernels leave one group per tile-block of 128 output pixels";
        in_groups_wino(*q);
    }
    return "";
}
// [cout] ones (the scale the conv bias rides on, as the packer writes it for InstanceNorm plans), then the statistics as in_bind_stats lays them out
size_t lspf2f_conv3x3_instnorm_scratch_bytes(int batch, int hs, int ws, int c0, int c1, int cout, int stride, int upsample, int tile_m, int tile_n, int split_k, int k_group,
                                             int dtype)
{
    (void)c0; (void)c1;
    ConvRoute prod;
    InstNormParams q{};
    if (*conv3x3_in_shape(batch, hs, ws, cout, stride, upsample, tile_m, tile_n, split_k, k_group, dtype, &prod, &q)) return 0;
    const size_t stats = prod == kRouteSmallM ? 0 : ((size_t)3 * q.groups + 2) * batch * cout;
    return ((size_t)cout + stats) * sizeof(float);
}

int lspf2f_conv3x3_instnorm(const void *src0, const void *src1, const void *w_packed, const float *bias, const void *residual, void *out, int batch, int hs, int ws,
                            int c0, int c1, int cout, int stride, int upsample, int relu, int tile_m, int tile_n, int split_k, int k_group, int dtype,
                            void *scratch, size_t scratch_bytes, void *stats, size_t stats_bytes, void *hip_stream)
{
    if (!src0 || !w_packed || !out) return fail(LSPF2F_ERR_INVALID_ARGUMENT, "null argument");
    ConvRoute prod;
    InstNormParams q{};
    const char *why = conv3x3_in_shape(batch, hs, ws, cout, stride, upsample, tile_m, tile_n, split_k, k_group, dtype, &prod, &q);
    if (*why) return fail(LSPF2F_ERR_UNSUPPORTED, why);
    const size_t need = lspf2f_conv3x3_instnorm_scratch_bytes(batch, hs, ws, c0, c1, cout, stride, upsample, tile_m, tile_n, split_k, k_group, dtype);
    if (!stats || stats_bytes < need || reinterpret_cast<uintptr_t>(stats) % 16)
        return fail(LSPF2F_ERR_STATE, "conv3x3_instnorm: statistics scratch missing, misaligned or smaller than lspf2f_conv3x3_instnorm_scratch_bytes()");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    float *ones = static_cast<float *>(stats);
    if (bias) {
        const hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ones), 0x3f800000, (size_t)cout, s);      // 1.0f
        if (e != hipSuccess) return hipfail(e, "lspf2f_conv3x3_instnorm (scale) memset");
    }
    q.three_pass = 0;
    q.x = static_cast<float *>(out); q.residual = static_cast<const float *>(residual); q.relu = relu; q.partial = nullptr; q.splits = 1; q.bias = nullptr;
    in_bind_stats(q, ones + cout, (size_t)batch * q.groups);
    // the tiny-M kernel normalises (+ residual, ReLU) in its own epilogue; behind the others the residual add and the ReLU follow the normalisation, in in_apply
    const bool tiny = prod == kRouteSmallM;
    const int rc = conv3x3_run(src0, src1, w_packed, bias ? ones : nullptr, bias, tiny ? residual : nullptr, out, batch, hs, ws, c0, c1, cout, stride, upsample, tiny ? relu : 0,
                               tile_m, tile_n, split_k, k_group, dtype, scratch, scratch_bytes, hip_stream, &q);
    if (rc != LSPF2F_OK || tiny) return rc;
    const hipError_t e = in_finalize_apply(q, s);
    if (e == hipErrorInvalidValue) return fail(LSPF2F_ERR_UNSUPPORTED, "conv3x3_instnorm: the launcher refused this shape");
    if (e != hipSuccess) return hipfail(e, "lspf2f_conv3x3_instnorm (finalize / apply) launch");
    return LSPF2F_OK;
}


}  // extern "C"
