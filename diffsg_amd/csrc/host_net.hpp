// Part of the ONE translation unit dsg_api.hip (included from there, after the kernel headers and `using namespace dsg`): not a
// stand-alone header.  The net description: error reporting, the operator plan and parameter layout (create_impl, carve), the handle, the forward workspace.
#pragma once

namespace {

thread_local std::string g_err;

int fail(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return 1;
}

#define HIPCK(expr)                                                                          \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

inline int cdiv(int a, int b) { return (a + b - 1) / b; }
inline int pad32(int n) { return cdiv(n, 32) * 32; }
inline int groups_of(int w) { return cdiv(w, 8); }

struct Param {
    std::string name;
    long long numel;
    long long off;  // offset in the flat state-dict-order buffer (gradient bucket)
    const float* ptr = nullptr;
};

struct LinearP {           // nn.Linear
    int N = 0, K = 0;
    int w = -1, b = -1;    // param indices
};
struct NormP { int w = -1, b = -1; };

struct ResP {              // ResidualBlock (UNetCF.py:49-95)
    int in0 = 0, in1 = 0, N = 0;
    bool sclin = false;
    NormP n1, n2, n3;
    LinearP l1, l2, l3, sc, te, ce;
    int tb_off = 0;        // slice of the time table row
    size_t ce_off = 0;     // per-tile float offset of this block's precomputed condition embedding
    // packed (arena offsets, floats)
    size_t W1p, g1p, b1p, W2p, g2p, b2p, c2p, Wcp, W3p, g3p, b3p, c3p, Wscp;
    size_t W1T, W2T, W3T, WscT;  // transposed packs (data gradients)
    size_t W1h = 0, W2h = 0, W3h = 0, Wsch = 0;  // fp16-split planes (blocks >= 64 wide, sampling)
    size_t W1Th = 0, W2Th = 0, W3Th = 0, WscTh = 0;  // transposed fp16-split planes (data gradients)
    size_t Wch = 0;        // fp16-split planes of the condition embedding
    bool split = false;
    // training workspace (per-tile float offsets)
    size_t h1, h2, du1, dh1, dh2, rs1, rs2, rs3;
    size_t cs_off = 0, cs_stride = 0;   // this block's column-sum region (float offset in tr_cs) and its per-tile row length
    int gslot_out = -1, gslot_h2 = -1, gslot_h1 = -1;   // max|G| slots of dout, dh2, dh1
    long long dtb_off;     // slab scratch: dTB_b [N][T]
};

struct LinOpP {            // feature_proj / Down/Upsample / final
    LinearP l;
    NormP ln;              // final only
    bool lnact = false;
    size_t Wp, bp, gp, betap, WT;
    size_t Wh = 0;         // fp16-split planes
    size_t du, rs;         // final only (training)
};

struct AttnP {             // AttentionBlock on a sequence of length 1 (UNetCF.py:98-157, dsg_attn.hpp)
    int N = 0;
    NormP norm;            // registered, never called by the reference's forward: its gradients are exact zeros
    LinearP proj, out;     // projection (d -> 3d: only rows 2d:3d = Wv reach the output), output (d -> d)
    size_t Wvp = 0, bvp = 0, Wop = 0, bop = 0, WvT = 0, WoT = 0;   // packed (arena offsets, floats)
    size_t Wvh = 0, Woh = 0;   // fp16-split planes (>= 64 wide: k_attn_h)
    size_t v = 0, dv = 0;  // training workspace (per-tile float offsets): v = Wv x + bv of the forward, dv = Wo^T dy of the backward
};

struct TensorInfo {
    int width;
    size_t data_off, stats_off;   // forward workspace, per-tile float offsets
    size_t ga, gb;                // training workspace: gradients from the chain / skip consumer
    bool is_skip;
};

enum OpKind { OP_PROJ, OP_RES, OP_LIN, OP_FINAL, OP_ATTN };
struct Op {
    OpKind kind;
    int p;          // index into res / lin / attn
    int in0, in1;   // tensor ids (-1: none)
    int out;        // tensor id (-1 for final)
    std::string name;
};

// launches with fewer row tiles than this leave SIMDs idle with one wave per tile (dsg_set_launch_policy)
// (narrow run: round 5 sweep, tools/policy_rows_ab.py -- at 1 536 / 2 048 tiles the small-launch form is 3-5 % of the step faster than the
// large-launch form without the LDS image: 0.489 -> 0.477 and 0.503 -> 0.479 ms per step at 24 576 / 32 768 rows; the LDS-resident form takes over above)
constexpr int kCoopMaxTilesDefault = 512, kNarrowSmallMaxTilesDefault = 2048, kCoopMaxTilesTrain = 1024;
// Persistent LDS-weight kernels (dsg_panel.hpp, dsg_res64.hpp) from this many row tiles on.  Rounds 3-4: 2 048 = 256 CUs x 8 tiles.  Round 5
// (tools/mid_batch_ab.py, same box): with the half-panel form (4-tile groups, two workgroups per CU) they beat the mid-size forms from 768
// tiles on -- 12 288 rows 0.339 -> 0.302 ms per step, 16 384: 0.356 -> 0.346, 24 576: 0.483 -> 0.454, 49 152 (3 072 tiles, where 8-tile
// groups left the second round half empty): 0.721 -> 0.674.
constexpr int kPanelMinTilesDefault = 768;

}  // namespace

constexpr int kMaxWgParts = 8;      // early parts of the weight-gradient launch (dsg_train_step)
constexpr int kWgForkMinTiles = 1024;

// One set of captured reverse steps of a workspace shape: exec[0] = one early (renorm) step, exec[1 + k] = 2^k later steps
// (runs of 1, 2, 4, 8, 16, 32), and the shape they were captured for
constexpr int kStepRunGraphs = 6;
// the kinds of a step: the plain one, and under a guidance schedule (dsg_set_step_guidance) the two-pass step with the
// scheduled update and the one-pass (unguided) step; and the same three with the history form of the update (dsg_set_step_history,
// k_update_hist, k_update_hist_sched), STEP_HIST + the kind without a history; and each of the six with the clip form of its
// update (dsg_set_xstart_clip, DESIGN.md 20: dsg_clip.hpp), STEP_CLIP + the kind without a clip.  kind % 3 == STEP_ONEPASS: one denoiser pass
enum StepKind { STEP_PLAIN = 0, STEP_SCHED = 1, STEP_ONEPASS = 2, STEP_HIST = 3, STEP_HIST_SCHED = 4, STEP_HIST_ONEPASS = 5, STEP_CLIP = 6,
                kStepKinds = 12 };
struct StepGraphs {
    GraphExec exec[kStepKinds][1 + kStepRunGraphs];
    int rows = -1, chunks = -1, chunk_rows = -1;    // chunk_rows: the renorm kernels capture the segment size as an argument
    void reset() {
        for (auto& k : exec)
            for (auto& g : k) g.reset();
        rows = chunks = chunk_rows = -1;
    }
};

// Ownership: every device buffer, stream, event and graph executable the handle creates is a member of an owning type (dsg_own.hpp)
// and is released by `delete h`.  Members are destroyed in reverse order of declaration, and the order below is the one that needs:
// the pinned word, the events and the streams come first (destroyed last, after everything enqueued on them is gone), then the
// buffers -- the forward workspace `fw` before the training workspace `tr`, whose descriptor tables point into `fw` -- and the graph
// executables last (destroyed first: their nodes hold buffer addresses and were captured on cap_stream).
// Raw pointers are NOT owned: range_flag, renorm_stats, bound_ptrs, Param::ptr and the *_key cache keys.
struct dsg_handle {
    PinnedBuf<int> range_pinned;    // pinned host word dsg_range_status_stream reads the flag through
    Event tev[6];                   // dsg_train_profile_enable: the phase boundaries of dsg_train_step
    Event ev_fork, ev_join;
    Event ev_tail[3];               // the tail of dsg_train_step: chain done / time path done / column sums done
    Stream cap_stream;              // capture-only stream (the caller's may be the null stream)
    Stream side_stream;

    dsg_unet_desc d;
    int td = 0;  // time_dim = 4*proj
    std::vector<Param> params;
    long long total_params = 0;
    std::vector<ResP> res;
    std::vector<LinOpP> lin;
    std::vector<AttnP> attn;     // dsg_create_attn; empty for a net without attention: nothing below changes then
    std::vector<TensorInfo> tensors;
    std::vector<Op> ops;
    size_t per_tile_floats = 0;
    int tb_stride = 0;
    int temb_l1w, temb_l1b, temb_l2w, temb_l2b;

    // packed-weight arena
    DevBuf<float> arena;
    size_t arena_floats = 0;
    DevBuf<TimeBlockDesc> tdesc_dev;
    DevBuf<PackDesc> pack_dev;
    int pack_n = 0;
    long long pack_blocks = 0;
    std::vector<const float*> bound_ptrs;   // the caller's tensors (not owned)
    bool bound = false;

    // dsg_generation: moves whenever something a captured training step (train.StepGraph) may hold stops being valid -- a workspace is
    // freed (free_workspace, free_train_workspace), the launch plan changes (precision mode, launch policy, an option that takes another
    // value), or the per-batch-size tables of the training step are rewritten for another batch (build_train_descs, the narrow run's
    // training table), or the train law or the train report is set, replaced or removed (dsg_set_train_law, dsg_set_train_report: the
    // captured launches hold the kernel forms chosen under them and their buffers).  Host only; never reset.
    unsigned long long generation = 0;

    // fp16-split path (dsg_split.hpp): wide blocks of the sampling loop
    bool use_split = true;
    // launch policy (dsg_set_launch_policy): launches of at most this many row tiles take the small-launch kernel forms
    int coop_max_tiles = kCoopMaxTilesDefault;          // wide blocks: k_resblock_c (N/32 waves per tile) and no pair kernels
    int narrow_small_max_tiles = kNarrowSmallMaxTilesDefault; // narrow run: k_fused_narrow_h<true> (first-step planes requested a stage ahead)
    // 128-wide blocks of the reverse loop: launches of at least this many tiles run the persistent panel kernels (dsg_panel.hpp:
    // one 8-wave workgroup per CU); coop_max_tiles == 0 ("every launch takes its large-launch form") lowers it to 0
    int panel_min_tiles = kPanelMinTilesDefault;
    int num_cus = 256;
    DevBuf<float> maxabs;              // [params]: max|W| per tensor, refreshed at every bind
    DevBuf<const float*> mx_ptrs_dev; DevBuf<long long> mx_numel_dev; DevBuf<int> mx_idx_dev; int mx_n = 0;
    std::vector<int> mx_param;         // param index of each k_maxabs block
    DevBuf<PackHDesc> packh_dev; int packh_n = 0; long long packh_blocks = 0;
    DevBuf<OpConstDesc> opc_desc_dev; DevBuf<float> opc_dev;   // [res | lin][4]: un-scale factors, refreshed at every bind (k_pack_h)
    // the weight-side envelope of the split path (dsg_split.hpp, EnvDesc): one entry per LayerNorm and per split-packed Linear, checked
    // by k_pack_h at every bind; the word it raises is the spare last word of `maxabs` (cleared with the others by k_pack_grouped)
    DevBuf<EnvDesc> env_dev; int env_n = 0;
    float* env_word() const { return maxabs.get() + params.size(); }

    // forward workspace (ensure_workspace: sized for cap_rows rows and cap_entries schedule entries)
    int cap_rows = 0, cap_entries = 0;
    struct FwdWorkspace {
        DevBuf<float> ws;           // activations
        DevBuf<float> condfrag;
        DevBuf<float> cembed;       // [tiles_per_pass cap][ce_per_tile]: Wc silu(cond) of every block (sampling)
        DevBuf<float> ce_stats;     // scratch statistics sink of the precompute launches
        DevBuf<float> tb;           // [entries][tb_stride]
        DevBuf<float> st;           // [entries][td]
        DevBuf<float> h1s;          // [entries][td] Swish(lin1) of the time MLP
        DevBuf<float> tvals;        // [entries]
        DevBuf<int> ts_ident;       // [rows] identity index
        DevBuf<float> eps;          // [2][rows][D]
        DevBuf<float> ywork;        // [rows][D]
        DevBuf<float> hist;         // [rows][D]: the history term of a two-step plan (dsg_set_step_history); allocated by the first call under one
    } fw;
    size_t ce_per_tile = 0;
    size_t zero_off = 0;        // 128 zero floats in the arena
    DevBuf<float> freq;         // [proj/2]
    DevBuf<double> red;         // [2][kRedBlocks]
    DevBuf<int> step_dev;
    // dsg_set_step_grid: the time value of every step index of a sampling call and the number of early renormalised steps; grid_n == 0: no
    // grid (t = i / T, min(T, 4) renorm steps).  The buffer only grows and is kept when the grid is removed.
    DevBuf<float> grid_dev; int grid_n = 0, grid_cap = 0, grid_renorm = 0;
    // dsg_set_step_guidance: one weight per step index of a sampling call; guid_n == 0: none held.  The buffer only grows and is kept when
    // the setting is removed.  The host copy chooses the launch sequence (a zero weight: a one-pass step).  The step graphs of the scheduled
    // kinds hold `guid_call` alone (one pointer, allocated once), never the buffer: k_set_guidance writes its address per call.
    DevBuf<float> guid_dev; int guid_n = 0, guid_cap = 0;
    std::vector<float> guid_host;
    DevBuf<const float*> guid_call;
    // dsg_set_step_history: one row {m, p, q} per step index of a sampling call; hist_n == 0: none held.  The buffer only
    // grows and is kept when the setting is removed.  The step graphs of the history kinds hold `hist_call` (one pointer, allocated once)
    // and the workspace tensor fw.hist, never this buffer: k_set_guidance writes its address into `hist_call` per call.
    DevBuf<float> hist_dev; int hist_n = 0, hist_cap = 0;
    DevBuf<const float*> hist_call;
    // dsg_set_xstart_clip: the bounds lo / hi [D] of the predicted solution and one row {s, ia, a, is} per step index of a sampling call
    // (DESIGN.md 20); clip_n == 0: none held.  The buffers are kept when the setting is removed and replaced whole by the next set.  The
    // step graphs of the clip kinds hold `clip_call` (one block, allocated once), never these buffers: k_set_clip writes their addresses per call.
    DevBuf<float> clip_bounds, clip_rows; int clip_n = 0;
    DevBuf<ClipParams> clip_call;
    double* renorm_stats = nullptr;              // dsg_set_renorm_hook: caller's 3 doubles (device, not owned), reduced across ranks by `renorm_fn`
    void (*renorm_fn)(void*) = nullptr; void* renorm_user = nullptr;
    int device = 0;              // the device that was current in dsg_create: the settings / status entry points select it themselves
    int* range_flag = nullptr;   // device word: a raw split-path operand left fp16's range since the last dsg_range_status (an alias into step_dev)
    DevBuf<CallParams> call_dev;
    std::vector<double> op_ms;   // DSG_SAMPLE_PROFILE: summed HIP-event time per op
    bool train_prof = false;     // dsg_train_profile_enable: HIP events at the phase boundaries of dsg_train_step
    bool tev_valid = false;
    std::vector<int> op_calls;

    // fused narrow run [fuse_lo, fuse_hi) of `ops` (inference only)
    int fuse_lo = 0, fuse_hi = 0;
    // Everything prepare_fused builds for ONE inference context (rows, pass count, unconditional tiles, precision mode): the tables on the
    // device, their host sources and what they were built for.  Two sets are resident.  tabs[0] serves every entry point as before.
    // tabs[1] is the one-pass context of a sampling call whose guidance schedule has a zero (dsg_set_step_guidance): the
    // captured step graphs of either context hold the addresses of their own set, so a call that alternates uploads nothing.  A context
    // names its set (RunCtx::set); prepare_fused and the launch code read no other.
    struct FusedSig { bool valid = false, sp = false, share = false; int nrows = 0, npass = 0, uncond_tiles = 0; const void* p[8] = {}; };
    struct InferTables {
        DevBuf<FusedOp> fused_dev;
        std::vector<FusedOp> fused_host;
        DevBuf<FusedOpH> fusedh_dev;
        std::vector<FusedOpH> fusedh_host;
        // operator table of the WHOLE net for k_unet_tile (dsg_tile.hpp: one launch per pass for small batches), rebuilt with the fused
        // narrow run's table; tile_valid: the net has the shapes the kernel covers
        DevBuf<FusedOpH> tileops_dev;
        std::vector<FusedOpH> tileops_host;
        bool tile_valid = false;
        // what the device copy was built for (dsg_sample / dsg_unet_forward / dsg_time_op share set 0)
        FusedSig fused_sig;
        // LDS-resident form of the narrow run (k_fused_narrow_lds): per-operator LDS offsets, the copy list of every phase, the phases
        DevBuf<NarrowLdsOp> nlds_ops_dev; DevBuf<NarrowLdsCopy> nlds_copies_dev; DevBuf<uint4> nlds_image;
        std::vector<NarrowPhaseArgs> nlds_phases;
        bool nlds_tail = false;            // the LDS form of the run also computes the 64-wide Linear at ops[fuse_hi] (kind 2)
        bool nlds_valid = false;
        int nlds_ncopies = 0;              // entries of nlds_copies_dev: dsg_bind_weights re-gathers the image from the re-packed arena
        size_t nlds_image_cap = 0;         // uint4 capacity of nlds_image (grow-only: captured graphs hold the pointer)
    } tabs[2];
    bool opt_tile = true;             // dsg_set_option(DSG_OPT_TILE_STEP)
    bool opt_panel_half = true;       // dsg_set_option(DSG_OPT_PANEL_HALF): the 128-wide panel kernels with 16 KiB panels, two workgroups per CU
    bool opt_cfg_share = true;        // dsg_set_option(DSG_OPT_CFG_SHARE): down.0 of a two-pass step runs lin1 / lin2 once per row tile (k_panel128_duo_h)
    DevBuf<FusedOpH> fusedh_train_dev;      // the same run for the training forward (every output stored, h1/h2 saved)
    const void* fusedh_train_key[4] = {nullptr, nullptr, nullptr, nullptr}; int fusedh_train_rows = 0;
    DevBuf<FusedOp> ce_dev;             // condition-embedding Linear table (narrow blocks, one launch)
    std::vector<FusedOp> ce_host;
    DevBuf<CondTile> ctile_dev; int ctile_n = 0; const float* ctile_key = nullptr; size_t ctile_cap = 0;
    // the 8-wide bottom of the net as ops [v8_lo, v8_hi) (Downsample 16 -> 8 ... Upsample 8 -> 16), or -1: computed on the vector unit
    // in float32 by the LDS form of the narrow run (dsg_narrow8.hpp); opt_v8: dsg_set_option(DSG_OPT_NARROW_VALU8)
    int v8_lo = -1, v8_hi = -1;
    bool opt_v8 = true;
    bool opt_f32_pair = true;          // exact path: block + consuming Linear in one launch (k_resblock_lin); DSG_OPT_F32_PAIR
    bool opt_time_beside = true;       // dsg_set_option(DSG_OPT_TRAIN_TIME_BESIDE): see the tail of dsg_train_step
    bool opt_wg_narrow_part = false;   // dsg_set_option(DSG_OPT_WGRAD_NARROW_PART); read when the descriptor tables are (re)built
    // the section's image in global memory (V8SecL layout: raw nn.Linear matrices and parameter vectors), gathered at every bind; the LDS
    // form of the narrow run stages it as one piece, small launches and the training forward read it from L1 / L2
    DevBuf<float> v8_image; DevBuf<NarrowLdsCopy> v8_copies_dev; int v8_ncopies = 0;

    // chunked calls (dsg_sample_chunked): per-chunk Philox seeds and per-chunk renorm partials
    DevBuf<unsigned long long> seeds_dev; int seeds_cap = 0;
    DevBuf<double> red_chunks; int red_chunks_cap = 0;
    // dsg_set_chunk_variants: per-chunk omega / renorm count / table index of a chunked call; var_chunks == 0: none held.  The buffers only grow
    // and are kept when the setting is removed.  The step graphs of the variant form hold `var_call` alone (one block, allocated once), never
    // these buffers: k_set_var writes their addresses into it per call.
    DevBuf<float> var_omega; DevBuf<int> var_renorm, var_table; int var_cap = 0;
    int var_chunks = 0, var_tables = 1; bool var_has_renorm = false, var_has_table = false;
    std::vector<int> var_renorm_host;            // the counts, for the checks a call makes before it enqueues anything
    DevBuf<VarParams> var_call;

    // dsg_set_train_law: the integer CDF and the loss weight per timestep of the training steps; law_T == 0: none held.  The buffers only
    // grow and are kept when the law is removed.  A captured training step holds their addresses and the kernel forms chosen under the
    // law, so setting, changing or removing it moves `generation`.
    DevBuf<unsigned> law_cdf; DevBuf<float> law_w; int law_T = 0, law_cap = 0; bool law_has_cdf = false, law_has_w = false;
    // dsg_set_train_report: the caller's per-timestep accumulators (device, NOT owned); rep_T == 0: none held.  Moves `generation` too.
    double* rep_sq = nullptr; long long* rep_rows = nullptr; int rep_T = 0;

    // training workspace
    size_t tr_per_tile = 0;      // floats per tile
    size_t tr_yt_frag = 0, tr_deps = 0;
    int tr_rows = 0, tr_T = 0, tr_chunks = 0;
    struct TrainWorkspace {      // ensure_train_workspace / build_train_descs: sized for tr_rows rows and tr_T schedule entries
        DevBuf<float> ws;
        DevBuf<float> slabs;         // [chunks][slab_stride]
        DevBuf<float> gsum;          // [slab_stride]
        DevBuf<unsigned> gmax;       // max|G| per gradient tensor (float bits)
        DevBuf<unsigned> gmax_t;     // [kMaxGmax][gmax_ld] per-tile words, zeroed every step
        DevBuf<float> cs;            // per block: [tiles][cs_stride of the block] column sums
        DevBuf<int4> cs_map_dev;     // [cs_slots] (slab destination, second destination, region base + slot, row stride)
        DevBuf<int> ts;              // [rows]
        DevBuf<float> noise, mask;   // [rows][D], [rows]: device-side draws (dsg_train_step_seeded), allocated on first use
        DevBuf<float> yt_rm;         // [rows][D]
        DevBuf<float> tsave;         // emb | h1pre | h1s | tpre | d_st | d_h1s
        DevBuf<WgradDesc> wg_desc_dev; DevBuf<WgradUnit> wg_unit_dev;
        DevBuf<ColsumDesc> cs_desc_dev; DevBuf<ColsumUnit> cs_unit_dev;
    } tr;
    int gmax_ld = 0;
    int cs_slots = 0;
    int n_gmax = 0;
    size_t slab_stride = 0;
    DevBuf<long long> tw_dst_dev; DevBuf<const float*> tw_src_dev; int tw_rows = 0;  // time_emb.weight rows of all blocks
    int wg_units = 0;
    // early parts of the weight-gradient launch: after the backward kernel of residual block number wg_forks[k] (counted from the
    // LAST block, the first one the backward reaches) the weight gradients of the blocks since the previous fork run on
    // side_stream beside the rest of the activation-gradient chain, see dsg_train_step
    std::vector<int> wg_forks = {3, 6};
    std::vector<int> wg_part_end;      // units [wg_part_end[k-1], wg_part_end[k]) = part k; the rest runs on the caller's stream
    DevBuf<long long> r2_dev; int r2_n = 0; long long r2_total = 0;   // [starts | prefix]: the parameter ranges the last reduce covers
    bool r2_vec4 = false;              // ... in float4 units (k_reduce_ranges4)
    int wg_onehot_end = 0;             // ... and opens with the final part's time-table units: [wg_part_end.back(), wg_onehot_end),
    int wg_blocks_end = 0;             // then its residual blocks' other units [wg_onehot_end, wg_blocks_end), then the plain Linears'
    std::vector<int> wg_fork_ops;      // operator index after whose backward kernel part k starts
    int wg_early_lds = 40960;
    DevBuf<FusedBwdOpH> fbwd_dev; int fbwd_n = 0;   // operator table of the fused narrow backward (split path), cached with the descriptors
    int cs_units = 0;
    // the descriptor tables depend only on (rows, T, precision mode) and the workspace addresses: built once, reused every step
    bool td_valid = false; int td_B = 0, td_T = 0, td_rows = 0; bool td_split = false; const void* td_key[6] = {};

    // cached step graphs: per-step pair (with / without the renorm kernels), keyed by (rows, chunks); and ONE graph of a whole
    // T-step loop for short schedules, keyed by (rows, chunks, T)
    // `graphs`: the plain form of the step.  `graphs_var`: the same set for calls with chunk variants (k_update_var, k_renorm_apply_var),
    // cached BESIDE the plain one under its own key: plain and variants calls alternating on one handle replay their own graphs
    StepGraphs graphs, graphs_var;
};

namespace {

int add_param(dsg_handle* h, const std::string& name, long long numel) {
    Param p;
    p.name = name; p.numel = numel; p.off = h->total_params;
    h->total_params += numel;
    h->params.push_back(p);
    return (int)h->params.size() - 1;
}
LinearP add_linear(dsg_handle* h, const std::string& prefix, int K, int N) {
    LinearP l;
    l.N = N; l.K = K;
    l.w = add_param(h, prefix + ".weight", (long long)N * K);
    l.b = add_param(h, prefix + ".bias", N);
    return l;
}
NormP add_norm(dsg_handle* h, const std::string& prefix, int n) {
    NormP p;
    p.w = add_param(h, prefix + ".weight", n);
    p.b = add_param(h, prefix + ".bias", n);
    return p;
}
int add_res(dsg_handle* h, const std::string& prefix, int in0, int in1, int N) {
    ResP r;
    const int in = in0 + in1;
    r.in0 = in0; r.in1 = in1; r.N = N;
    r.n1 = add_norm(h, prefix + ".norm1", in);
    r.l1 = add_linear(h, prefix + ".lin1", in, N);
    r.n2 = add_norm(h, prefix + ".norm2", N);
    r.l2 = add_linear(h, prefix + ".lin2", N, N);
    r.n3 = add_norm(h, prefix + ".norm3", N);
    r.l3 = add_linear(h, prefix + ".lin3", N, N);
    r.sclin = in != N;
    if (r.sclin) r.sc = add_linear(h, prefix + ".shortcut", in, N);
    r.te = add_linear(h, prefix + ".time_emb", h->td, N);
    r.ce = add_linear(h, prefix + ".cond_emb", h->d.cond_dim, N);
    r.tb_off = h->tb_stride;
    h->tb_stride += pad32(N);
    h->res.push_back(r);
    return (int)h->res.size() - 1;
}
int add_attn(dsg_handle* h, const std::string& prefix, int N) {
    AttnP a;
    a.N = N;
    a.norm = add_norm(h, prefix + ".norm", N);
    a.proj = add_linear(h, prefix + ".projection", N, 3 * N);
    a.out = add_linear(h, prefix + ".output", N, N);
    h->attn.push_back(a);
    return (int)h->attn.size() - 1;
}
int add_tensor(dsg_handle* h, int width, bool is_skip) {
    TensorInfo t;
    t.width = width;
    t.is_skip = is_skip;
    t.data_off = h->per_tile_floats;
    h->per_tile_floats += (size_t)groups_of(width) * 256;
    t.stats_off = h->per_tile_floats;
    h->per_tile_floats += 64;
    t.ga = t.gb = 0;
    h->tensors.push_back(t);
    return (int)h->tensors.size() - 1;
}

bool width_supported(int n) { return n == 4 || n == 8 || n == 16 || n == 32 || n == 64 || n == 128; }

struct Carver {
    size_t off = 0;
    size_t take(size_t floats) { size_t o = off; off += (floats + 63) / 64 * 64; return o; }
};

void carve(dsg_handle* h) {
    Carver c;
    const int CG = groups_of(h->d.cond_dim);
    for (auto& r : h->res) {
        const int NT = cdiv(r.N, 32), NG = groups_of(r.N), KG = groups_of(r.in0) + groups_of(r.in1), OT1 = cdiv(KG, 4);
        r.W1p = c.take((size_t)NT * KG * 256);
        r.g1p = c.take((size_t)KG * 8 + 32);
        r.b1p = c.take((size_t)KG * 8 + 32);
        r.W2p = c.take((size_t)NT * NG * 256);
        r.g2p = c.take(NT * 32); r.b2p = c.take(NT * 32); r.c2p = c.take(NT * 32);
        r.Wcp = c.take((size_t)NT * CG * 256);
        r.W3p = c.take((size_t)NT * NG * 256);
        r.g3p = c.take(NT * 32); r.b3p = c.take(NT * 32); r.c3p = c.take(NT * 32);
        r.Wscp = r.sclin ? c.take((size_t)NT * KG * 256) : 0;
        r.W1T = c.take((size_t)OT1 * NG * 256);
        r.W2T = c.take((size_t)NT * NG * 256);
        r.W3T = c.take((size_t)NT * NG * 256);
        r.WscT = r.sclin ? c.take((size_t)OT1 * NG * 256) : 0;
        r.split = true;
        if (r.split) {
            const size_t KS1 = (size_t)(groups_of(r.in0) + 1) / 2 + (size_t)(groups_of(r.in1) + 1) / 2;
            r.W1h = c.take((size_t)NT * KS1 * 128 * 4);
            r.W2h = c.take((size_t)NT * ((NG + 1) / 2) * 128 * 4);
            r.W3h = c.take((size_t)NT * ((NG + 1) / 2) * 128 * 4);
            r.Wsch = r.sclin ? c.take((size_t)NT * KS1 * 128 * 4) : 0;
            const size_t KSn = (size_t)(NG + 1) / 2;
            r.W1Th = c.take((size_t)OT1 * KSn * 128 * 4);
            r.W2Th = c.take((size_t)NT * KSn * 128 * 4);
            r.W3Th = c.take((size_t)NT * KSn * 128 * 4);
            r.WscTh = r.sclin ? c.take((size_t)OT1 * KSn * 128 * 4) : 0;
        }
    }
    for (auto& l : h->lin) {
        const int NT = cdiv(l.l.N, 32), KG = groups_of(l.l.K);
        l.Wp = c.take((size_t)NT * KG * 256);
        l.bp = c.take(NT * 32);
        l.gp = l.lnact ? c.take((size_t)KG * 8 + 32) : 0;
        l.betap = l.lnact ? c.take((size_t)KG * 8 + 32) : 0;
        l.WT = c.take((size_t)cdiv(KG, 4) * groups_of(l.l.N) * 256);
        l.Wh = c.take((size_t)NT * ((KG + 1) / 2) * 128 * 4);
    }
    {   // condition-embedding planes of every block, consecutive: one grouped launch walks them (k_cond_embed_h)
        const size_t KSc = (size_t)(CG + 1) / 2;
        for (auto& r : h->res) r.Wch = c.take((size_t)cdiv(r.N, 32) * KSc * 128 * 4);
    }
    for (auto& a : h->attn) {   // behind everything else: the arena of a net without attention is laid out as before
        const int NT = cdiv(a.N, 32), NG = groups_of(a.N);
        a.Wvp = c.take((size_t)NT * NG * 256); a.bvp = c.take(NT * 32);
        a.Wop = c.take((size_t)NT * NG * 256); a.bop = c.take(NT * 32);
        a.WvT = c.take((size_t)NT * NG * 256); a.WoT = c.take((size_t)NT * NG * 256);
        if (a.N >= 64) { a.Wvh = c.take((size_t)NT * ((NG + 1) / 2) * 128 * 4); a.Woh = c.take((size_t)NT * ((NG + 1) / 2) * 128 * 4); }
    }
    h->zero_off = c.take(128);
    h->arena_floats = c.off;
    for (auto& r : h->res) { r.ce_off = h->ce_per_tile; h->ce_per_tile += (size_t)groups_of(r.N) * 256; }
    // training workspace layout (per-tile float offsets)
    size_t o = 0;
    auto take = [&](size_t f) { size_t r = o; o += f; return r; };
    for (auto& t : h->tensors) {
        t.ga = take((size_t)groups_of(t.width) * 256);
        t.gb = t.is_skip ? take((size_t)groups_of(t.width) * 256) : 0;
    }
    for (auto& r : h->res) {
        const size_t NGf = (size_t)groups_of(r.N) * 256, KGf = (size_t)(groups_of(r.in0) + groups_of(r.in1)) * 256;
        r.h1 = take(NGf); r.h2 = take(NGf); r.du1 = take(KGf);
        r.dh1 = take(NGf); r.dh2 = take(NGf); r.rs1 = take(64); r.rs2 = take(64); r.rs3 = take(64);
    }
    for (auto& l : h->lin)
        if (l.lnact) { l.du = take((size_t)groups_of(l.l.K) * 256); l.rs = take(64); }
    for (auto& a : h->attn) { a.v = take((size_t)groups_of(a.N) * 256); a.dv = take((size_t)groups_of(a.N) * 256); }
    h->tr_yt_frag = take((size_t)groups_of(h->d.input_dim) * 256);
    h->tr_deps = take((size_t)groups_of(h->d.input_dim) * 256);
    h->tr_per_tile = o;
}

void free_graphs(dsg_handle* h) {
    h->graphs.reset();
    h->graphs_var.reset();
}

constexpr int kMaxGmax = 256;   // distinct gradient tensors whose max|G| is tracked (3 per block + 1 per Linear)

void free_train_workspace(dsg_handle* h) {
    ++h->generation;          // a captured training step holds these buffers
    h->tr = {};
    h->wg_units = h->cs_units = 0;
    h->tr_rows = h->tr_T = 0;
    h->td_valid = false;
}

void free_workspace(dsg_handle* h) {
    ++h->generation;
    for (auto& t : h->tabs) t.fused_sig.valid = false;
    free_graphs(h);
    free_train_workspace(h);  // its descriptors point into the forward workspace
    h->fw = {};
    h->cap_rows = h->cap_entries = 0;
}

__global__ void k_iota(int* p, int n) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = i;
}
__global__ void k_linspace_t(float* p, int T) {  // t = i / T in float32, as `torch.full(..., i) / T` (MSR.py:126)
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < T; i += gridDim.x * blockDim.x) p[i] = (float)i / (float)T;
}

__global__ void k_grid_t(float* p, const float* __restrict__ grid, int n) {  // dsg_set_step_grid: the handle's own time values
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = grid[i];
}

int ensure_workspace(dsg_handle* h, int rows, int entries) {
    if (rows <= h->cap_rows && entries <= h->cap_entries) return 0;
    const int nrows = rows > h->cap_rows ? rows : h->cap_rows;
    // the per-entry tables are a few MB: size them for 1024 schedule entries at once (T = 1000 is the longest shipped schedule), so
    // that a longer call after a short one -- a K-step run after a W-step warm-up -- does not free and re-create the multi-GB row
    // workspace and the captured graphs in the middle of a timed region
    int nent = entries > h->cap_entries ? entries : h->cap_entries;
    if (nent < 1024) nent = 1024;
    HIPCK(hipDeviceSynchronize());
    free_workspace(h);
    const size_t tiles = (size_t)cdiv(nrows, 32) * 2;  // two passes
    const int D = h->d.input_dim, CG = groups_of(h->d.cond_dim);
    HIPCK(h->fw.ws.alloc(tiles * h->per_tile_floats));
    HIPCK(hipMemset(h->fw.ws, 0, tiles * h->per_tile_floats * sizeof(float)));
    HIPCK(h->fw.condfrag.alloc((tiles / 2) * CG * 256));
    HIPCK(h->fw.cembed.alloc((tiles / 2) * h->ce_per_tile));
    HIPCK(h->fw.ce_stats.alloc((tiles / 2) * 64));
    HIPCK(h->fw.tb.alloc((size_t)nent * h->tb_stride));
    HIPCK(h->fw.st.alloc((size_t)nent * h->td));
    HIPCK(h->fw.h1s.alloc((size_t)nent * h->td));
    HIPCK(h->fw.tvals.alloc((size_t)nent));
    HIPCK(h->fw.ts_ident.alloc((size_t)nrows));
    HIPCK(h->fw.eps.alloc((size_t)2 * nrows * D));
    HIPCK(h->fw.ywork.alloc((size_t)nrows * D));
    hipLaunchKernelGGL(k_iota, dim3(cdiv(nrows, 256)), dim3(256), 0, 0, h->fw.ts_ident, nrows);
    HIPCK(hipDeviceSynchronize());
    h->cap_rows = nrows;
    h->cap_entries = nent;
    return 0;
}

bool fusable(const dsg_handle* h, const Op& op) {
    if (op.kind == OP_RES) return h->res[op.p].N <= 32;
    if (op.kind == OP_LIN) return h->lin[op.p].l.N <= 32;
    return false;
}


int check_bound(const dsg_handle* h) {
    if (!h) return fail("null handle");
    if (!h->bound) return fail("dsg_bind_weights has not been called");
    return 0;
}


// what dsg_create refuses before it builds anything; 0: the descriptor is one the kernels cover
int check_unet_desc(const dsg_unet_desc* desc, const int* is_attn, int middle_attn) {
    if (!desc) return fail("null desc");
    const dsg_unet_desc d = *desc;
    if (d.n_res < 1 || d.n_res > 8 || d.n_blocks < 1 || d.input_dim < 1 || d.cond_dim < 1) return fail("bad UNet1D descriptor");
    if (d.input_dim > 128) return fail("input_dim %d is not supported (at most 128)", d.input_dim);
    if (d.cond_dim > 4096) return fail("cond_dim %d is not supported (at most 4096)", d.cond_dim);
    if (!width_supported(d.proj_dim) || d.proj_dim < 8)
        return fail("proj_dim %d unsupported (supported block widths: 4 (dims only), 8, 16, 32, 64, 128)", d.proj_dim);
    for (int i = 0; i < d.n_res; ++i)
        if (!width_supported(d.dims[i])) return fail("dims[%d]=%d unsupported (4, 8, 16, 32, 64, 128)", i, d.dims[i]);
    auto attn_at = [&](int i) { return is_attn && is_attn[i] != 0; };     // (as create_impl reads it)
    {
        std::vector<int> aw;      // every width an AttentionBlock is asked for
        for (int i = 0; i < d.n_res; ++i) {
            if (!attn_at(i)) continue;
            aw.push_back(i > 0 ? d.dims[i - 1] : d.proj_dim);      // down blocks of resolution i
            aw.push_back(d.dims[i]);                               // up blocks of resolution i (and the extra down blocks of the last one)
            if (i == 0) aw.push_back(d.proj_dim);                  // the extra up blocks
        }
        if (middle_attn) aw.push_back(d.dims[d.n_res - 1]);
        for (int w4 : aw)
            if (w4 < 8 || !width_supported(w4)) return fail("AttentionBlock width %d unsupported (8, 16, 32, 64, 128)", w4);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("no HIP device: libdiffsg_hip needs an MI355X");
    return 0;
}

// the fused narrow run = the longest consecutive run of narrow operators, and the float32 section inside it
void plan_fused_run(dsg_handle* h) {
    const dsg_unet_desc& d = h->d;
    int best_lo = 0, best_hi = 0, lo = -1;
    for (int i = 0; i <= (int)h->ops.size(); ++i) {
        const bool f = i < (int)h->ops.size() && fusable(h, h->ops[i]);
        if (f && lo < 0) lo = i;
        if (!f && lo >= 0) { if (i - lo > best_hi - best_lo) { best_lo = lo; best_hi = i; } lo = -1; }
    }
    h->fuse_lo = best_lo; h->fuse_hi = best_hi;
    // the float32 section must be the shape dsg_narrow8.hpp is written for and lie inside the fused run
    if (h->v8_lo < 0 || h->v8_hi != h->v8_lo + 2 * d.n_blocks + 5 || h->v8_lo < h->fuse_lo || h->v8_hi > h->fuse_hi) h->v8_lo = h->v8_hi = -1;
    for (int i = h->v8_lo + 1; h->v8_lo >= 0 && i + 1 < h->v8_hi; ++i) {
        const Op& o = h->ops[i];
        const bool up = i - h->v8_lo > d.n_blocks + 2;
        if (o.kind != OP_RES || h->res[o.p].N != 8 || h->res[o.p].in0 != 8 || h->res[o.p].in1 != (up ? 8 : 0) || o.in0 != h->ops[i - 1].out ||
            h->res[o.p].tb_off != h->res[h->ops[h->v8_lo + 1].p].tb_off + 32 * (i - h->v8_lo - 1) || o.p != h->ops[h->v8_lo + 1].p + (i - h->v8_lo - 1) ||
            (up && o.in1 != h->ops[h->v8_lo + d.n_blocks - (i - h->v8_lo - d.n_blocks - 3)].out))
            h->v8_lo = h->v8_hi = -1;
    }
}

// the device side of a fresh handle: the arena and the per-handle tables and words; false: an allocation or a copy failed
bool create_device_state(dsg_handle* h) {
    const dsg_unet_desc& d = h->d;
    {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0)
            h->num_cus = cus;
    }
    bool ok = h->ce_dev.alloc(h->res.size() + 1) == hipSuccess &&
              h->tabs[0].fusedh_dev.alloc(h->ops.size() + 1) == hipSuccess &&
              h->tabs[0].tileops_dev.alloc(h->ops.size() + 1) == hipSuccess &&
              h->maxabs.alloc(h->params.size() + 1) == hipSuccess &&
              h->tabs[0].fused_dev.alloc(2 * (h->ops.size() + 1)) == hipSuccess &&
              h->arena.alloc(h->arena_floats) == hipSuccess &&
              hipMemset(h->arena, 0, h->arena_floats * sizeof(float)) == hipSuccess &&
              h->tdesc_dev.alloc(h->res.size()) == hipSuccess &&
              h->freq.alloc(d.proj_dim / 2) == hipSuccess &&
              h->red.alloc(2 * kRedBlocks) == hipSuccess &&
              h->step_dev.alloc(32) == hipSuccess &&
              hipMemset(h->step_dev, 0, 128) == hipSuccess &&
              h->call_dev.alloc(1) == hipSuccess &&
              hipStreamCreateWithFlags(h->cap_stream.put(), hipStreamNonBlocking) == hipSuccess;
    if (ok) h->range_flag = h->step_dev + 16;      // its own 64-byte line of the same small allocation
    if (ok) {
        std::vector<OpConstDesc> oc;
        for (const ResP& r : h->res) oc.push_back(OpConstDesc{r.l1.w, r.l2.w, r.l3.w, r.sclin ? r.sc.w : -1});
        for (const LinOpP& l : h->lin) oc.push_back(OpConstDesc{l.l.w, -1, -1, -1});
        ok = h->opc_desc_dev.alloc(oc.size()) == hipSuccess &&
             h->opc_dev.alloc(oc.size() * 4) == hipSuccess &&
             hipMemcpy(h->opc_desc_dev, oc.data(), oc.size() * sizeof(OpConstDesc), hipMemcpyHostToDevice) == hipSuccess;
    }
    if (ok) {
        // freq[k] = exp(k * -(ln 1e4 / (half-1))) in float32 (UNetCF.py:37-38)
        const int half = d.proj_dim / 2;
        std::vector<float> f(half);
        const float c = (float)(-(log(10000.0) / (half - 1)));
        for (int k = 0; k < half; ++k) f[k] = expf((float)k * c);
        ok = hipMemcpy(h->freq, f.data(), half * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
    }
    return ok;
}

dsg_handle* create_impl(const dsg_unet_desc* desc, const int* is_attn, int middle_attn) {
    if (check_unet_desc(desc, is_attn, middle_attn)) return nullptr;
    const dsg_unet_desc d = *desc;
    // is_attn[i] of the blocks of resolution i; the extra blocks at the last width (down path) and at proj_dim (up path) use the
    // loop's final i, as the reference constructor does (UNetCF.py:289,310)
    auto attn_at = [&](int i) { return is_attn && is_attn[i] != 0; };
    dsg_handle* h = new dsg_handle();
    h->d = d;
    h->td = 4 * d.proj_dim;
    (void)hipGetDevice(&h->device);
    // ---- parameter table + plan, in the registration order of UNet1D.__init__ (UNetCF.py:272-316)
    LinOpP proj;
    proj.l = add_linear(h, "feature_proj", d.input_dim, d.proj_dim);
    h->lin.push_back(proj);
    {
        LinearP t1 = add_linear(h, "time_emb.lin1", d.proj_dim, h->td);
        LinearP t2 = add_linear(h, "time_emb.lin2", h->td, h->td);
        h->temb_l1w = t1.w; h->temb_l1b = t1.b; h->temb_l2w = t2.w; h->temb_l2b = t2.b;
    }
    std::vector<int> skips;
    int cur = add_tensor(h, d.proj_dim, true);
    h->ops.push_back(Op{OP_PROJ, 0, -1, -1, cur, "feature_proj"});
    skips.push_back(cur);
    int w = d.proj_dim, idx = 0;
    char nm[64];
    // res, then attn (UNetCF.py:177-178): the operator sits behind its residual block with an output tensor of its own; what the block
    // hands on -- and what the down path pushes as the skip -- is the attention output
    auto push_attn = [&](const char* prefix, int width, bool is_skip) {
        snprintf(nm, sizeof nm, "%s.attn", prefix);
        const int p = add_attn(h, nm, width);
        const int out = add_tensor(h, width, is_skip);
        h->ops.push_back(Op{OP_ATTN, p, cur, -1, out, nm});
        cur = out;
    };
    auto push_down_res = [&](int width, bool attn) {
        snprintf(nm, sizeof nm, "down.%d.res", idx);
        const int p = add_res(h, nm, width, 0, width);
        const int out = add_tensor(h, width, !attn);
        h->ops.push_back(Op{OP_RES, p, cur, -1, out, nm});
        cur = out;
        if (attn) { char pf[32]; snprintf(pf, sizeof pf, "down.%d", idx); push_attn(pf, width, true); }
        skips.push_back(cur); ++idx;
    };
    for (int i = 0; i < d.n_res; ++i) {
        for (int b = 0; b < d.n_blocks; ++b) push_down_res(w, attn_at(i));
        snprintf(nm, sizeof nm, "down.%d.lin", idx);
        LinOpP l; l.l = add_linear(h, nm, w, d.dims[i]);
        h->lin.push_back(l);
        const int out = add_tensor(h, d.dims[i], true);
        h->ops.push_back(Op{OP_LIN, (int)h->lin.size() - 1, cur, -1, out, nm});
        if (i == d.n_res - 1 && w == 16 && d.dims[i] == 8 && (d.n_blocks == 2 || d.n_blocks == 3)) h->v8_lo = (int)h->ops.size() - 1;
        cur = out; skips.push_back(cur); ++idx;
        w = d.dims[i];
        if (i == d.n_res - 1)
            for (int b = 0; b < d.n_blocks; ++b) push_down_res(w, attn_at(i));
    }
    for (int m = 1; m <= 2; ++m) {
        snprintf(nm, sizeof nm, "middle.res%d", m);
        const int p = add_res(h, nm, w, 0, w);
        const int out = add_tensor(h, w, false);
        h->ops.push_back(Op{OP_RES, p, cur, -1, out, nm});
        cur = out;
        if (m == 1 && middle_attn) push_attn("middle", w, false);
    }
    idx = 0;
    auto push_up_res = [&](int width, bool attn) {
        snprintf(nm, sizeof nm, "up.%d.res", idx);
        const int sk = skips.back(); skips.pop_back();
        const int p = add_res(h, nm, width, h->tensors[sk].width, width);
        const int out = add_tensor(h, width, false);
        h->ops.push_back(Op{OP_RES, p, cur, sk, out, nm});
        cur = out;
        if (attn) { char pf[32]; snprintf(pf, sizeof pf, "up.%d", idx); push_attn(pf, width, false); }
        ++idx;
    };
    for (int i = d.n_res - 1; i >= 0; --i) {
        for (int b = 0; b < d.n_blocks + 1; ++b) push_up_res(w, attn_at(i));
        const int nw = i > 0 ? d.dims[i - 1] : d.proj_dim;
        snprintf(nm, sizeof nm, "up.%d.lin", idx);
        LinOpP l; l.l = add_linear(h, nm, w, nw);
        h->lin.push_back(l);
        const int out = add_tensor(h, nw, false);
        h->ops.push_back(Op{OP_LIN, (int)h->lin.size() - 1, cur, -1, out, nm});
        if (i == d.n_res - 1 && h->v8_lo >= 0 && nw == 16) h->v8_hi = (int)h->ops.size();
        cur = out; ++idx;
        w = nw;
        if (i == 0)
            for (int b = 0; b < d.n_blocks + 1; ++b) push_up_res(w, attn_at(i));
    }
    {
        LinOpP f;
        f.ln = add_norm(h, "norm", w);
        f.l = add_linear(h, "final", w, d.input_dim);
        f.lnact = true;
        h->lin.push_back(f);
        h->ops.push_back(Op{OP_FINAL, (int)h->lin.size() - 1, cur, -1, -1, "final"});
    }
    for (const ResP& r : h->res)
        if ((r.in1 && r.in1 != r.in0) || (r.sclin != (r.in1 != 0))) { fail("internal: unexpected block shape"); delete h; return nullptr; }
    for (size_t i = 0; i < h->ops.size(); ++i) {     // an attention operator is the ONLY reader of its input (k_attn_bwd stores into its `ga`)
        if (h->ops[i].kind != OP_ATTN) continue;
        int readers = 0;
        for (const Op& o : h->ops) readers += (o.in0 == h->ops[i].in0) + (o.in1 == h->ops[i].in0);
        if (readers != 1 || h->tensors[h->ops[i].in0].is_skip) { fail("internal: attention input with another reader"); delete h; return nullptr; }
    }
    carve(h);
    plan_fused_run(h);
    if (!create_device_state(h)) { fail("device allocation failed in dsg_create"); delete h; return nullptr; }
    return h;
}

}  // namespace
