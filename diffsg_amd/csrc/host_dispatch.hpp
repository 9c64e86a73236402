// Part of the ONE translation unit dsg_api.hip (included from there, after the kernel headers and `using namespace dsg`): not a
// stand-alone header.  Argument fill and kernel dispatch: which kernel form runs an operator, a pair or the fused narrow run, and the walk over the operators.
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------------
// kernel dispatch
// ------------------------------------------------------------------------------------------------------
// One width dispatch: f(std::integral_constant<int, V>{}) for the V of the list that equals n; false (and no call) for any other n.
// Fully inlined: a chain of compares, as the switch ladders it replaces.  A lambda that must not instantiate a kernel for some V says so
// with `if constexpr` (the set of instantiated kernels is part of the library's contract: tools/resusage.py, kernel_resources()).
template <class F, int... Vs>
inline bool dispatch_ints(int n, F&& f, std::integer_sequence<int, Vs...>) {
    return ((n == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}
// the block widths (N) and the 32-feature tile counts (cdiv(N, 32)) the kernels are instantiated for
template <class F> inline bool dispatch_width(int N, F&& f) { return dispatch_ints(N, f, std::integer_sequence<int, 4, 8, 16, 32, 64, 128>{}); }
template <class F> inline bool dispatch_tiles(int nt, F&& f) { return dispatch_ints(nt, f, std::integer_sequence<int, 1, 2, 3, 4>{}); }
template <class F> inline void dispatch_bool(bool b, F&& f) { if (b) f(std::true_type{}); else f(std::false_type{}); }
#define DSG_V(x) decltype(x)::value
// An explicit list of the instantiated combinations of a kernel family (the list is information): the first entry whose condition
// holds launches and returns true.  Every family below is a one-line entry macro over this form.
#define DSG_TRY_LAUNCH(cond, launch) if (cond) { launch; return true; }

inline dim3 wave_grid(int ntiles) { return dim3(cdiv(ntiles, kWavesPerBlock)); }   // one wave per row tile, kWavesPerBlock waves per workgroup

void launch_res(int N, bool sclin, const BlockArgs& a, hipStream_t s) {
    const dim3 grid = wave_grid(a.ntiles), block(256);
    dispatch_width(N, [&](auto n) { dispatch_bool(sclin, [&](auto sc) {
        constexpr int W = DSG_V(n);
        // the unrolled-chain form when the input tensors have N / 8 groups each (every shipped net)
        if constexpr (W >= 64) {
            if (a.in0.groups == W / 8 && a.in1.groups == (sclin ? W / 8 : 0)) {
                hipLaunchKernelGGL((k_resblock<W, DSG_V(sc), true>), grid, block, 0, s, a);
                return;
            }
        }
        hipLaunchKernelGGL((k_resblock<W, DSG_V(sc)>), grid, block, 0, s, a);
    }); });
}
// the cooperative form needs the block's inputs exactly N wide (every 64- / 128-wide block of the shipped architectures)
bool bwd_coop_ok(int N, bool sclin, const BlockBwdArgsH& a) {
    if (N != 64 && N != 128) return false;
    if (a.b.in0.width != N) return false;
    return sclin ? (a.b.in1.width == N && a.WscTh != nullptr) : a.b.in1.groups == 0;
}
// `coop`: the cooperative form where the shapes allow it (faster at every batch size measured: 512 rows 72 -> 20 us per up-128 block,
// 32 768 rows 105 -> 65 us); the fused narrow backward's table keeps the one-wave-per-tile bodies
// Returns false for a shape no kernel is instantiated for: a 64- / 128-wide block whose inputs are not exactly N wide.  UNet1D builds
// none (DownBlock w -> w, UpBlock 2w -> w, UNetCF.py:278-311); the one-wave-per-tile form that covered them kept 72-108 bytes of scratch
// per lane at N = 128 and was never launched: removed rather than shipped unmeasured.
bool launch_res_bwd_h(int N, bool sclin, const BlockBwdArgsH& a, hipStream_t s, bool coop = false) {
    const dim3 block(256);
    if (N == 64 || N == 128) {
        if (!(coop && bwd_coop_ok(N, sclin, a))) return false;
        dispatch_bool(sclin, [&](auto sc) {
            if (N == 128) hipLaunchKernelGGL((k_resblock_bwd_c<128, DSG_V(sc)>), dim3(a.b.ntiles), block, 0, s, a);
            else hipLaunchKernelGGL((k_resblock_bwd_c<64, DSG_V(sc)>), dim3(cdiv(a.b.ntiles, 2)), block, 0, s, a);
        });
        return true;
    }
    return dispatch_width(N, [&](auto n) { dispatch_bool(sclin, [&](auto sc) {
        if constexpr (DSG_V(n) <= 32) hipLaunchKernelGGL((k_resblock_bwd_h<DSG_V(n), DSG_V(sc)>), wave_grid(a.b.ntiles), block, 0, s, a);
    }); });
}
void launch_res_bwd(int N, bool sclin, const BlockBwdArgs& a, hipStream_t s) {
    dispatch_width(N, [&](auto n) { dispatch_bool(sclin, [&](auto sc) {
        hipLaunchKernelGGL((k_resblock_bwd<DSG_V(n), DSG_V(sc)>), wave_grid(a.ntiles), dim3(256), 0, s, a);
    }); });
}
// the three instantiated forms of a Linear: row-major input (feature_proj), LayerNorm + SiLU with row-major output (final), fragments
#define DSG_LIN_FORMS(KERNEL, NT, ntiles, a)                                                                                     \
    do {                                                                                                                         \
        const dim3 grid = wave_grid(ntiles), block(256);                                                                         \
        if (inmode == IN_ROWMAJOR) hipLaunchKernelGGL((KERNEL<NT, IN_ROWMAJOR, OUT_FRAG, false>), grid, block, 0, s, a);         \
        else if (outmode == OUT_ROWMAJOR && lnact) hipLaunchKernelGGL((KERNEL<NT, IN_FRAG, OUT_ROWMAJOR, true>), grid, block, 0, s, a); \
        else hipLaunchKernelGGL((KERNEL<NT, IN_FRAG, OUT_FRAG, false>), grid, block, 0, s, a);                                  \
    } while (0)
void launch_lin(int N, int inmode, int outmode, bool lnact, const LinArgs& a, hipStream_t s) {
    dispatch_tiles(cdiv(N, 32), [&](auto nt) { DSG_LIN_FORMS(k_linear, DSG_V(nt), a.ntiles, a); });
}
void launch_lin_bwd(int K, bool lnbwd, const LinBwdArgs& a, hipStream_t s) {
    dispatch_tiles(cdiv(K, 32), [&](auto ot) { dispatch_bool(lnbwd, [&](auto ln) {
        hipLaunchKernelGGL((k_linear_bwd<DSG_V(ot), DSG_V(ln)>), wave_grid(a.ntiles), dim3(256), 0, s, a);
    }); });
}

struct RunCtx {
    int nrows;           // rows per pass
    int npass;           // 1 or 2
    int uncond_tiles;    // leading tiles without the condition term
    const float* y;      // row-major [nrows][D]
    float* eps_out;      // row-major [npass][nrows][D]
    const int* step_ptr; // or null
    const int* ts;       // or null
    bool train;          // save h1/h2 for the backward pass
    bool cond_pre;       // condition embeddings precomputed for this call (dsg_sample)
    int* advance_step = nullptr;   // reverse loop: feature_proj decrements the step index (LinArgs::advance_step)
    bool share_proj = false;       // reverse loop, split path: feature_proj(y) computed for ONE pass, read by both (Seg::wrap)
    int set = 0;                   // which resident table set (dsg_handle::tabs) the context's tables live in; 1: the one-pass context of a scheduled call
};

size_t cap_tiles_of(const dsg_handle* h) { return (size_t)cdiv(h->cap_rows, 32) * 2; }
size_t tr_tiles_of(const dsg_handle* h) { return (size_t)cdiv(h->tr_rows, 32); }

Seg seg_of(const dsg_handle* h, int tid) {
    const TensorInfo& t = h->tensors[tid];
    const size_t cap = cap_tiles_of(h);
    Seg s;
    s.data = h->fw.ws + t.data_off * cap;
    s.stats = h->fw.ws + t.stats_off * cap;
    s.groups = groups_of(t.width);
    s.width = t.width;
    s.wrap = 0;
    return s;
}
float* trp(const dsg_handle* h, size_t off) { return h->tr.ws + off * tr_tiles_of(h); }

void fill_block_args(const dsg_handle* h, const Op& op, const RunCtx& c, BlockArgs& a) {
    const int tpp = cdiv(c.nrows, 32);
    const ResP& r = h->res[op.p];
    const float* A = h->arena;
    memset(&a, 0, sizeof a);
    a.in0 = seg_of(h, op.in0);
    if (op.in1 >= 0) a.in1 = seg_of(h, op.in1);
    if (c.share_proj) {
        const int pt = h->ops[0].out;
        if (op.in0 == pt) a.in0.wrap = tpp;
        if (op.in1 == pt) a.in1.wrap = tpp;
    }
    a.W1 = A + r.W1p; a.gamma1 = A + r.g1p; a.beta1 = A + r.b1p;
    a.tbias = h->fw.tb + r.tb_off; a.step_ptr = c.step_ptr; a.ts = c.ts; a.tb_stride = h->tb_stride;
    a.W2 = A + r.W2p; a.gamma2 = A + r.g2p; a.beta2 = A + r.b2p; a.c2 = A + r.c2p;
    a.Wc = A + r.Wcp; a.condfrag = h->fw.condfrag; a.cond_groups = groups_of(h->d.cond_dim);
    a.W3 = A + r.W3p; a.gamma3 = A + r.g3p; a.beta3 = A + r.b3p; a.c3 = A + r.c3p;
    a.Wsc = r.sclin ? A + r.Wscp : nullptr;
    const Seg o = seg_of(h, op.out);
    a.out = const_cast<float*>(o.data); a.out_stats = const_cast<float*>(o.stats);
    if (c.train) { a.save_h1 = trp(h, r.h1); a.save_h2 = trp(h, r.h2); }
    if (c.cond_pre) a.cond_pre = h->fw.cembed + r.ce_off * (cap_tiles_of(h) / 2);
    a.ntiles = tpp * c.npass; a.tiles_per_pass = tpp; a.uncond_tiles = c.uncond_tiles; a.nrows = c.nrows;
    a.range_flag = h->range_flag;
    {
        const float n0 = (float)a.in0.width, n1 = (float)a.in1.width, nt = n0 + n1;
        a.chan_w = n0 * n1 / nt; a.chan_f = n1 / nt; a.inv_nin = 1.0f / nt;
    }
}

void fill_lin_args(const dsg_handle* h, const Op& op, const RunCtx& c, LinArgs& a) {
    const int tpp = cdiv(c.nrows, 32);
    const LinOpP& l = h->lin[op.p];
    const float* A = h->arena;
    memset(&a, 0, sizeof a);
    a.W = A + l.Wp; a.bias = A + l.bp;
    a.in_width = l.l.K; a.in_groups = groups_of(l.l.K);
    a.out_width = l.l.N;
    a.ntiles = tpp * c.npass; a.tiles_per_pass = tpp; a.nrows = c.nrows;
    a.range_flag = h->range_flag;
    a.inv_in_w = 1.0f / (float)l.l.K; a.inv_out_w = 1.0f / (float)l.l.N;
    if (op.kind == OP_PROJ) {
        a.in_rm = c.y; a.advance_step = c.advance_step;
        if (c.share_proj) a.ntiles = tpp;            // one pass: the second pass's consumers wrap onto these tiles
    } else {
        a.in = seg_of(h, op.in0);
        if (c.share_proj && op.in0 == h->ops[0].out) a.in.wrap = tpp;
    }
    if (op.kind == OP_FINAL) {
        a.gamma = A + l.gp; a.beta = A + l.betap; a.out_rm = c.eps_out;
    } else {
        const Seg o = seg_of(h, op.out);
        a.out = const_cast<float*>(o.data); a.out_stats = const_cast<float*>(o.stats);
    }
}

void fill_block_args_h(const dsg_handle* h, const ResP& r, const BlockArgs& b, BlockArgsH& a) {
    a.b = b;
    const float* A = h->arena;
    a.W1h = reinterpret_cast<const uint4*>(A + r.W1h); a.W2h = reinterpret_cast<const uint4*>(A + r.W2h);
    a.W3h = reinterpret_cast<const uint4*>(A + r.W3h); a.Wsch = r.sclin ? reinterpret_cast<const uint4*>(A + r.Wsch) : nullptr;
    a.m1 = h->maxabs + r.l1.w; a.m2 = h->maxabs + r.l2.w; a.m3 = h->maxabs + r.l3.w; a.msc = r.sclin ? h->maxabs + r.sc.w : nullptr;
    a.kc = h->opc_dev + 4 * (size_t)(&r - h->res.data());
}
void fill_lin_args_h(const dsg_handle* h, const LinOpP& l, const LinArgs& b, LinArgsH& a) {
    a.l = b;
    a.Wh = reinterpret_cast<const uint4*>(h->arena + l.Wh);
    a.m = h->maxabs + l.l.w;
    a.kc = h->opc_dev + 4 * (h->res.size() + (size_t)(&l - h->lin.data()));
}

// k_wide128_h: 128-wide block whose inputs are one or two 128-wide tensors, condition embedding precomputed
bool wide128_ok(const ResP& r, const BlockArgs& b) {
    return r.N == 128 && b.in0.groups == 16 && (b.in1.groups == 0 || b.in1.groups == 16) && (b.in1.groups != 0) == r.sclin && b.cond_pre;
}

// persistent panel kernels (dsg_panel.hpp): sampling launches only (the time bias is one row: no per-row `ts`)
bool panel128_ok(const dsg_handle* h, const ResP& r, const BlockArgs& b) {
    return wide128_ok(r, b) && !b.ts && !b.save_h1 && b.tiles_per_pass * 2 >= b.ntiles && b.ntiles >= h->panel_min_tiles &&
           b.ntiles > h->coop_max_tiles;
}
// grid of a persistent kernel: one workgroup per group of row tiles, at most `per_cu` workgroups per CU
inline dim3 persistent_grid(const dsg_handle* h, int ngroups, int per_cu = 1) {
    return dim3(ngroups < per_cu * h->num_cus ? ngroups : per_cu * h->num_cus);
}
template <bool SC, int EPI, int NTO>
void launch_panel128(const dsg_handle* h, const BlockLinArgsH& w, hipStream_t s) {
    if (h->opt_panel_half) {
        // half-size panels, 4 waves per workgroup, two workgroups per CU (dsg_panel.hpp, STEPS = 2)
        const int ngroups = cdiv(w.b.b.ntiles, 4);
        hipLaunchKernelGGL((k_panel128_h<SC, EPI, NTO, 2>), persistent_grid(h, ngroups, 2), dim3(256), 0, s, w, ngroups);
        return;
    }
    const int ngroups = cdiv(w.b.b.ntiles, kPW);
    hipLaunchKernelGGL((k_panel128_h<SC, EPI, NTO>), persistent_grid(h, ngroups), dim3(kPW * 64), 0, s, w, ngroups);
}

// Both guidance passes of a row tile in one wave (k_panel128_duo_h, DSG_OPT_CFG_SHARE).  The ONE copy of the rule; the caller has
// established panel128_ok and that no Linear is fused behind the block.  The block reads the shared feature_proj (one tile for both
// passes), the launch is exactly two passes with the first one unconditional, and the condition embeddings are precomputed.
bool cfg_share_ok(const dsg_handle* h, const ResP& r, const BlockArgs& b) {
    return h->opt_cfg_share && !r.sclin && b.tiles_per_pass > 0 && b.in0.wrap == b.tiles_per_pass && b.ntiles == 2 * b.tiles_per_pass &&
           b.uncond_tiles == b.tiles_per_pass && b.cond_pre;
}
void launch_panel128_duo(const dsg_handle* h, const BlockArgsH& a, hipStream_t s) {
    if (h->opt_panel_half) {
        const int ngroups = cdiv(a.b.tiles_per_pass, 4);
        hipLaunchKernelGGL((k_panel128_duo_h<2>), persistent_grid(h, ngroups, 2), dim3(256), 0, s, a, ngroups);
        return;
    }
    const int ngroups = cdiv(a.b.tiles_per_pass, kPW);
    hipLaunchKernelGGL((k_panel128_duo_h<4>), persistent_grid(h, ngroups), dim3(kPW * 64), 0, s, a, ngroups);
}

// 64-wide blocks of large sampling launches: the block's planes resident in LDS (dsg_res64.hpp)
bool res64_lds_ok(const dsg_handle* h, const ResP& r, const BlockArgs& b) {
    return r.N == 64 && b.in0.groups == 8 && (b.in1.groups == 0 || b.in1.groups == 8) && (b.in1.groups != 0) == r.sclin && b.cond_pre && !b.ts &&
           !b.save_h1 && b.tiles_per_pass * 2 >= b.ntiles && b.ntiles >= h->panel_min_tiles && b.ntiles > h->coop_max_tiles;
}

// The cooperative wide-block body (resblock_coop_body, k_resblock_c and k_unet_tile) fits: a 64- / 128-wide block whose inputs are
// exactly N wide (compile-time step counts) and whose first-stage image takes at most half of its tile slot of the LDS buffer.
// The ONE copy of the rule: launch_res_h and the whole-net table of k_unet_tile (build_tile_table) both ask here.  For the four shapes
// create_impl builds (N = 64 / 128, with and without the Linear shortcut: ks1 = N / 16 or N / 8) the slot bound holds with equality
// in the shortcut case and with a factor of two to spare otherwise.
bool coop_fits(const ResP& r) {
    if (r.N != 64 && r.N != 128) return false;
    const int ks1 = (groups_of(r.in0) + 1) / 2 + (groups_of(r.in1) + 1) / 2, tpw = 4 / (r.N / 32);
    return ks1 * 128 <= kCoopLdsU4 / tpw / 2 && r.in0 == r.N && r.in1 == (r.sclin ? r.N : 0);
}

// a block alone through a block + Linear kernel: no Linear (EPI / NTO = 0), the block's output stored
BlockLinArgsH block_only(const BlockArgsH& a) {
    BlockLinArgsH w;
    memset(&w, 0, sizeof w);
    w.b = a; w.store_block_out = 1;
    return w;
}

void launch_res_h(const dsg_handle* h, const ResP& r, const BlockArgs& b, hipStream_t s) {
    BlockArgsH a;
    fill_block_args_h(h, r, b, a);
    const dim3 block(256);
    // launches with few row tiles leave SIMDs idle with one wave per tile: the wide blocks then run cooperatively (N/32 waves per tile,
    // k_resblock_c).  The training forward (it stores h1 / h2) takes the cooperative form up to 1 024 tiles -- 32 768 rows: 1.939 -> 1.923
    // ms per step (profiles/r04_train_tail_ab.txt); a sampling launch of that size has two passes' worth of tiles per row and stays as measured
    const int coop_max = (a.b.save_h1 && h->coop_max_tiles > 0 && h->coop_max_tiles < kCoopMaxTilesTrain) ? kCoopMaxTilesTrain : h->coop_max_tiles;
    if (coop_fits(r) && a.b.ntiles <= coop_max) {
        const dim3 grid(cdiv(a.b.ntiles, 4 / (r.N / 32)));
        dispatch_bool(r.sclin, [&](auto sc) {
            if (r.N == 128) hipLaunchKernelGGL((k_resblock_c<128, DSG_V(sc)>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((k_resblock_c<64, DSG_V(sc)>), grid, block, 0, s, a);
        });
        return;
    }
    if (res64_lds_ok(h, r, a.b)) {
        const int ngroups = cdiv(a.b.ntiles, kR64Waves);
        const BlockLinArgsH w = block_only(a);
        dispatch_bool(r.sclin, [&](auto sc) {
            hipLaunchKernelGGL((k_res64_lds<DSG_V(sc), 0>), persistent_grid(h, ngroups), dim3(kR64Waves * 64), 0, s, w, ngroups);
        });
        return;
    }
    if (panel128_ok(h, r, a.b)) {
        if (cfg_share_ok(h, r, a.b)) { launch_panel128_duo(h, a, s); return; }
        if (r.sclin) launch_panel128<true, 0, 1>(h, block_only(a), s); else launch_panel128<false, 0, 1>(h, block_only(a), s);
        return;
    }
    if (wide128_ok(r, a.b)) {
        // large launch, 128 wide: 4 tiles per workgroup, weight planes shared through an LDS ring (dsg_wide.hpp)
        const BlockLinArgsH w = block_only(a);
        dispatch_bool(r.sclin, [&](auto sc) { hipLaunchKernelGGL((k_wide128_h<DSG_V(sc), 0, 1>), dim3(cdiv(a.b.ntiles, 4)), block, 0, s, w); });
        return;
    }
    dispatch_width(r.N, [&](auto n) { dispatch_bool(r.sclin, [&](auto sc) {
        hipLaunchKernelGGL((k_resblock_h<DSG_V(n), DSG_V(sc)>), wave_grid(a.b.ntiles), block, 0, s, a);
    }); });
}
void launch_lin_h(int N, int inmode, int outmode, bool lnact, const LinArgsH& a, hipStream_t s) {
    dispatch_tiles(cdiv(N, 32), [&](auto nt) { DSG_LIN_FORMS(k_linear_h, DSG_V(nt), a.l.ntiles, a); });
}

// block (64/128 wide) + the Linear that consumes it, in one launch; returns false if the shape pair is not instantiated
bool launch_res_lin_h(const dsg_handle* h, const ResP& r, const BlockArgs& b, const LinOpP& l, const LinArgs& la, bool final_op,
                      bool store_block_out, hipStream_t s) {
    BlockLinArgsH a;
    fill_block_args_h(h, r, b, a.b);
    fill_lin_args_h(h, l, la, a.l);
    a.store_block_out = store_block_out ? 1 : 0;
    a.dbg = 0;
    const dim3 grid = wave_grid(b.ntiles), block(256);
    const int NTO = cdiv(l.l.N, 32), EPI = final_op ? 2 : 1;
    if (res64_lds_ok(h, r, b) && l.l.K == 64 && !final_op) {
        const int ngroups = cdiv(b.ntiles, kR64Waves);
        const dim3 g64 = persistent_grid(h, ngroups), b64(kR64Waves * 64);
#define DSG_R64(SC_, NTO_) DSG_TRY_LAUNCH(r.sclin == SC_ && NTO == NTO_, hipLaunchKernelGGL((k_res64_lds<SC_, NTO_>), g64, b64, 0, s, a, ngroups))
        DSG_R64(true, 4) DSG_R64(true, 2) DSG_R64(false, 2) DSG_R64(false, 1)
#undef DSG_R64
    }
    // (block has the Linear shortcut, epilogue, out tiles of the Linear): the panel and the LDS-ring form share one list
#define DSG_W128(LAUNCH) LAUNCH(false, 1, 2) LAUNCH(false, 1, 1) LAUNCH(true, 2, 1) LAUNCH(true, 2, 3)
#define DSG_W128_IS(SC_, EPI_, NTO_) (r.sclin == SC_ && EPI == EPI_ && NTO == NTO_)
    if (panel128_ok(h, r, b) && l.l.K == 128) {
#define DSG_PANEL(SC_, EPI_, NTO_) DSG_TRY_LAUNCH(DSG_W128_IS(SC_, EPI_, NTO_), (launch_panel128<SC_, EPI_, NTO_>(h, a, s)))
        DSG_W128(DSG_PANEL)
#undef DSG_PANEL
    }
    if (wide128_ok(r, b) && l.l.K == 128) {
#define DSG_RING(SC_, EPI_, NTO_) DSG_TRY_LAUNCH(DSG_W128_IS(SC_, EPI_, NTO_), hipLaunchKernelGGL((k_wide128_h<SC_, EPI_, NTO_>), grid, block, 0, s, a))
        DSG_W128(DSG_RING)
#undef DSG_RING
    }
#undef DSG_W128
#undef DSG_W128_IS
#define DSG_PAIR(N_, SC_, NTO_, FIN_) \
    DSG_TRY_LAUNCH(r.N == N_ && r.sclin == SC_ && NTO == NTO_ && final_op == FIN_, hipLaunchKernelGGL((k_resblock_lin_h<N_, SC_, NTO_, FIN_>), grid, block, 0, s, a))
    DSG_PAIR(128, false, 2, false) DSG_PAIR(128, false, 1, false) DSG_PAIR(64, true, 4, false) DSG_PAIR(64, false, 2, false)
    DSG_PAIR(64, true, 2, false) DSG_PAIR(64, false, 1, false)
    DSG_PAIR(128, true, 1, true) DSG_PAIR(128, true, 3, true) DSG_PAIR(64, true, 1, true) DSG_PAIR(64, true, 3, true)
#undef DSG_PAIR
    return false;
}

bool split_ctx(const dsg_handle* h, const RunCtx& c) { return h->use_split && c.cond_pre; }

// AttentionBlock: one launch per operator, exact float32 MFMA under both precision modes (dsg_attn.hpp)
void launch_attn(const dsg_handle* h, const Op& op, const RunCtx& c, hipStream_t s) {
    const AttnP& t = h->attn[op.p];
    const float* A = h->arena;
    const int tpp = cdiv(c.nrows, 32);
    AttnArgs a;
    memset(&a, 0, sizeof a);
    a.l.in = seg_of(h, op.in0);
    a.l.in_width = t.N; a.l.in_groups = groups_of(t.N); a.l.out_width = t.N;
    a.l.ntiles = tpp * c.npass; a.l.tiles_per_pass = tpp; a.l.nrows = c.nrows;
    a.l.inv_in_w = a.l.inv_out_w = 1.0f / (float)t.N;
    const Seg o = seg_of(h, op.out);
    a.l.out = const_cast<float*>(o.data); a.l.out_stats = const_cast<float*>(o.stats);
    a.Wv = A + t.Wvp; a.bv = A + t.bvp; a.Wo = A + t.Wop; a.bo = A + t.bop;
    a.save_v = c.train ? trp(h, t.v) : nullptr;
    const dim3 grid = wave_grid(a.l.ntiles), block(256);
    const bool split = split_ctx(h, c) && t.N >= 64;          // dsg_set_precision: the split-f16 form is the default from 64 wide on
    if (split) {
        a.l.range_flag = h->range_flag;
        a.Wvh = reinterpret_cast<const uint4*>(A + t.Wvh); a.Woh = reinterpret_cast<const uint4*>(A + t.Woh);
        a.mv = h->maxabs + t.proj.w; a.mo = h->maxabs + t.out.w;
    }
    // an AttentionBlock is 8 .. 128 wide, a power of two (create_impl): 1, 2 or 4 feature tiles, the split form from 2 on
    dispatch_tiles(cdiv(t.N, 32), [&](auto nt) {
        if constexpr (DSG_V(nt) != 3) {
            if constexpr (DSG_V(nt) >= 2) if (split) { hipLaunchKernelGGL(k_attn_h<DSG_V(nt)>, grid, block, 0, s, a); return; }
            hipLaunchKernelGGL(k_attn<DSG_V(nt)>, grid, block, 0, s, a);
        }
    });
}
void launch_attn_bwd(const dsg_handle* h, const Op& op, int tiles, hipStream_t s) {
    const AttnP& t = h->attn[op.p];
    const float* A = h->arena;
    AttnBwdArgs a;
    memset(&a, 0, sizeof a);
    a.gout_a = trp(h, h->tensors[op.out].ga);
    a.gout_b = h->tensors[op.out].is_skip ? trp(h, h->tensors[op.out].gb) : nullptr;
    a.WoT = A + t.WoT; a.WvT = A + t.WvT;
    a.dv = trp(h, t.dv);
    // a STORE into the producer's chain slot, as every backward kernel here does (ga has one writer, gb the skip consumer): the residual
    // block in front of an attention operator is never a skip tensor and the operator is its only consumer (checked in create_impl)
    a.gin = trp(h, h->tensors[op.in0].ga);
    a.groups = groups_of(t.N); a.ntiles = tiles;
    dispatch_tiles(cdiv(t.N, 32), [&](auto nt) {
        if constexpr (DSG_V(nt) != 3) hipLaunchKernelGGL(k_attn_bwd<DSG_V(nt)>, wave_grid(tiles), dim3(256), 0, s, a);
    });
}

// Exact path, two-pass launches with the step counter (the reverse loop, dsg_time_op): a narrow operator OUTSIDE the fused run (fuse_lo / fuse_hi is only the longest run: a net with two narrow
// runs, or one whose run the attention operators cut up, has others) goes through k_fused_narrow as a chain of ONE operator (second
// half of the table, prepare_fused) -- the register-input form of the block body, which is what the exact path's sampling launches of
// every shipped net run for <= 32-wide blocks.  The plain per-operator launch (k_resblock<32> with the step counter, precomputed
// condition embeddings and two passes of >= 2 row tiles each in one launch) returns a wrong UNCONDITIONAL pass (eps off by ~1e-2
// relative; one tile per pass and the conditional pass are exact) -- with or without attention (proj_dim 32, dims (64, 32):
// test_attention_gpu.test_exact_path_sampling_of_a_net_with_two_narrow_runs).  The cause is not found; no launch takes that path any more.
bool narrow_singles(const dsg_handle* h, const RunCtx& c) {
    return !split_ctx(h, c) && !c.train && c.step_ptr && !c.ts;
}

void launch_op(const dsg_handle* h, const Op& op, const RunCtx& c, hipStream_t s) {
    if (op.kind == OP_ATTN) { launch_attn(h, op, c, s); return; }
    const long long opi = &op - h->ops.data();       // every caller passes an element of h->ops; anything else takes the plain launch below
    if (narrow_singles(h, c) && fusable(h, op) && opi >= 0 && opi < (long long)h->ops.size()) {
        const int ntiles = cdiv(c.nrows, 32) * c.npass;
        const size_t at = h->ops.size() + 1 + (size_t)opi;
        hipLaunchKernelGGL(k_fused_narrow, dim3(cdiv(ntiles, kWavesPerBlock)), dim3(256), 0, s, (const FusedOp*)(h->tabs[c.set].fused_dev + at), 1, ntiles);
        return;
    }
    if (op.kind == OP_RES) {
        BlockArgs a;
        fill_block_args(h, op, c, a);
        const ResP& r = h->res[op.p];
        if (split_ctx(h, c)) launch_res_h(h, r, a, s);
        else launch_res(r.N, r.sclin, a, s);
    } else {
        LinArgs a;
        fill_lin_args(h, op, c, a);
        const int inmode = op.kind == OP_PROJ ? IN_ROWMAJOR : IN_FRAG;
        const int outmode = op.kind == OP_FINAL ? OUT_ROWMAJOR : OUT_FRAG;
        if (split_ctx(h, c)) {
            LinArgsH ah;
            fill_lin_args_h(h, h->lin[op.p], a, ah);
            launch_lin_h(h->lin[op.p].l.N, inmode, outmode, op.kind == OP_FINAL, ah, s);
        } else {
            launch_lin(h->lin[op.p].l.N, inmode, outmode, op.kind == OP_FINAL, a, s);
        }
    }
}

// the float32 section (the 8-wide bottom of the net on the vector unit, dsg_narrow8.hpp) as the kernels that read it from the global
// image take it: nb = blocks per resolution (the kernels' template argument; 0: no section), at / n = its operators relative to fuse_lo
struct V8Sec { int nb, at, n; };
V8Sec v8_section(const dsg_handle* h, const RunCtx& c) {
    const bool v8 = h->opt_v8 && h->v8_lo >= 0 && h->v8_ncopies > 0 && c.cond_pre;
    return v8 ? V8Sec{h->d.n_blocks, h->v8_lo - h->fuse_lo, h->v8_hi - h->v8_lo} : V8Sec{0, -1, 0};
}
// the section's kernels are instantiated for 2 and 3 blocks per resolution (create_impl sets v8_lo for nothing else) and for "none"
template <class F> inline void dispatch_v8nb(int nb, F&& f) { dispatch_ints(nb, f, std::integer_sequence<int, 0, 2, 3>{}); }

// returns the number of operators BEHIND the run that the launch computed as well (0, or 1: the LDS form's tail Linear)
int launch_fused(const dsg_handle* h, const RunCtx& c, hipStream_t s) {
    const int ntiles = cdiv(c.nrows, 32) * c.npass;
    const dim3 grid = wave_grid(ntiles), block(256);
    if (!split_ctx(h, c)) {
        hipLaunchKernelGGL(k_fused_narrow, grid, block, 0, s, h->tabs[c.set].fused_dev, h->fuse_hi - h->fuse_lo, ntiles);
        return 0;
    }
    const FusedOpH* tab = c.train ? h->fusedh_train_dev : h->tabs[c.set].fusedh_dev;
    if (!c.train && !c.ts && h->tabs[c.set].nlds_valid && ntiles >= h->panel_min_tiles && ntiles > h->narrow_small_max_tiles) {
        // large sampling launch: the run's planes and vectors resident in LDS, one launch walks the phases (dsg_split.hpp)
        NarrowPhases P;
        memset(&P, 0, sizeof P);
        P.n = (int)h->tabs[c.set].nlds_phases.size();
        for (int k = 0; k < P.n; ++k) P.p[k] = h->tabs[c.set].nlds_phases[k];
        const NarrowLdsOp* lops = h->tabs[c.set].nlds_ops_dev;
        dispatch_v8nb((h->opt_v8 && h->v8_lo >= 0) ? h->d.n_blocks : 0, [&](auto nb) {
            hipLaunchKernelGGL(k_fused_narrow_lds<DSG_V(nb)>, dim3(cdiv(ntiles, 16)), dim3(1024), 0, s, tab, lops, P, ntiles, c.step_ptr, h->tb_stride);
        });
        return h->tabs[c.set].nlds_tail ? 1 : 0;
    }
    // the 8-wide bottom of the net on the vector unit (float32, dsg_narrow8.hpp) from the global image: sampling launches below the
    // LDS form's threshold, dsg_unet_forward, and the training forward (which stores what the backward pass reads)
    const V8Sec v8 = v8_section(h, c);
    const int st = c.train ? 1 : 0, nops = h->fuse_hi - h->fuse_lo;
    // small launches: the latency of one wave is the kernel time -> first-step weight planes requested a stage ahead
    dispatch_bool(ntiles <= h->narrow_small_max_tiles, [&](auto pre) { dispatch_v8nb(v8.nb, [&](auto nb) {
        hipLaunchKernelGGL((k_fused_narrow_h<DSG_V(pre), DSG_V(nb)>), grid, block, 0, s, tab, nops, ntiles, v8.at, v8.n, (const float*)h->v8_image, st);
    }); });
    return 0;
}

// Operators i and i + 1 of a sampling launch can be one launch as far as the plan goes: the second reads the first, and the pair
// lies outside the fused narrow run
bool pair_outside_run(const dsg_handle* h, int i, const RunCtx& c) {
    if (c.train || i + 1 >= (int)h->ops.size() || h->ops[i + 1].in0 != h->ops[i].out) return false;
    const bool fuse = h->fuse_hi - h->fuse_lo >= 2;
    return !(fuse && i + 1 >= h->fuse_lo && i < h->fuse_hi);
}
bool is_wide_block_and_linear(const dsg_handle* h, int i) {
    const Op& a = h->ops[i];
    const Op& b = h->ops[i + 1];
    return a.kind == OP_RES && (b.kind == OP_LIN || b.kind == OP_FINAL) && h->res[a.p].N >= 64;
}

// wide block followed by its consuming Linear (Down/Upsample or final), both outside the fused narrow run
bool try_pair(const dsg_handle* h, int i, const RunCtx& c, hipStream_t s) {
    if (!split_ctx(h, c) || !pair_outside_run(h, i, c) || !is_wide_block_and_linear(h, i)) return false;
    if (cdiv(c.nrows, 32) * c.npass <= h->coop_max_tiles) return false;   // small launch: cooperative block, then the Linear
    const Op& a = h->ops[i];
    const Op& b = h->ops[i + 1];
    BlockArgs ba; LinArgs la;
    fill_block_args(h, a, c, ba);
    fill_lin_args(h, b, c, la);
    return launch_res_lin_h(h, h->res[a.p], ba, h->lin[b.p], la, b.kind == OP_FINAL, h->tensors[a.out].is_skip, s);
}

// exact path: the same pairs (k_resblock_lin, dsg_kernels.hpp) when both input tensors of the block have N / 8 groups
bool try_pair_f32(const dsg_handle* h, int i, const RunCtx& c, hipStream_t s) {
    if (split_ctx(h, c) || !h->opt_f32_pair || !pair_outside_run(h, i, c) || !is_wide_block_and_linear(h, i)) return false;
    const Op& a = h->ops[i];
    const Op& b = h->ops[i + 1];
    const ResP& r = h->res[a.p];
    BlockArgs ba; LinArgs la;
    fill_block_args(h, a, c, ba);
    fill_lin_args(h, b, c, la);
    if (ba.in0.groups != r.N / 8 || ba.in1.groups != (r.sclin ? r.N / 8 : 0) || la.in_groups != r.N / 8) return false;
    const bool fin = b.kind == OP_FINAL;
    const int NTO = cdiv(h->lin[b.p].l.N, 32), store = h->tensors[a.out].is_skip ? 1 : 0;
    const dim3 grid = wave_grid(ba.ntiles), block(256);
#define DSG_PAIR32(N_, SC_, NTO_, FIN_) \
    DSG_TRY_LAUNCH(r.N == N_ && r.sclin == SC_ && NTO == NTO_ && fin == FIN_, hipLaunchKernelGGL((k_resblock_lin<N_, SC_, NTO_, FIN_>), grid, block, 0, s, ba, la, store))
    DSG_PAIR32(128, false, 2, false) DSG_PAIR32(64, true, 4, false) DSG_PAIR32(128, true, 3, true) DSG_PAIR32(128, true, 1, true)
    DSG_PAIR32(128, false, 1, false) DSG_PAIR32(64, true, 2, false) DSG_PAIR32(64, true, 1, true) DSG_PAIR32(64, true, 3, true)
#undef DSG_PAIR32
    return false;
}

// two consecutive down-64 blocks of a large sampling launch in one launch (k_res64_dual)
bool try_dual64(const dsg_handle* h, int i, const RunCtx& c, hipStream_t s) {
    if (!split_ctx(h, c) || !pair_outside_run(h, i, c)) return false;
    const Op& oa = h->ops[i];
    const Op& ob = h->ops[i + 1];
    if (oa.kind != OP_RES || ob.kind != OP_RES) return false;
    const ResP& ra = h->res[oa.p];
    const ResP& rb = h->res[ob.p];
    if (ra.N != 64 || rb.N != 64 || ra.sclin || rb.sclin) return false;
    BlockArgs ba, bb;
    fill_block_args(h, oa, c, ba);
    fill_block_args(h, ob, c, bb);
    if (!res64_lds_ok(h, ra, ba) || !res64_lds_ok(h, rb, bb)) return false;
    if (bb.in0.wrap || ba.ntiles != bb.ntiles || ba.tiles_per_pass != bb.tiles_per_pass || ba.uncond_tiles != bb.uncond_tiles) return false;
    BlockArgsH a0, a1;
    fill_block_args_h(h, ra, ba, a0);
    fill_block_args_h(h, rb, bb, a1);
    const int ngroups = cdiv(ba.ntiles, kR64Waves);
    hipLaunchKernelGGL(k_res64_dual, persistent_grid(h, ngroups), dim3(kR64Waves * 64), 0, s, a0, a1, ngroups);
    return true;
}

// Small launches: feature_proj, then ONE launch that carries every row tile through the rest of the net (dsg_tile.hpp)
bool tile_step_ok(const dsg_handle* h, const RunCtx& c) {
    return h->opt_tile && h->tabs[c.set].tile_valid && split_ctx(h, c) && !c.train && !c.ts && h->fuse_hi - h->fuse_lo >= 2 &&
           cdiv(c.nrows, 32) * c.npass <= h->coop_max_tiles;
}
void launch_tile_step(const dsg_handle* h, const RunCtx& c, hipStream_t s) {
    launch_op(h, h->ops[0], c, s);            // feature_proj: moves the device step counter on (reverse loop), one pass when shared
    const int ntiles = cdiv(c.nrows, 32) * c.npass, nops = (int)h->ops.size();
    const V8Sec v8 = v8_section(h, c);
    dispatch_v8nb(v8.nb, [&](auto nb) {
        hipLaunchKernelGGL((k_unet_tile<DSG_V(nb)>), dim3(ntiles), dim3(256), 0, s, (const FusedOpH*)h->tabs[c.set].tileops_dev, 1, nops, ntiles, h->fuse_lo, h->fuse_hi,
                           v8.at, v8.n, (const float*)h->v8_image);
    });
}

// The ONE walk over the operators of a forward pass: the fused narrow run as one launch, the pair forms where they apply, every other
// operator on its own.  `before(i)` / `after(i)` run around EVERY operator index, in order, with the operator's launch between them --
// an operator that an earlier launch covered (the rest of the narrow run, the second of a pair) has nothing between them.
// f32_pairs: whether the exact path's block + Linear pairs (try_pair_f32) are tried.
template <class Before, class After>
int walk_ops(const dsg_handle* h, const RunCtx& c, hipStream_t s, bool f32_pairs, Before&& before, After&& after) {
    const bool fuse = (!c.train || split_ctx(h, c)) && h->fuse_hi - h->fuse_lo >= 2;
    int covered = 0;                       // operators behind the current launch that it computed as well
    for (int i = 0; i < (int)h->ops.size(); ++i) {
        if (before(i)) return 1;
        if (covered > 0) --covered;
        else if (fuse && i == h->fuse_lo) covered = h->fuse_hi - h->fuse_lo - 1 + launch_fused(h, c, s);
        else if (try_dual64(h, i, c, s) || try_pair(h, i, c, s) || (f32_pairs && try_pair_f32(h, i, c, s))) covered = 1;
        else launch_op(h, h->ops[i], c, s);
        if (after(i)) return 1;
    }
    return 0;
}

void run_unet(const dsg_handle* h, const RunCtx& c, hipStream_t s) {
    if (tile_step_ok(h, c)) { launch_tile_step(h, c, s); return; }
    const auto none = [](int) { return 0; };
    (void)walk_ops(h, c, s, /*f32_pairs=*/true, none, none);
}

}  // namespace
