// Part of the ONE translation unit dsg_api.hip (included from there, after the kernel headers and `using namespace dsg`): not a
// stand-alone header.  Training: the workspace, the descriptor tables (build_train_descs) and the step (train_step_impl).
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------------
// training workspace + descriptor tables
// ------------------------------------------------------------------------------------------------------
int ensure_train_workspace(dsg_handle* h, int rows, int T) {
    if (ensure_workspace(h, rows, T)) return 1;
    if (h->tr.ws && rows <= h->tr_rows && T == h->tr_T) return 0;
    HIPCK(hipDeviceSynchronize());
    const int nrows = rows > h->tr_rows ? rows : h->tr_rows;
    free_train_workspace(h);
    h->tr_rows = nrows; h->tr_T = T;
    const size_t tiles = tr_tiles_of(h);
    const int D = h->d.input_dim, td = h->td, half = h->d.proj_dim / 2;
    // slab = [flat parameter gradients | dTB_b [N_b][T] for every block]
    long long so = h->total_params;
    for (auto& r : h->res) { r.dtb_off = so; so += (long long)r.N * T; }
    h->slab_stride = (size_t)((so + 63) / 64 * 64);
    const int max_chunks = 32;
    HIPCK(h->tr.ws.alloc(tiles * h->tr_per_tile));
    HIPCK(hipMemset(h->tr.ws, 0, tiles * h->tr_per_tile * sizeof(float)));
    HIPCK(h->tr.slabs.alloc((size_t)max_chunks * h->slab_stride));
    // INVARIANT (AttentionBlock): the slab entries of attn.norm.* and of rows 0:2d of attn.projection.* are written by NOTHING after this
    // memset -- no weight-gradient unit, column sum or one-hot unit has an out_off inside them -- so the fixed-order reduce stores exact
    // zeros for them into the caller's bucket on every step.  Whoever adds a writer to those ranges must zero them per step instead.
    HIPCK(hipMemset(h->tr.slabs, 0, (size_t)max_chunks * h->slab_stride * sizeof(float)));
    HIPCK(h->tr.gsum.alloc(h->slab_stride));
    // + one set per early weight-gradient part + the complete set of the step's tail (the blocks' slots AND the Linears')
    HIPCK(h->tr.gmax.alloc((size_t)(2 + kMaxWgParts) * kMaxGmax));
    h->gmax_ld = (int)tiles;
    HIPCK(h->tr.gmax_t.alloc((size_t)kMaxGmax * h->gmax_ld));
    {   // per-tile column sums of the residual blocks, one contiguous [tile][slot] region per block:
        // [dout | dh2 | dh1 | beta3 | gamma3 | beta2 | gamma2] x NP, [beta1 | gamma1] x KP
        const Param* P = h->params.data();
        size_t off = 0;
        std::vector<int4> map;
        size_t base = 0, stride = 0, slot = 0;
        auto vec = [&](int width_pad, int w0, int w1, long long d0, long long d1) {
            // padded feature order: each concat segment padded to whole groups
            const int g0 = groups_of(w0);
            for (int f = 0; f < width_pad; ++f, ++slot) {
                const int G = f >> 3, e = f & 7;
                int col = -1;
                if (G < g0) { if (8 * G + e < w0) col = 8 * G + e; }
                else { const int c = 8 * (G - g0) + e; if (c < w1) col = w0 + c; }
                map.push_back(make_int4(col >= 0 ? (int)(d0 + col) : -1, (col >= 0 && d1 >= 0) ? (int)(d1 + col) : -1, (int)(base + slot), (int)stride));
            }
        };
        for (auto& r : h->res) {
            const int NP = cdiv(r.N, 32) * 32;
            const int KGT = r.sclin ? cdiv(2 * groups_of(r.N), 4) : cdiv(r.N, 32);   // as resblock_bwd_body
            const int KP = KGT * 32;
            r.cs_off = off; r.cs_stride = (size_t)7 * NP + 2 * KP;
            base = off; stride = r.cs_stride; slot = 0;
            vec(NP, r.N, 0, P[r.l3.b].off, r.sclin ? P[r.sc.b].off : -1);
            vec(NP, r.N, 0, P[r.l2.b].off, P[r.ce.b].off);
            vec(NP, r.N, 0, P[r.l1.b].off, P[r.te.b].off);
            vec(NP, r.N, 0, P[r.n3.b].off, -1);
            vec(NP, r.N, 0, P[r.n3.w].off, -1);
            vec(NP, r.N, 0, P[r.n2.b].off, -1);
            vec(NP, r.N, 0, P[r.n2.w].off, -1);
            vec(KP, r.in0, r.in1, P[r.n1.b].off, -1);
            vec(KP, r.in0, r.in1, P[r.n1.w].off, -1);
            off += tiles * r.cs_stride;
        }
        if (off >= ((size_t)1 << 31)) { fail("training batch too large for the column-sum index (%zu floats)", off); return 1; }
        h->cs_slots = (int)map.size();
        HIPCK(h->tr.cs.alloc(off));
        HIPCK(h->tr.cs_map_dev.alloc(map.size()));
        HIPCK(hipMemcpy(h->tr.cs_map_dev, map.data(), map.size() * sizeof(int4), hipMemcpyHostToDevice));
    }
    HIPCK(h->tr.ts.alloc((size_t)nrows));
    HIPCK(h->tr.yt_rm.alloc((size_t)nrows * D));
    HIPCK(h->tr.tsave.alloc((size_t)T * 2 * half + (size_t)(5 + kTimeChunks) * T * td));
    return 0;
}

// Descriptors depend on the batch size of THIS call (tile counts, row masks) and on T: rebuilt per call (host only,
// one upload); cheap next to the step.
// Arguments of one operator's activation-gradient kernel (dsg_train_step, and the fused narrow backward's table)
void fill_res_bwd_args(const dsg_handle* h, const Op& op, int tiles, BlockBwdArgs& a, BlockBwdArgsH& ah) {
    const float* A = h->arena;
    const ResP& r = h->res[op.p];
    memset(&a, 0, sizeof a);
    a.in0 = seg_of(h, op.in0);
    if (op.in1 >= 0) a.in1 = seg_of(h, op.in1);
    a.h1 = trp(h, r.h1); a.h2 = trp(h, r.h2);
    a.gout_a = trp(h, h->tensors[op.out].ga);
    a.gout_b = h->tensors[op.out].is_skip ? trp(h, h->tensors[op.out].gb) : nullptr;
    a.W3T = A + r.W3T; a.W2T = A + r.W2T; a.W1T = A + r.W1T; a.WscT = r.sclin ? A + r.WscT : nullptr;
    a.gamma1 = A + r.g1p; a.beta1 = A + r.b1p; a.gamma2 = A + r.g2p; a.beta2 = A + r.b2p; a.gamma3 = A + r.g3p; a.beta3 = A + r.b3p;
    a.gin0 = trp(h, h->tensors[op.in0].ga);
    a.gin1 = op.in1 >= 0 ? trp(h, h->tensors[op.in1].gb) : nullptr;
    a.du1 = trp(h, r.du1); a.dh1 = trp(h, r.dh1); a.dh2 = trp(h, r.dh2);
    a.cs = h->tr.cs + r.cs_off; a.cs_stride = r.cs_stride;
    a.rs1 = trp(h, r.rs1); a.rs2 = trp(h, r.rs2); a.rs3 = trp(h, r.rs3);
    a.ntiles = tiles;
    ah.b = a;
    ah.W3Th = reinterpret_cast<const uint4*>(A + r.W3Th); ah.W2Th = reinterpret_cast<const uint4*>(A + r.W2Th);
    ah.W1Th = reinterpret_cast<const uint4*>(A + r.W1Th);
    ah.WscTh = r.sclin ? reinterpret_cast<const uint4*>(A + r.WscTh) : nullptr;
    ah.m1 = h->maxabs + r.l1.w; ah.m2 = h->maxabs + r.l2.w; ah.m3 = h->maxabs + r.l3.w;
    ah.msc = r.sclin ? h->maxabs + r.sc.w : nullptr;
    ah.gmax_t = h->tr.gmax_t; ah.gmax_ld = h->gmax_ld; ah.slot_out = r.gslot_out; ah.slot_h2 = r.gslot_h2; ah.slot_h1 = r.gslot_h1;
}
void fill_lin_bwd_args(const dsg_handle* h, const Op& op, int tiles, LinBwdArgs& a) {
    const float* A = h->arena;
    const LinOpP& l = h->lin[op.p];
    memset(&a, 0, sizeof a);
    if (op.kind == OP_FINAL) {
        a.gout_a = trp(h, h->tr_deps);
        a.gamma = A + l.gp; a.beta = A + l.betap; a.du = trp(h, l.du); a.rs = trp(h, l.rs);
    } else {
        a.gout_a = trp(h, h->tensors[op.out].ga);
        a.gout_b = h->tensors[op.out].is_skip ? trp(h, h->tensors[op.out].gb) : nullptr;
    }
    a.out_groups = groups_of(l.l.N);
    a.WT = A + l.WT;
    a.in = seg_of(h, op.in0);
    a.gin = trp(h, h->tensors[op.in0].ga);
    a.ntiles = tiles;
}

// host side of the tables build_train_descs uploads
struct TrainDescs {
    std::vector<WgradDesc> wd;
    std::vector<int> wd_op;            // operator (index + 1) each weight-gradient descriptor belongs to
    std::vector<ColsumDesc> cd;
    // part of each operator (index + 1): k for a residual block reached before fork k (only blocks: the scale of their G operands comes
    // from their own backward kernel, a plain Linear's from k_colsum at the end), -1 = the final launch on the caller's stream
    std::vector<int> op_part;
    std::vector<WgradUnit> wu;
    std::vector<ColsumUnit> cu;
    std::vector<FusedBwdOpH> fb;
};

// which residual blocks' weight gradients start early, beside the rest of the activation-gradient chain (wg_fork_ops, op_part)
void assign_wgrad_parts(dsg_handle* h, int tiles, std::vector<int>& op_part) {
    op_part.assign(h->ops.size() + 1, -1);
    h->wg_fork_ops.clear();
    // Only where the step is GPU-bound (>= 1 024 row tiles): the cross-stream hand-offs cost host time, and below that the step is
    // bound by the host's enqueue rate (measured: 32 768 rows 2.65 -> 2.53 ms, 65 536 rows 4.03 -> 3.98; 16 384 rows 2.00 -> 2.26).
    if (!(h->use_split && tiles >= kWgForkMinTiles)) return;
    int n = 0;
    size_t k = 0;
    for (int oi = (int)h->ops.size() - 1; oi >= 0 && k < h->wg_forks.size(); --oi) {
        if (h->ops[oi].kind != OP_RES) continue;
        op_part[oi + 1] = (int)k;
        if (++n == h->wg_forks[k]) { h->wg_fork_ops.push_back(oi); ++k; }
    }
    if (k < h->wg_forks.size())                   // fewer blocks than the last fork asks for: those stay in the final launch
        for (size_t i = 0; i < op_part.size(); ++i) if (op_part[i] == (int)k) op_part[i] = -1;
    // one more part: the residual blocks of the fused narrow run (17 of MSR-80c's 27 blocks, ~2 700 small units).  Their backward is
    // one launch (k_fused_narrow_bwd_h); behind it the chain still has the 64- and 128-wide down blocks to go.
    if (k == h->wg_forks.size() && h->opt_wg_narrow_part && h->fuse_hi - h->fuse_lo >= 2 && (int)h->wg_fork_ops.size() < kMaxWgParts) {
        int lowest = -1;
        for (int oi = h->fuse_hi - 1; oi >= h->fuse_lo; --oi)
            if (h->ops[oi].kind == OP_RES && op_part[oi + 1] < 0) { op_part[oi + 1] = (int)k; lowest = oi; }
        if (lowest >= 0) h->wg_fork_ops.push_back(lowest);
    }
}

// collects the weight-gradient and column-sum descriptors of every operator, and the slot of max|G| of every distinct G tensor
struct TrainDescCollector {
    dsg_handle* h; int B, T;
    TrainDescs& t;
    int cur_op = 0;
    std::vector<int> bwd_slots;        // slots tracked by the block backward kernels
    std::vector<const float*> gsrc;    // distinct G tensors, by first pointer: slot of max|G|

    int slot_of(const float* g) {
        for (size_t i = 0; i < gsrc.size(); ++i) if (gsrc[i] == g) return (int)i;
        gsrc.push_back(g);
        return (int)gsrc.size() - 1;
    }
    static Seg gseg(const float* data, int width) { Seg sg; sg.data = data; sg.stats = nullptr; sg.groups = groups_of(width); sg.width = width; sg.wrap = 0; return sg; }
    static Seg none() { return gseg(nullptr, 0); }
    const float* grad_a(int tid) const { return trp(h, h->tensors[tid].ga); }
    const float* grad_b(int tid) const { return h->tensors[tid].is_skip ? (const float*)trp(h, h->tensors[tid].gb) : (const float*)nullptr; }
    void wgrad(const float* G0, const float* G1, int N, int amode, Seg a0, Seg a1, const float* rs, const float* gm, const float* bt, long long out_off, int ld) {
        WgradDesc d;
        memset(&d, 0, sizeof d);
        d.G0 = G0; d.G1 = G1; d.N = N; d.NG = groups_of(N); d.amode = amode; d.a0 = a0; d.a1 = a1; d.rs = rs; d.gamma = gm; d.beta = bt;
        d.ts = h->tr.ts; d.onehot_n = T; d.out_off = out_off; d.ld = ld;
        d.KG = amode == A_ONEHOT ? groups_of(T) : a0.groups + a1.groups;
        d.nrows = B;
        d.gmax_slot = slot_of(G0);
        t.wd.push_back(d);
        t.wd_op.push_back(cur_op);
    }
    void colsum(const float* P0, const float* P1, int groups, Seg x0, Seg x1, const float* rs, int w0, int w1, long long o1, long long o1b, long long o2) {
        ColsumDesc d;
        memset(&d, 0, sizeof d);
        d.P0 = P0; d.P1 = P1; d.groups = groups; d.x0 = x0; d.x1 = x1; d.rs = rs; d.w0 = w0; d.w1 = w1;
        d.out_off = o1; d.out_off_b = o1b; d.out2_off = o2;
        d.gmax_slot = o2 < 0 ? slot_of(P0) : -1;     // the plain sums are exactly the G tensors of the weight gradients
        t.cd.push_back(d);
    }
    void collect_op(const Op& op);
    int check();
};

void TrainDescCollector::collect_op(const Op& op) {
    const float* A = h->arena;
    const Param* P = h->params.data();
    ++cur_op;
    if (op.kind == OP_ATTN) {
        // two plain Linears as far as the weight gradients go: output (G = dy, A = v) and rows 2d:3d of projection (G = dv, A = x).
        // Nothing writes the slab entries of projection's q / k rows and of attn.norm: the fixed-order reduce stores their zeros
        // into the caller's bucket every step.
        const AttnP& at = h->attn[op.p];
        const float *ga = grad_a(op.out), *gb = grad_b(op.out), *dv = trp(h, at.dv);
        const long long d = at.N;
        wgrad(ga, gb, at.N, A_RAW, gseg(trp(h, at.v), at.N), none(), nullptr, nullptr, nullptr, P[at.out.w].off, at.N);
        colsum(ga, gb, groups_of(at.N), none(), none(), nullptr, at.N, 0, P[at.out.b].off, -1, -1);
        wgrad(dv, nullptr, at.N, A_RAW, seg_of(h, op.in0), none(), nullptr, nullptr, nullptr, P[at.proj.w].off + 2 * d * d, at.N);
        colsum(dv, nullptr, groups_of(at.N), none(), none(), nullptr, at.N, 0, P[at.proj.b].off + 2 * d, -1, -1);
    } else if (op.kind == OP_RES) {
        ResP& r = h->res[op.p];
        const Seg in0 = seg_of(h, op.in0), in1 = op.in1 >= 0 ? seg_of(h, op.in1) : none();
        const float *ga = grad_a(op.out), *gb = grad_b(op.out);
        const float *dh1 = trp(h, r.dh1), *dh2 = trp(h, r.dh2);
        const int in = r.in0 + r.in1;
        wgrad(dh1, nullptr, r.N, A_LNSILU, in0, in1, trp(h, r.rs1), A + r.g1p, A + r.b1p, P[r.l1.w].off, in);
        if (r.sclin) wgrad(ga, gb, r.N, A_RAW, in0, in1, nullptr, nullptr, nullptr, P[r.sc.w].off, in);
        wgrad(dh2, nullptr, r.N, A_LNSILU, gseg(trp(h, r.h1), r.N), none(), trp(h, r.rs2), A + r.g2p, A + r.b2p, P[r.l2.w].off, r.N);
        wgrad(dh2, nullptr, r.N, A_RAW, gseg(h->fw.condfrag, h->d.cond_dim), none(), nullptr, nullptr, nullptr, P[r.ce.w].off, h->d.cond_dim);
        wgrad(ga, gb, r.N, A_LNSILU, gseg(trp(h, r.h2), r.N), none(), trp(h, r.rs3), A + r.g3p, A + r.b3p, P[r.l3.w].off, r.N);
        wgrad(dh1, nullptr, r.N, A_ONEHOT, none(), none(), nullptr, nullptr, nullptr, r.dtb_off, T);
        // bias and LayerNorm gradients of the block come from the backward kernel's own column sums (k_cs_reduce); so does
        // max|G| of its three gradient tensors
        r.gslot_out = slot_of(ga); r.gslot_h2 = slot_of(dh2); r.gslot_h1 = slot_of(dh1);
        bwd_slots.push_back(r.gslot_out); bwd_slots.push_back(r.gslot_h2); bwd_slots.push_back(r.gslot_h1);
    } else if (op.kind == OP_FINAL) {
        const LinOpP& l = h->lin[op.p];
        const float* deps = trp(h, h->tr_deps);
        const Seg in = seg_of(h, op.in0);
        wgrad(deps, nullptr, l.l.N, A_LNSILU, in, none(), trp(h, l.rs), A + l.gp, A + l.betap, P[l.l.w].off, l.l.K);
        colsum(deps, nullptr, groups_of(h->d.input_dim), none(), none(), nullptr, l.l.N, 0, P[l.l.b].off, -1, -1);
        colsum(trp(h, l.du), nullptr, in.groups, in, none(), trp(h, l.rs), l.l.K, 0, P[l.ln.b].off, -1, P[l.ln.w].off);
    } else {
        const LinOpP& l = h->lin[op.p];
        const float *ga = grad_a(op.out), *gb = grad_b(op.out);
        const Seg a0 = op.kind == OP_PROJ ? gseg(trp(h, h->tr_yt_frag), l.l.K) : seg_of(h, op.in0);
        wgrad(ga, gb, l.l.N, A_RAW, a0, none(), nullptr, nullptr, nullptr, P[l.l.w].off, l.l.K);
        colsum(ga, gb, groups_of(l.l.N), none(), none(), nullptr, l.l.N, 0, P[l.l.b].off, -1, -1);
    }
}

// every G tensor of a weight gradient must be covered by a plain column sum (each Linear has a bias), or its scale is never set
int TrainDescCollector::check() {
    std::vector<char> seen(gsrc.size(), 0);
    for (const ColsumDesc& c : t.cd) if (c.gmax_slot >= 0) seen[c.gmax_slot] = 1;
    for (int sl : bwd_slots) seen[sl] = 1;
    for (const WgradDesc& w : t.wd) if (!seen[w.gmax_slot]) return fail("internal: weight-gradient operand without a tracked maximum");
    if ((int)gsrc.size() > kMaxGmax)
        return fail("dsg_train_step: this net (n_res %d, n_blocks %d) has %d gradient tensors whose maximum is tracked (3 per residual block, "
                    "1 per Linear); training supports at most %d", h->d.n_res, h->d.n_blocks, (int)gsrc.size(), kMaxGmax);
    h->n_gmax = (int)gsrc.size();
    return 0;
}

// Launch order of the (descriptor, k-block, row-chunk) units:
//   * operators with the longest units first (the proj_dim-wide up blocks come last in op order and would form the tail);
//   * inside an operator, 8 row chunks at a time, every unit of the operator over those 8 chunks: workgroup i runs on XCD
//     i % 8, so the units that re-read the same rows of dh1 / dh2 / dout / the block input are neighbours in time on the
//     same XCD and find them in its L2.
void order_wgrad_units(dsg_handle* h, TrainDescs& t) {
    const std::vector<WgradDesc>& wd = t.wd;
    auto cost = [&](int di, int kb) {
        const WgradDesc& d = wd[di];
        const int nt = cdiv(d.N, 32), ntp = nt <= 1 ? 1 : (nt == 2 ? 2 : 4);
        const int ngr = d.KG - kb * 16 < 16 ? d.KG - kb * 16 : 16;
        return ntp * cdiv(ngr, 4);
    };
    struct OpUnits { int cost; std::vector<std::pair<int, int>> u; };
    std::vector<OpUnits> ou;
    for (size_t i = 0; i < wd.size(); ++i) {
        if (i == 0 || t.wd_op[i] != t.wd_op[i - 1]) ou.push_back(OpUnits{0, {}});
        for (int kb = 0; kb < cdiv(wd[i].KG, 16); ++kb) {
            ou.back().u.push_back({(int)i, kb});
            ou.back().cost = std::max(ou.back().cost, cost((int)i, kb));
        }
    }
    std::stable_sort(ou.begin(), ou.end(), [](const OpUnits& a, const OpUnits& b) { return a.cost > b.cost; });
    h->wg_part_end.clear();
    const int nparts = (int)h->wg_fork_ops.size();
    // the final part opens with its time-table (one-hot) units: once they are through, every dTB row of the step is complete and
    // the time path can run on the side stream beside the rest of the final launch (dsg_train_step)
    // ... then the other units of its residual blocks, then the plain Linears' (the scale of a block's G operands is known when
    // the block's backward kernel has run, a Linear's only after k_colsum)
    for (int part = 0; part <= nparts; ++part) {
        for (int pass = (part < nparts ? 2 : 0); pass < 3; ++pass) {
            for (const OpUnits& o : ou) {
                const int op1 = t.wd_op[o.u.front().first];          // operator index + 1
                if (t.op_part[op1] != (part < nparts ? part : -1)) continue;
                const bool block = h->ops[op1 - 1].kind == OP_RES;
                for (int c0 = 0; c0 < h->tr_chunks; c0 += 8)
                    for (const auto& u : o.u) {
                        const int cls = wd[u.first].amode == A_ONEHOT ? 0 : (block ? 1 : 2);
                        if (part == nparts && cls != pass) continue;
                        for (int c = c0; c < c0 + 8 && c < h->tr_chunks; ++c) t.wu.push_back(WgradUnit{u.first, u.second, c, 0});
                    }
            }
            if (part == nparts && pass == 0) h->wg_onehot_end = (int)t.wu.size();
            if (part == nparts && pass == 1) h->wg_blocks_end = (int)t.wu.size();
        }
        if (part < nparts) h->wg_part_end.push_back((int)t.wu.size());
    }
}

// fused narrow backward: the operators of the forward's narrow run, last first (empty: a shape the kernel does not take)
void build_fused_bwd_table(const dsg_handle* h, int tiles, std::vector<FusedBwdOpH>& fb) {
    if (!(h->use_split && h->fuse_hi - h->fuse_lo >= 2)) return;
    bool ok = true;
    for (int oi = h->fuse_hi - 1; oi >= h->fuse_lo && ok; --oi) {
        const Op& op = h->ops[oi];
        FusedBwdOpH f;
        memset(&f, 0, sizeof f);
        if (op.kind == OP_RES) {
            const ResP& r = h->res[op.p];
            BlockBwdArgs a;
            f.kind = 0; f.N = r.N; f.sclin = r.sclin ? 1 : 0;
            fill_res_bwd_args(h, op, tiles, a, f.b);
            ok = r.N <= 32;
        } else if (op.kind == OP_LIN) {
            f.kind = 1; f.ot = cdiv(h->lin[op.p].l.K, 32);
            fill_lin_bwd_args(h, op, tiles, f.l);
            ok = f.ot <= 2;
        } else ok = false;
        fb.push_back(f);
    }
    if (!ok) fb.clear();
}

// the ranges of the flat gradient that the slabs hold: everything but what the time path produces (dsg_train_step); a function of
// the parameter layout only (the slab stride is a multiple of 64 whatever T): built once per handle
int build_reduce_ranges(dsg_handle* h) {
    const Param* P = h->params.data();
    std::vector<std::pair<long long, long long>> skip;
    for (const ResP& r : h->res) skip.push_back({P[r.te.w].off, P[r.te.w].numel});
    for (int pi : {h->temb_l1w, h->temb_l1b, h->temb_l2w, h->temb_l2b}) skip.push_back({P[pi].off, P[pi].numel});
    std::sort(skip.begin(), skip.end());
    std::vector<long long> starts, prefix;
    long long at = 0, acc = 0;
    for (const auto& sk : skip) {
        if (sk.first > at) { starts.push_back(at); prefix.push_back(acc); acc += sk.first - at; }
        at = std::max(at, sk.first + sk.second);
    }
    if (h->total_params > at) { starts.push_back(at); prefix.push_back(acc); acc += h->total_params - at; }
    // every range on a multiple of four elements (all shipped configurations: layer widths are multiples of 4) and the slab stride
    // too: the reduce then moves 16 bytes per access, the table counts float4 units
    bool vec4 = h->slab_stride % 4 == 0;
    for (size_t i = 0; i < starts.size(); ++i) {
        const long long len = (i + 1 < starts.size() ? prefix[i + 1] : acc) - prefix[i];
        if (starts[i] % 4 || len % 4) vec4 = false;
    }
    h->r2_vec4 = vec4;
    h->r2_n = (int)starts.size(); h->r2_total = acc;
    std::vector<long long> tab = starts;      // starts, then prefix sums
    tab.insert(tab.end(), prefix.begin(), prefix.end());
    if (vec4) {                                        // the same table in float4 units behind the scalar one
        for (long long v : starts) tab.push_back(v / 4);
        for (long long v : prefix) tab.push_back(v / 4);
    }
    HIPCK(h->r2_dev.alloc(tab.size()));
    HIPCK(hipMemcpy(h->r2_dev, tab.data(), tab.size() * sizeof(long long), hipMemcpyHostToDevice));
    return 0;
}

int build_train_descs(dsg_handle* h, int B, int T, hipStream_t s) {
    // Rebuilding and uploading the tables costs four pageable host-to-device copies and a stream synchronise - a pipeline
    // drain in front of every step (the enqueue of a step's ~85 launches then no longer hides behind the previous step)
    const void* key[6] = {h->tr.ws, h->fw.ws, h->arena, h->fw.cembed, h->fw.condfrag, h->fw.tb};
    if (h->td_valid && h->td_B == B && h->td_T == T && h->td_rows == h->tr_rows && h->td_split == h->use_split &&
        memcmp(key, h->td_key, sizeof key) == 0)
        return 0;
    h->td_valid = false;
    const int tiles = cdiv(B, 32);
    h->tr_chunks = tiles < 32 ? tiles : 32;
    TrainDescs t;
    assign_wgrad_parts(h, tiles, t.op_part);
    TrainDescCollector col{h, B, T, t};
    for (const Op& op : h->ops) col.collect_op(op);
    if (col.check()) return 1;
    ++h->generation;          // the tables below are rewritten in place (another batch size, T or mode): a captured step would read the new ones
    order_wgrad_units(h, t);
    build_fused_bwd_table(h, tiles, t.fb);
    h->fbwd_n = (int)t.fb.size();
    if (h->fbwd_n) {
        if (!h->fbwd_dev) HIPCK(h->fbwd_dev.alloc(h->ops.size() + 1));
        HIPCK(hipMemcpyAsync(h->fbwd_dev, t.fb.data(), t.fb.size() * sizeof(FusedBwdOpH), hipMemcpyHostToDevice, s));
    }
    // chunk-major, group-minor: neighbouring waves stream neighbouring 1 KiB fragments of the same row tiles
    for (size_t i = 0; i < t.cd.size(); ++i)
        for (int c = 0; c < h->tr_chunks; ++c)
            for (int g = 0; g < t.cd[i].groups; ++g) t.cu.push_back(ColsumUnit{(int)i, g, c, 0});
    if (!h->tr.wg_desc_dev) {
        HIPCK(h->tr.wg_desc_dev.alloc(t.wd.size()));
        HIPCK(h->tr.cs_desc_dev.alloc(t.cd.size()));
    }
    if (h->wg_units != (int)t.wu.size() || !h->tr.wg_unit_dev) HIPCK(h->tr.wg_unit_dev.alloc(t.wu.size()));   // (alloc frees the old table first)
    if (h->cs_units != (int)t.cu.size() || !h->tr.cs_unit_dev) HIPCK(h->tr.cs_unit_dev.alloc(t.cu.size()));
    h->wg_units = (int)t.wu.size(); h->cs_units = (int)t.cu.size();
    HIPCK(hipMemcpyAsync(h->tr.wg_desc_dev, t.wd.data(), t.wd.size() * sizeof(WgradDesc), hipMemcpyHostToDevice, s));
    HIPCK(hipMemcpyAsync(h->tr.cs_desc_dev, t.cd.data(), t.cd.size() * sizeof(ColsumDesc), hipMemcpyHostToDevice, s));
    HIPCK(hipMemcpyAsync(h->tr.wg_unit_dev, t.wu.data(), t.wu.size() * sizeof(WgradUnit), hipMemcpyHostToDevice, s));
    HIPCK(hipMemcpyAsync(h->tr.cs_unit_dev, t.cu.data(), t.cu.size() * sizeof(ColsumUnit), hipMemcpyHostToDevice, s));
    HIPCK(hipStreamSynchronize(s));  // the host vectors of `t` go out of scope
    memcpy(h->td_key, key, sizeof key);
    if (!h->r2_dev && build_reduce_ranges(h)) return 1;
    h->td_B = B; h->td_T = T; h->td_rows = h->tr_rows; h->td_split = h->use_split; h->td_valid = true;
    return 0;
}

void small_gemm(const float* A, long long ai, long long al, const float* B, long long bl, long long bj, float* C, long long ci,
                long long cj, int M, int N, int L, int acc, hipStream_t s) {
    const long long total = (long long)M * N;
    const unsigned blocks = (unsigned)((total + 63) / 64 < 8192 ? (total + 63) / 64 : 8192);
    hipLaunchKernelGGL(k_small_gemm, dim3(blocks), dim3(256), 0, s, A, ai, al, B, bl, bj, C, ci, cj, M, N, L, acc);
}


// the device-side draws of the seeded steps ([rows][D] noise, [rows] mask): allocated on first use, dropped with the training workspace
int ensure_train_draws(dsg_handle* h) {
    if (h->tr.noise) return 0;
    HIPCK(h->tr.noise.alloc((size_t)h->tr_rows * h->d.input_dim));
    HIPCK(h->tr.mask.alloc((size_t)h->tr_rows));
    return 0;
}

// the shapes the backward kernels cannot take (the message is set)
int train_shape_refused(dsg_handle* h) {
    if (h->use_split)
        for (const ResP& r : h->res)
            if (r.N >= 64 && (r.in0 != r.N || (r.in1 != 0 && r.in1 != r.N)))
                return fail("dsg_train_step: no backward kernel for a %d-wide block with inputs %d + %d wide", r.N, r.in0, r.in1);
    return 0;
}

// a training call whose T is not the one of the law or report the handle holds (dsg_set_train_law, dsg_set_train_report): refused by
// the entry points before anything is enqueued -- the kernels index [T]-sized buffers with ts
int train_law_refused(const dsg_handle* h, const char* who, int T) {
    if (h->law_T && T != h->law_T)
        return fail("%s: the handle's train law (dsg_set_train_law) has T = %d, the call has T = %d", who, h->law_T, T);
    if (h->rep_T && T != h->rep_T)
        return fail("%s: the handle's train report (dsg_set_train_report) has T = %d, the call has T = %d", who, h->rep_T, T);
    return 0;
}

// the draws of a seeded step: k_train_draws, or under a law with a CDF its second kernel (same grid, same noise and mask)
void launch_train_draws(const dsg_handle* h, int B, int D, int T, float keep_prob, unsigned long long seed, unsigned call_v,
                        const unsigned long long* call_ptr, hipStream_t s) {
    const size_t blocks = (((size_t)B * D + 3) / 4 + 255) / 256;
    const unsigned grid = (unsigned)(blocks < 4096 ? blocks : 4096);
    if (h->law_T && h->law_has_cdf)
        hipLaunchKernelGGL(k_train_draws_law, dim3(grid), dim3(256), 0, s, h->tr.ts, h->tr.noise, h->tr.mask, B, D, T, keep_prob, seed, call_v,
                           call_ptr, (const unsigned*)h->law_cdf);
    else
        hipLaunchKernelGGL(k_train_draws, dim3(grid), dim3(256), 0, s, h->tr.ts, h->tr.noise, h->tr.mask, B, D, T, keep_prob, seed, call_v, call_ptr);
}

int train_step_impl(dsg_handle* h, const float* y, const float* cond, const int* ts, const float* noise, const float* cond_mask,
                    const float* sqrt_acp, const float* sqrt_1m_acp, int T, float* grads_flat, float* loss_out, int B, hipStream_t s) {
    // every shape the backward kernels cannot take is refused HERE, before anything is enqueued (the same check in the middle of
    // the enqueue left forked streams unjoined and the gradient bucket half written)
    if (train_shape_refused(h) || build_train_descs(h, B, T, s)) return 1;
    const int D = h->d.input_dim, C = h->d.cond_dim, CG = groups_of(C), DG = groups_of(D), tiles = cdiv(B, 32);
    const int td = h->td, half = h->d.proj_dim / 2;
    const float* A = h->arena;
    const Param* P = h->params.data();

    // ---- forward
    auto mark = [&](int i) { if (h->train_prof) (void)hipEventRecord(h->tev[i], s); };
    mark(0);
    if (ts != h->tr.ts) HIPCK(hipMemcpyAsync(h->tr.ts, ts, (size_t)B * sizeof(int), hipMemcpyDeviceToDevice, s));
    // The time path forward (TimeEmbedding + the blocks' time_emb Linears over the T table rows: five short dependent launches) needs
    // nothing of the batch: once the side stream exists (large batches, from the second step on) it runs there, beside the draws'
    // consumers (condition fragments, q-sample, condition embeddings), and joins in front of the first block.
    const bool time_fwd_beside = h->side_stream && h->opt_time_beside && h->use_split;
    hipStream_t tstream = time_fwd_beside ? h->side_stream : s;
    if (time_fwd_beside) {
        HIPCK(hipEventRecord(h->ev_tail[0], s));                           // the weights of this step (optimizer step, re-pack) are in place
        HIPCK(hipStreamWaitEvent(h->side_stream, h->ev_tail[0], 0));
    }
    hipLaunchKernelGGL(k_linspace_t, dim3(cdiv(T, 256)), dim3(256), 0, tstream, h->fw.tvals, T);
    run_time_path(h, T, tstream, true);
    if (time_fwd_beside) HIPCK(hipEventRecord(h->ev_tail[2], h->side_stream));
    hipLaunchKernelGGL(k_cond_frag, dim3(cdiv(tiles * CG * 256, 256)), dim3(256), 0, s, cond, cond_mask, B, C, CG, h->fw.condfrag, tiles,
                       h->use_split ? h->range_flag : nullptr, kCondLimit);
    hipLaunchKernelGGL(k_qsample, dim3(cdiv(tiles * DG * 256, 256)), dim3(256), 0, s, y, noise, h->tr.ts, sqrt_acp, sqrt_1m_acp, B, D,
                       h->tr.yt_rm, trp(h, h->tr_yt_frag), tiles);
    // the forward may run on the split-f16 kernels (they need the condition embeddings as an additive term)
    if (h->use_split) run_cond_embed(h, B, s);
    RunCtx c{B, 1, 0, h->tr.yt_rm, h->fw.eps, nullptr, h->tr.ts, true, h->use_split};
    if (prepare_fused(h, c, s)) return 1;
    if (time_fwd_beside) HIPCK(hipStreamWaitEvent(s, h->ev_tail[2], 0));   // the time table
    run_unet(h, c, s);
    if (h->law_T && h->law_has_w)      // a weight per timestep (dsg_set_train_law): the second kernel; without one, today's launch
        hipLaunchKernelGGL(k_loss_grad_w, dim3(kRedBlocks), dim3(256), 0, s, h->fw.eps, noise, B, D, trp(h, h->tr_deps), tiles, h->red,
                           (const int*)h->tr.ts, (const float*)h->law_w);
    else
        hipLaunchKernelGGL(k_loss_grad, dim3(kRedBlocks), dim3(256), 0, s, h->fw.eps, noise, B, D, trp(h, h->tr_deps), tiles, h->red);
    hipLaunchKernelGGL(k_loss_final, dim3(1), dim3(256), 0, s, h->red, kRedBlocks, (double)B * (double)D, loss_out);
    if (h->rep_T)                      // dsg_set_train_report: one extra small launch, only while a report is held
        hipLaunchKernelGGL(k_loss_report, dim3(h->rep_T), dim3(256), 0, s, h->fw.eps, noise, (const int*)h->tr.ts, B, D, h->rep_sq, h->rep_rows);

    // ---- backward: activation gradients in reverse operator order
    mark(1);
    HIPCK(hipMemsetAsync(h->tr.gmax_t, 0, (size_t)h->n_gmax * h->gmax_ld * sizeof(unsigned), s));
    int next_part = 0;
    if (h->use_split && !h->wg_fork_ops.empty() && !h->side_stream) {
        HIPCK(hipStreamCreateWithFlags(h->side_stream.put(), hipStreamNonBlocking));
        HIPCK(hipEventCreateWithFlags(h->ev_fork.put(), hipEventDisableTiming));
        HIPCK(hipEventCreateWithFlags(h->ev_join.put(), hipEventDisableTiming));
        HIPCK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_wgrad_h), hipFuncAttributeMaxDynamicSharedMemorySize, 65536));
        // (The step's tail runs on the side stream too, behind the early parts.  A separate high-priority stream for it measured 2 %
        // faster in a process of its own and 2.2x SLOWER -- 4.3 ms per step -- as soon as a second handle was alive in the process,
        // bench.py's sampling model: profiles/r04_train_tail_ab.txt.  No stream priorities.)
        for (auto& e : h->ev_tail) HIPCK(hipEventCreateWithFlags(e.put(), hipEventDisableTiming));
    }
    // the G and A operands of a part are final once the backward kernel of its last block is enqueued: its weight gradients run
    // on the side stream from there, beside the remaining chain kernels (one wave per SIMD below 65 536 rows: latency-bound,
    // half the CU idle).  Extra dynamic LDS keeps them to one workgroup per CU so that a chain kernel's workgroup always finds room.
    auto fork_parts = [&](int done_op) -> int {
        while (next_part < (int)h->wg_fork_ops.size() && h->wg_fork_ops[next_part] >= done_op) {
            const int u0 = next_part ? h->wg_part_end[next_part - 1] : 0, u1 = h->wg_part_end[next_part];
            unsigned* gm = h->tr.gmax + (size_t)(1 + next_part) * kMaxGmax;
            HIPCK(hipEventRecord(h->ev_fork, s));
            HIPCK(hipStreamWaitEvent(h->side_stream, h->ev_fork, 0));
            hipLaunchKernelGGL(k_gmax_reduce, dim3(h->n_gmax), dim3(256), 0, h->side_stream, h->tr.gmax_t, h->gmax_ld, gm);
            if (u1 > u0)
                hipLaunchKernelGGL(k_wgrad_h, dim3(u1 - u0), dim3(256), h->wg_early_lds, h->side_stream, h->tr.wg_desc_dev, h->tr.wg_unit_dev + u0,
                                   gm, h->tr.slabs, h->slab_stride, tiles, h->tr_chunks);
            ++next_part;
        }
        return 0;
    };
    for (int oi = (int)h->ops.size() - 1; oi >= 0; --oi) {
        const Op& op = h->ops[oi];
        if (op.kind == OP_PROJ) continue;
        if (op.kind == OP_ATTN) { launch_attn_bwd(h, op, tiles, s); continue; }
        if (h->use_split && h->fbwd_n > 0 && oi == h->fuse_hi - 1) {
            // the narrow run: one launch walks its operators in reverse (k_fused_narrow_bwd_h)
            hipLaunchKernelGGL(k_fused_narrow_bwd_h, dim3(cdiv(tiles, kWavesPerBlock)), dim3(256), 0, s, h->fbwd_dev, h->fbwd_n, tiles);
            oi = h->fuse_lo;
            if (fork_parts(oi)) return 1;
            continue;
        }
        if (op.kind == OP_RES) {
            const ResP& r = h->res[op.p];
            BlockBwdArgs a;
            BlockBwdArgsH ah;
            fill_res_bwd_args(h, op, tiles, a, ah);
            if (h->use_split) {
                if (!launch_res_bwd_h(r.N, r.sclin, ah, s, true))
                    return fail("dsg_train_step: no backward kernel for a %d-wide block with inputs %d + %d wide", r.N, r.in0, r.in1);
                if (fork_parts(oi)) return 1;
            } else {
                launch_res_bwd(r.N, r.sclin, a, s);
            }
        } else {
            const LinOpP& l = h->lin[op.p];
            LinBwdArgs a;
            fill_lin_bwd_args(h, op, tiles, a);
            launch_lin_bwd(l.l.K, op.kind == OP_FINAL, a, s);
        }
    }
    // ---- weight / bias / LayerNorm gradients: grouped launches into per-chunk slabs, then a fixed-order reduce.
    // Small batches: everything in order on the caller's stream.  With the side stream (>= 32 768 rows) the tail runs on two streams:
    //   caller's stream       max|G| of the blocks -> the blocks' units (ONE launch, longest first) -> the Linears' units -> reduce (parameters)
    //   side stream (behind   time-table units -> column sums (k_cs_reduce, k_colsum) -> max|G| of everything --^                ^
    //   the early parts)      -> reduce (dTB) -> time path ----------------------------------------------------------------------+
    // A residual block's G operands have their scale from the block's own backward kernel; only the plain Linears' wait for k_colsum.
    // The time path (UNetCF.py:35-44 backward: ~10 short dependent launches) needs nothing but the dTB rows; its five results go
    // straight into the caller's gradient bucket, and the fixed-order reduce at the end covers every OTHER parameter
    // (k_reduce_ranges: the time_emb weights are ~40 % of the parameters and nothing in the slabs belongs to them).
    mark(2);
    const bool time_beside = h->use_split && next_part > 0 && h->side_stream && h->opt_time_beside;
    hipStream_t cs_stream = time_beside ? h->side_stream : s;
    unsigned* const gm_all = time_beside ? h->tr.gmax + (size_t)(1 + kMaxWgParts) * kMaxGmax : h->tr.gmax;
    auto units = [&](int lo, int hi, const unsigned* gm, hipStream_t us) {
        if (hi > lo)
            hipLaunchKernelGGL(k_wgrad_h, dim3(hi - lo), dim3(256), 0, us, h->tr.wg_desc_dev, h->tr.wg_unit_dev + lo, gm, h->tr.slabs, h->slab_stride,
                               tiles, h->tr_chunks);
    };
    const int u0 = next_part ? h->wg_part_end[next_part - 1] : 0;
    if (time_beside) {
        // the blocks' slots are complete; the Linears' are not yet, and nothing reads them from this set
        hipLaunchKernelGGL(k_gmax_reduce, dim3(h->n_gmax), dim3(256), 0, s, h->tr.gmax_t, h->gmax_ld, h->tr.gmax);
        HIPCK(hipEventRecord(h->ev_tail[0], s));
        HIPCK(hipStreamWaitEvent(h->side_stream, h->ev_tail[0], 0));
        units(u0, h->wg_onehot_end, h->tr.gmax, h->side_stream);
    }
    hipLaunchKernelGGL(k_cs_reduce, dim3(cdiv(h->cs_slots, 256), h->tr_chunks), dim3(256), 0, cs_stream, h->tr.cs, h->tr.cs_map_dev, h->cs_slots,
                       h->tr.slabs, h->slab_stride, tiles, h->tr_chunks);
    hipLaunchKernelGGL(k_colsum, dim3(cdiv(h->cs_units, 4)), dim3(256), 0, cs_stream, h->tr.cs_desc_dev, h->tr.cs_unit_dev, h->cs_units, h->tr.slabs,
                       h->slab_stride, tiles, h->tr_chunks, B, h->tr.gmax_t, h->gmax_ld);
    hipLaunchKernelGGL(k_gmax_reduce, dim3(h->n_gmax), dim3(256), 0, cs_stream, h->tr.gmax_t, h->gmax_ld, gm_all);
    mark(3);
    const size_t dtb0 = (size_t)h->total_params, dtb_n = h->slab_stride - dtb0;
    auto reduce_blocks = [](size_t n) { return dim3((unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096)); };
    auto time_path = [&](float* G, hipStream_t ts) {
        float* emb = h->tr.tsave;
        float* h1pre = emb + (size_t)T * 2 * half;
        float* h1s = h1pre + (size_t)T * td;
        float* tpre = h1s + (size_t)T * td;
        float* d_st = tpre + (size_t)T * td;
        float* d_h1s = d_st + (size_t)T * td;
        float* tpart = d_h1s + (size_t)T * td;   // [kTimeChunks][T][td]
        // all blocks at once: their dTB rows are contiguous from the first block's dtb_off
        const float* dtb_all = h->tr.gsum + h->res[0].dtb_off;
        hipLaunchKernelGGL(k_time_wgrad, dim3(2048), dim3(256), 0, ts, dtb_all, T, h->fw.st, td, h->tw_dst_dev, G, h->tw_rows);
        hipLaunchKernelGGL(k_time_dgrad, dim3(cdiv(T * td, 256), kTimeChunks), dim3(256), 0, ts, dtb_all, T, h->tw_src_dev, td, tpart, h->tw_rows);
        const unsigned eb = (unsigned)cdiv(T * td, 256);
        hipLaunchKernelGGL(k_time_dgrad_finish, dim3(eb), dim3(256), 0, ts, tpart, tpre, d_st, (size_t)T * td);  // d temb (pre-Swish)
        small_gemm(d_st, 1, td, h1s, td, 1, G + P[h->temb_l2w].off, td, 1, td, td, T, 0, ts);                   // d lin2.weight
        hipLaunchKernelGGL(k_col_sum_small, dim3(cdiv(td, 256)), dim3(256), 0, ts, d_st, T, td, (long long)td, G + P[h->temb_l2b].off);
        small_gemm(d_st, td, 1, P[h->temb_l2w].ptr, td, 1, d_h1s, td, 1, T, td, td, 0, ts);                     // d h1 (post-Swish)
        hipLaunchKernelGGL(k_mul_silu_grad, dim3(eb), dim3(256), 0, ts, d_h1s, h1pre, (size_t)T * td);
        small_gemm(d_h1s, 1, td, emb, 2 * half, 1, G + P[h->temb_l1w].off, 2 * half, 1, td, 2 * half, T, 0, ts);  // d lin1.weight
        hipLaunchKernelGGL(k_col_sum_small, dim3(cdiv(td, 256)), dim3(256), 0, ts, d_h1s, T, td, (long long)td, G + P[h->temb_l1b].off);
    };
    if (time_beside) {
        units(h->wg_onehot_end, h->wg_blocks_end, h->tr.gmax, s);
        HIPCK(hipEventRecord(h->ev_tail[2], h->side_stream));              // column sums done: the Linears' scales
        HIPCK(hipStreamWaitEvent(s, h->ev_tail[2], 0));
        units(h->wg_blocks_end, h->wg_units, gm_all, s);
        hipLaunchKernelGGL(k_reduce_slabs, reduce_blocks(dtb_n), dim3(256), 0, h->side_stream, h->tr.slabs + dtb0, h->slab_stride, h->tr_chunks,
                           h->tr.gsum + dtb0, dtb_n);
        time_path(grads_flat, h->side_stream);       // straight into the caller's bucket: the last reduce leaves these regions out
        HIPCK(hipEventRecord(h->ev_tail[1], h->side_stream));
        HIPCK(hipStreamWaitEvent(s, h->ev_tail[1], 0));
        mark(4);
        if (h->r2_vec4 && (reinterpret_cast<unsigned long long>(grads_flat) & 15ull) == 0)
            hipLaunchKernelGGL(k_reduce_ranges4, reduce_blocks((size_t)h->r2_total / 4), dim3(256), 0, s, h->tr.slabs, h->slab_stride, h->tr_chunks,
                               grads_flat, (const long long*)(h->r2_dev + 2 * h->r2_n), (const long long*)(h->r2_dev + 3 * h->r2_n), h->r2_n,
                               h->r2_total / 4);
        else
            hipLaunchKernelGGL(k_reduce_ranges, reduce_blocks((size_t)h->r2_total), dim3(256), 0, s, h->tr.slabs, h->slab_stride, h->tr_chunks,
                               grads_flat, (const long long*)h->r2_dev, (const long long*)(h->r2_dev + h->r2_n), h->r2_n, h->r2_total);
    } else {
        if (h->use_split) {
            if (next_part) HIPCK(hipEventRecord(h->ev_join, h->side_stream));
            units(u0, h->wg_units, h->tr.gmax, s);
            if (next_part) HIPCK(hipStreamWaitEvent(s, h->ev_join, 0));
        } else
            hipLaunchKernelGGL(k_wgrad, dim3(h->wg_units), dim3(256), 0, s, h->tr.wg_desc_dev, h->tr.wg_unit_dev, h->tr.slabs, h->slab_stride, tiles,
                               h->tr_chunks);
        mark(4);
        hipLaunchKernelGGL(k_reduce_slabs, reduce_blocks(h->slab_stride), dim3(256), 0, s, h->tr.slabs, h->slab_stride, h->tr_chunks,
                           h->tr.gsum, h->slab_stride);
        time_path(h->tr.gsum, s);
        HIPCK(hipMemcpyAsync(grads_flat, h->tr.gsum, (size_t)h->total_params * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    mark(5);
    if (h->train_prof) h->tev_valid = true;
    HIPCK(hipGetLastError());
    return 0;
}

}  // namespace
