// Part of the ONE translation unit dsg_api.hip (included from there, after the kernel headers and `using namespace dsg`): not a
// stand-alone header.  Forward tables and plans: the tables prepare_fused uploads (singles, narrow run, whole-net tile table, LDS image plan), the time path, the condition embeddings.
#pragma once

namespace {

// ---- forward tables and plans: one function per table, prepare_fused is the driver ------------------------------------------------

// Is the table on the device already the one of this context?  Stores the new key when it is not.
// training forward: split path only; the table depends on the workspaces and the batch, not on the step -> cached.
// inference: same context as the table already on the device (consecutive dsg_sample calls of one batch size): nothing to do - and
// no stream synchronise between calls, so the host can enqueue the next call while this one runs
int fused_tables_current(dsg_handle* h, const RunCtx& c, bool sp, bool& current) {
    current = true;
    if (c.train) {
        if (!sp) return 0;
        const void* key[4] = {h->fw.ws, h->tr.ws, h->fw.cembed, h->fw.tb};
        if (h->fusedh_train_dev && h->fusedh_train_rows == c.nrows && !memcmp(key, h->fusedh_train_key, sizeof key)) return 0;
        if (!h->fusedh_train_dev) HIPCK(h->fusedh_train_dev.alloc(h->ops.size() + 1));
        ++h->generation;      // the training table of the narrow run is rewritten in place for this batch size (dsg_generation)
        memcpy(h->fusedh_train_key, key, sizeof key);
        h->fusedh_train_rows = c.nrows;
    } else {
        dsg_handle::FusedSig sig;
        sig.valid = true; sig.sp = sp; sig.share = c.share_proj; sig.nrows = c.nrows; sig.npass = c.npass; sig.uncond_tiles = c.uncond_tiles;
        const void* ptrs[8] = {c.y, c.eps_out, c.step_ptr, c.ts, h->fw.ws, h->fw.cembed, h->fw.tb,
                               reinterpret_cast<const void*>((size_t)h->cap_rows * 2 + (c.cond_pre ? 1 : 0))};
        memcpy(sig.p, ptrs, sizeof ptrs);
        const dsg_handle::FusedSig& o = h->tabs[c.set].fused_sig;
        if (o.valid && o.sp == sig.sp && o.share == sig.share && o.nrows == sig.nrows && o.npass == sig.npass && o.uncond_tiles == sig.uncond_tiles &&
            !memcmp(o.p, sig.p, sizeof sig.p))
            return 0;
        h->tabs[c.set].fused_sig = sig;
    }
    current = false;
    return 0;
}

// exact path: every narrow operator as a chain of ONE, in the second half of fused_host (launch_op, narrow_singles)
void build_singles_table(dsg_handle* h, const RunCtx& c) {
    const size_t nops = h->ops.size();
    h->tabs[c.set].fused_host.assign(2 * (nops + 1), FusedOp{});
    for (size_t k = 0; k < nops; ++k) {
        const Op& op = h->ops[k];
        if (!fusable(h, op)) continue;
        FusedOp& f = h->tabs[c.set].fused_host[nops + 1 + k];
        memset(&f, 0, sizeof f);
        f.kind = op.kind == OP_RES ? 0 : 1;
        f.N = f.kind == 0 ? h->res[op.p].N : h->lin[op.p].l.N;
        f.sclin = f.kind == 0 ? (int)h->res[op.p].sclin : 0;
        if (f.kind == 0) fill_block_args(h, op, c, f.b); else fill_lin_args(h, op, c, f.l);
        f.pad = 2 | 1;             // a chain of one: input into registers, output stored
    }
}

// the narrow run's table in the layout of the context (FusedOpH: split path, FusedOp: exact path) and, split sampling only, the tail
// entry behind it; returns whether there is a tail
bool build_narrow_table(dsg_handle* h, const RunCtx& c, bool sp, int n) {
    for (int i = 0; i < n; ++i) {
        const Op& op = h->ops[h->fuse_lo + i];
        BlockArgs b; LinArgs l;
        memset(&b, 0, sizeof b); memset(&l, 0, sizeof l);
        const int kind = op.kind == OP_RES ? 0 : 1;
        const int N = kind == 0 ? h->res[op.p].N : h->lin[op.p].l.N;
        const int sclin = kind == 0 ? (int)h->res[op.p].sclin : 0;
        if (kind == 0) fill_block_args(h, op, c, b); else fill_lin_args(h, op, c, l);
        if (sp) {
            FusedOpH& f = h->tabs[c.set].fusedh_host[i];
            memset(&f, 0, sizeof f);
            f.kind = kind; f.N = N; f.sclin = sclin;
            f.store_out = (c.train || h->tensors[op.out].is_skip || i == n - 1) ? 1 : 0;   // training: the backward reads every tensor
            if (kind == 0) fill_block_args_h(h, h->res[op.p], b, f.b); else fill_lin_args_h(h, h->lin[op.p], l, f.l);
        } else {
            FusedOp& f = h->tabs[c.set].fused_host[i];
            memset(&f, 0, sizeof f);
            f.kind = kind; f.N = N; f.sclin = sclin; f.b = b; f.l = l;
            // a link of the chain (bit 1): input handed over in registers; stored (bit 0) if something else reads it from memory
            f.pad = 2 | ((h->tensors[op.out].is_skip || i == n - 1) ? 1 : 0);
        }
    }
    // the Linear behind the run (Upsample 32 -> 64 of the shipped nets): the LDS form of the run computes it from the registers of
    // the run's last tensor (one launch and one round trip of that tensor less); entry n of the table, read by that form only
    if (!(sp && !c.train && !c.ts && h->fuse_hi < (int)h->ops.size())) return false;
    const Op& t = h->ops[h->fuse_hi];
    const Op& last = h->ops[h->fuse_hi - 1];
    if (!(t.kind == OP_LIN && t.in0 == last.out && !h->tensors[last.out].is_skip && !h->lin[t.p].lnact && h->lin[t.p].l.N == 64 && h->lin[t.p].l.K <= 32))
        return false;
    LinArgs l;
    memset(&l, 0, sizeof l);
    fill_lin_args(h, t, c, l);
    h->tabs[c.set].fusedh_host.resize(n + 1);
    FusedOpH& f = h->tabs[c.set].fusedh_host[n];
    memset(&f, 0, sizeof f);
    f.kind = 2; f.N = 64; f.store_out = 1;
    fill_lin_args_h(h, h->lin[t.p], l, f.l);
    return true;
}

// the whole net's table for k_unet_tile: the run's entries as in the narrow table, every other operator stored (its consumer reads
// memory); sets tile_valid and uploads the table when the net has the shapes the kernel covers
int build_tile_table(dsg_handle* h, const RunCtx& c, hipStream_t s) {
    const int nops = (int)h->ops.size();
    h->tabs[c.set].tileops_host.assign(nops, FusedOpH{});
    bool ok = nops >= 2 && h->ops[0].kind == OP_PROJ && h->fuse_lo >= 1;
    int wide = 0;
    for (int i = 0; i < nops && ok; ++i) {
        const Op& op = h->ops[i];
        FusedOpH& f = h->tabs[c.set].tileops_host[i];
        memset(&f, 0, sizeof f);
        if (i >= h->fuse_lo && i < h->fuse_hi) { f = h->tabs[c.set].fusedh_host[i - h->fuse_lo]; continue; }
        f.store_out = 1;
        if (op.kind == OP_ATTN) { ok = false; break; }      // k_unet_tile has not learned the operator: per-operator launches
        if (op.kind == OP_RES) {
            const ResP& r = h->res[op.p];
            BlockArgs b;
            fill_block_args(h, op, c, b);
            f.kind = 0; f.N = r.N; f.sclin = r.sclin ? 1 : 0;
            fill_block_args_h(h, r, b, f.b);
            if (!(coop_fits(r) && b.cond_pre)) ok = false;     // the kernel runs every wide block through the cooperative body
            ++wide;
        } else {
            const LinOpP& l = h->lin[op.p];
            LinArgs la;
            fill_lin_args(h, op, c, la);
            f.kind = op.kind == OP_FINAL ? 3 : 1; f.N = l.l.N;
            fill_lin_args_h(h, l, la, f.l);
            if (op.kind == OP_PROJ) f.kind = 1;            // never executed by the kernel (its range starts behind feature_proj)
            else if (l.l.N > 128 || (op.kind == OP_FINAL) != l.lnact) ok = false;
        }
    }
    h->tabs[c.set].tile_valid = ok && wide > 0;
    if (h->tabs[c.set].tile_valid)
        HIPCK(hipMemcpyAsync(h->tabs[c.set].tileops_dev, h->tabs[c.set].tileops_host.data(), (size_t)nops * sizeof(FusedOpH), hipMemcpyHostToDevice, s));
    return 0;
}

// LDS image of the run, cut into phases that fit kNarrowLdsU4: per operator its packed planes and per-feature vectors (static:
// gathered once into tb.nlds_image, a phase's part contiguous) and, behind them, the phase's slice of the time-table row
struct NarrowLdsPlan {
    dsg_handle* h;
    dsg_handle::InferTables& tb;                // the table set of the context the plan is made for
    int n, n_all;                               // operators of the run; with the tail Linear when it joined the last phase
    std::vector<NarrowLdsOp> lops;
    std::vector<NarrowLdsCopy> copies;          // dst_u4: offset in the GLOBAL image buffer
    std::vector<unsigned> phase_base{0u};
    unsigned used = 0, image_base = 0;          // used: static part of the current phase
    int phase_lo = 0;
    int tb_first = -1, tb_last_end = 0;         // time-table slice of the current phase (floats in the row)
    // the float32 section (ops [s_lo, s_hi) of the run): one unit of the plan, placed at its first operator
    int s_lo, s_hi;
    unsigned s_u4, s_tb_u4;

    NarrowLdsPlan(dsg_handle* h_, dsg_handle::InferTables& tb_, int n_) : h(h_), tb(tb_), n(n_), n_all(n_), lops(n_ + 1) {
        s_lo = (h->opt_v8 && h->v8_lo >= 0) ? h->v8_lo - h->fuse_lo : -1; s_hi = s_lo >= 0 ? h->v8_hi - h->fuse_lo : -1;
        const int s_nb = h->d.n_blocks;
        s_u4 = (unsigned)(s_nb == 3 ? V8SecL<3>::SIZE : V8SecL<2>::SIZE) / 4; s_tb_u4 = (unsigned)(2 * s_nb + 3) * 8;
    }
    unsigned take(const void* src, unsigned n_u4) {
        const unsigned off = used;
        copies.push_back(NarrowLdsCopy{src, image_base + off, n_u4});
        used += n_u4;
        return off;
    }
    unsigned tb_now() const { return tb_first < 0 ? 0 : (unsigned)(tb_last_end - tb_first) / 4; }
    // a phase's time-bias slices must be one contiguous piece of the row
    bool take_tb(const ResP& r) {
        if (tb_first < 0) tb_first = r.tb_off;
        else if (r.tb_off != tb_last_end) return false;
        tb_last_end = r.tb_off + pad32(r.N);
        return true;
    }
    void close_phase(int hi) {
        NarrowPhaseArgs ph;
        ph.image = nullptr; ph.n_u4 = used; ph.tb = h->fw.tb + (tb_first < 0 ? 0 : tb_first); ph.tb_u4 = tb_now();
        ph.op_lo = phase_lo; ph.op_hi = hi;
        ph.v8_at = -1; ph.v8_nops = 0; ph.v8_store = 0; ph.v8_sec = 0; ph.v8_tb = 0;
        if (s_lo >= phase_lo && s_lo < hi) {       // the float32 section lies in this phase (its image offset was noted when it was taken)
            ph.v8_at = s_lo; ph.v8_nops = s_hi - s_lo; ph.v8_sec = 4 * lops[s_lo].w1; ph.v8_store = lops[s_lo].store_out;
            ph.v8_tb = 4 * used + (unsigned)(h->res[h->ops[h->fuse_lo + s_lo + 1].p].tb_off - tb_first);
        }
        tb.nlds_phases.push_back(ph);              // the image pointer is filled by upload() (it needs the buffer): phase_base remembers where
        for (int k = phase_lo; k < hi; ++k) {      // the time-bias rows sit behind the static part
            const Op& o = h->ops[h->fuse_lo + k];
            if (o.kind == OP_RES) lops[k].tb = 4 * used + (unsigned)(h->res[o.p].tb_off - tb_first);
        }
        image_base += used;
    }
    bool place_op(int i);       // operator i of the run into the current phase, or a new one; false: the run does not fit
    void place_tail();
    int upload(hipStream_t s);
};

bool NarrowLdsPlan::place_op(int i) {
    const Op& op = h->ops[h->fuse_lo + i];
    const float* A = h->arena;
    if (s_lo >= 0 && i > s_lo && i < s_hi) return true;      // inside the section: planned with its first operator (its entry stays zero)
    const ResP* r = (i != s_lo && op.kind == OP_RES) ? &h->res[op.p] : nullptr;
    const LinOpP* l = (i != s_lo && op.kind != OP_RES) ? &h->lin[op.p] : nullptr;
    const unsigned KG = r ? groups_of(r->in0) + groups_of(r->in1) : 0, KS1 = r ? (groups_of(r->in0) + 1) / 2 + (groups_of(r->in1) + 1) / 2 : 0;
    const unsigned KS2 = r ? (groups_of(r->N) + 1) / 2 : 0, nv1 = (KG * 8 + 32 + 3) / 4, KSl = l ? (groups_of(l->l.K) + 1) / 2 : 0;
    unsigned need = KSl * 128 + 8, need_tb = 0;
    if (i == s_lo) { need = s_u4; need_tb = s_tb_u4; }
    else if (r) { need = KS1 * 128 * (r->sclin ? 2 : 1) + 2 * KS2 * 128 + 2 * nv1 + 6 * 8; need_tb = 8; }
    if (need + need_tb > (unsigned)kNarrowLdsU4) return false;
    if (used + need + tb_now() + need_tb > (unsigned)kNarrowLdsU4) {
        close_phase(i);
        // (round 6: one launch walks every phase, the running tensor crosses the boundary in registers)
        if ((int)tb.nlds_phases.size() >= kNarrowMaxPhases) return false;
        phase_base.push_back(image_base);
        phase_lo = i; used = 0; tb_first = -1; tb_last_end = 0;
    }
    NarrowLdsOp& lo = lops[i];
    lo.store_out = tb.fusedh_host[(s_lo >= 0 && i == s_lo) ? s_hi - 1 : i].store_out;
    if (i == s_lo) {
        // the section's image as one piece (gathered at bind time into h->v8_image, dsg_bind_weights)
        lo.w1 = take(h->v8_image, s_u4);
        for (int k = s_lo + 1; k + 1 < s_hi; ++k)
            if (!take_tb(h->res[h->ops[h->fuse_lo + k].p])) return false;
    } else if (r) {
        lo.w1 = take(A + r->W1h, KS1 * 128);
        lo.w2 = take(A + r->W2h, KS2 * 128);
        lo.w3 = take(A + r->W3h, KS2 * 128);
        lo.wsc = r->sclin ? take(A + r->Wsch, KS1 * 128) : lo.w1;
        lo.g1 = 4 * take(A + r->g1p, nv1); lo.b1 = 4 * take(A + r->b1p, nv1);
        lo.g2 = 4 * take(A + r->g2p, 8); lo.b2 = 4 * take(A + r->b2p, 8);
        lo.g3 = 4 * take(A + r->g3p, 8); lo.b3 = 4 * take(A + r->b3p, 8);
        lo.c2 = 4 * take(A + r->c2p, 8); lo.c3 = 4 * take(A + r->c3p, 8);
        if (!take_tb(*r)) return false;
    } else {
        lo.w1 = take(A + l->Wh, KSl * 128);
        lo.c2 = 4 * take(A + l->bp, 8);
    }
    return true;
}

// the tail Linear's planes (2 out tiles x 2 steps) and bias join the last phase when they fit
void NarrowLdsPlan::place_tail() {
    const LinOpP& l = h->lin[h->ops[h->fuse_hi].p];
    const unsigned KSl = (groups_of(l.l.K) + 1) / 2, need = 2 * KSl * 128 + 16;
    if (used + need + tb_now() > (unsigned)kNarrowLdsU4) return;
    NarrowLdsOp& lo = lops[n];
    lo.store_out = 1;
    lo.w1 = take(h->arena + l.Wh, 2 * KSl * 128);
    lo.c2 = 4 * take(h->arena + l.bp, 16);
    n_all = n + 1;
    if (phase_lo < n) lops[n - 1].store_out = 0;      // the run's last tensor stays in registers: only the tail reads it
}

int NarrowLdsPlan::upload(hipStream_t s) {
    const size_t image_u4 = image_base;
    if (!tb.nlds_ops_dev) HIPCK(tb.nlds_ops_dev.alloc(h->ops.size() + 1));
    if (!tb.nlds_copies_dev) HIPCK(tb.nlds_copies_dev.alloc((h->ops.size() + 1) * 16));
    if (image_u4 + 1 > tb.nlds_image_cap) {
        // grow-only: the captured step graphs hold the image pointer (phase arguments are passed by value); when it has
        // to move, every graph captured with the old one goes (nothing is in flight: the stream was synchronised by the driver)
        if (tb.nlds_image) { tb.nlds_image.reset(); free_graphs(h); }
        HIPCK(tb.nlds_image.alloc(image_u4 + 1));
        tb.nlds_image_cap = image_u4 + 1;
    }
    HIPCK(hipMemcpy(tb.nlds_ops_dev, lops.data(), n_all * sizeof(NarrowLdsOp), hipMemcpyHostToDevice));
    tb.nlds_tail = n_all > n;
    HIPCK(hipMemcpy(tb.nlds_copies_dev, copies.data(), copies.size() * sizeof(NarrowLdsCopy), hipMemcpyHostToDevice));
    for (size_t k = 0; k < tb.nlds_phases.size(); ++k) tb.nlds_phases[k].image = tb.nlds_image + phase_base[k];
    hipLaunchKernelGGL(k_narrow_image_build, dim3((unsigned)copies.size()), dim3(256), 0, s, (const NarrowLdsCopy*)tb.nlds_copies_dev, tb.nlds_image);
    tb.nlds_ncopies = (int)copies.size();
    tb.nlds_valid = true;
    return 0;
}

int build_lds_plan(dsg_handle* h, dsg_handle::InferTables& tb, int n, bool tail, hipStream_t s) {
    NarrowLdsPlan plan(h, tb, n);
    tb.nlds_phases.clear();
    for (int i = 0; i < n; ++i)
        if (!plan.place_op(i)) return 0;              // does not fit: nlds_valid stays false, the run takes its other forms
    if (n <= 0) return 0;
    if (tail) plan.place_tail();
    plan.close_phase(plan.n_all);
    return plan.upload(s);
}

// Upload the operator descriptors of the fused narrow run for this context (stream ordered; replayed graphs read them).
int prepare_fused(dsg_handle* h, const RunCtx& c, hipStream_t s) {
    const int n = h->fuse_hi - h->fuse_lo;
    const bool singles = narrow_singles(h, c);
    if (n < 2 && !singles) return 0;
    const bool sp = split_ctx(h, c);
    bool current = false;
    if (fused_tables_current(h, c, sp, current)) return 1;
    if (current) return 0;
    HIPCK(hipStreamSynchronize(s));  // the host tables may still be the source of an earlier async copy
    if (sp) h->tabs[c.set].fusedh_host.resize(n); else h->tabs[c.set].fused_host.resize(n);
    if (singles) build_singles_table(h, c);
    const bool tail = build_narrow_table(h, c, sp, n);
    if (sp) HIPCK(hipMemcpyAsync(c.train ? h->fusedh_train_dev : h->tabs[c.set].fusedh_dev, h->tabs[c.set].fusedh_host.data(), h->tabs[c.set].fusedh_host.size() * sizeof(FusedOpH), hipMemcpyHostToDevice, s));
    else HIPCK(hipMemcpyAsync(h->tabs[c.set].fused_dev, h->tabs[c.set].fused_host.data(), (singles ? h->tabs[c.set].fused_host.size() : (size_t)n) * sizeof(FusedOp), hipMemcpyHostToDevice, s));
    if (sp && !c.train && build_tile_table(h, c, s)) return 1;
    // the training forward has its own table and leaves the inference plan (and fused_sig) alone: resetting the LDS plan here
    // would drop the eager sampling path to the non-LDS kernels for good while cached graphs keep replaying the LDS form
    if (!c.train) { h->tabs[c.set].nlds_valid = false; h->tabs[c.set].nlds_tail = false; }
    if (sp && !c.train && !c.ts) return build_lds_plan(h, h->tabs[c.set], n, tail, s);
    return 0;
}

// time path for `entries` t values already in h->fw.tvals (saves for the backward when `train`)
void run_time_path(dsg_handle* h, int entries, hipStream_t s, bool train = false) {
    const int half = h->d.proj_dim / 2, td = h->td;
    const Param* P = h->params.data();
    float *emb = nullptr, *h1pre = nullptr, *tpre = nullptr;
    float* h1s = h->fw.h1s;
    if (train) {
        emb = h->tr.tsave; h1pre = emb + (size_t)h->tr_T * 2 * half; h1s = h1pre + (size_t)h->tr_T * td;
        tpre = h1s + (size_t)h->tr_T * td;
    }
    const dim3 grid(entries, cdiv(td, 16));
    hipLaunchKernelGGL(k_time_embed1, grid, dim3(256), 2 * half * sizeof(float), s, h->fw.tvals, h->freq, half, P[h->temb_l1w].ptr,
                       P[h->temb_l1b].ptr, td, h1s, emb, h1pre);
    hipLaunchKernelGGL(k_time_embed2, grid, dim3(256), td * sizeof(float), s, h1s, P[h->temb_l2w].ptr, P[h->temb_l2b].ptr, td, h->fw.st, tpre);
    const int nb = (int)h->res.size();
    hipLaunchKernelGGL(k_time_table, dim3(entries, nb * 8), dim3(256), td * sizeof(float), s, h->fw.st, td, h->tdesc_dev, nb, h->fw.tb, h->tb_stride);
}

// cembed[block] = Wc silu(cond * mask) for every block from the condition fragments (one launch per block)
void run_cond_embed(dsg_handle* h, int B, hipStream_t s) {
    const int tpp = cdiv(B, 32), CG = groups_of(h->d.cond_dim);
    if (h->use_split && (CG + 1) / 2 <= kCondMaxSteps) {
        // split path: every block in ONE launch
        if (h->ctile_key != h->fw.cembed || h->ctile_cap != cap_tiles_of(h)) {
            std::vector<CondTile> tab;
            for (const ResP& r : h->res) {
                const int NG = groups_of(r.N);
                for (int lt = 0; lt < cdiv(r.N, 32); ++lt) {
                    CondTile t;
                    t.out = h->fw.cembed + r.ce_off * (cap_tiles_of(h) / 2) + (size_t)lt * 4 * 256;
                    t.m = h->maxabs + r.ce.w;
                    t.groups = NG - 4 * lt < 4 ? NG - 4 * lt : 4;
                    t.ng_block = NG;
                    tab.push_back(t);
                }
            }
            if (!h->ctile_dev) (void)h->ctile_dev.alloc(tab.size());
            (void)hipMemcpy(h->ctile_dev, tab.data(), tab.size() * sizeof(CondTile), hipMemcpyHostToDevice);
            h->ctile_n = (int)tab.size(); h->ctile_key = h->fw.cembed; h->ctile_cap = cap_tiles_of(h);
        }
        // enough waves for ~2 per SIMD: row tiles x parts
        const int parts = tpp >= 2048 ? 1 : (tpp >= 1024 ? 2 : (tpp >= 512 ? 4 : 8));
        hipLaunchKernelGGL(k_cond_embed_h, dim3(cdiv(tpp, kWavesPerBlock), parts), dim3(256), 0, s, h->fw.condfrag, CG,
                           reinterpret_cast<const uint4*>(h->arena + h->res[0].Wch), h->ctile_dev, h->ctile_n, tpp);
        return;
    }
    // wide blocks: one launch each; all blocks <= 32 wide: ONE launch (a wave walks the list for its tile)
    std::vector<FusedOp>& tab = h->ce_host;
    tab.clear();
    for (const ResP& r : h->res) {
        LinArgs a;
        memset(&a, 0, sizeof a);
        a.in.data = h->fw.condfrag; a.in.groups = CG; a.in.width = h->d.cond_dim;
        a.in_width = h->d.cond_dim; a.in_groups = CG;
        a.W = h->arena + r.Wcp; a.bias = h->arena + h->zero_off;
        a.out = h->fw.cembed + r.ce_off * (cap_tiles_of(h) / 2); a.out_stats = h->fw.ce_stats; a.out_width = r.N;
        a.ntiles = tpp; a.tiles_per_pass = tpp; a.nrows = B;
        if (r.N > 32) { launch_lin(r.N, IN_FRAG, OUT_FRAG, false, a, s); continue; }
        FusedOp f;
        memset(&f, 0, sizeof f);
        f.kind = 1; f.N = r.N; f.l = a;
        tab.push_back(f);
    }
    if (!tab.empty()) {
        (void)hipStreamSynchronize(s);  // ce_host may still be the source of the previous upload
        (void)hipMemcpyAsync(h->ce_dev, tab.data(), tab.size() * sizeof(FusedOp), hipMemcpyHostToDevice, s);
        hipLaunchKernelGGL(k_fused_narrow, dim3(cdiv(tpp, kWavesPerBlock)), dim3(256), 0, s, h->ce_dev, (int)tab.size(), tpp);
    }
}

}  // namespace
