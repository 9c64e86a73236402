// Part of the ONE translation unit dsg_api.hip (included from there, after the kernel headers and `using namespace dsg`): not a
// stand-alone header.  The tables dsg_bind_weights builds when the caller's tensors change: what is packed where.
#pragma once

namespace {

// copy list of the float32 section's image: raw matrices and vectors in the order of V8SecL / V8BlockL (dsg_narrow8.hpp)
int bind_v8_image(dsg_handle* h) {
    const unsigned sec_u4 = (unsigned)(h->d.n_blocks == 3 ? V8SecL<3>::SIZE : V8SecL<2>::SIZE) / 4;
    std::vector<NarrowLdsCopy> cp;
    unsigned used = 0;
    auto take = [&](const void* src, unsigned n_u4) { cp.push_back(NarrowLdsCopy{src, used, n_u4}); used += n_u4; };
    const Param* P = h->params.data();
    const float* A = h->arena;
    const LinOpP& ld = h->lin[h->ops[h->v8_lo].p];
    take(P[ld.l.w].ptr, 32); take(P[ld.l.b].ptr, 2);
    for (int k = h->v8_lo + 1; k + 1 < h->v8_hi; ++k) {
        const ResP& r = h->res[h->ops[k].p];
        const unsigned k1 = r.sclin ? 16 : 8;
        take(P[r.l1.w].ptr, 2 * k1); take(P[r.l2.w].ptr, 16); take(P[r.l3.w].ptr, 16);
        if (r.sclin) take(P[r.sc.w].ptr, 32);
        take(P[r.n1.w].ptr, k1 / 4); take(P[r.n1.b].ptr, k1 / 4);
        take(P[r.n2.w].ptr, 2); take(P[r.n2.b].ptr, 2); take(P[r.n3.w].ptr, 2); take(P[r.n3.b].ptr, 2);
        take(A + r.c2p, 2); take(A + r.c3p, 2);
    }
    const LinOpP& lu = h->lin[h->ops[h->v8_hi - 1].p];
    take(P[lu.l.w].ptr, 32); take(P[lu.l.b].ptr, 4);
    if (used != sec_u4) return fail("internal: float32 section image is %u uint4, expected %u", used, sec_u4);
    if (!h->v8_image) {
        HIPCK(h->v8_image.alloc((size_t)sec_u4 * 4));
        HIPCK(h->v8_copies_dev.alloc(cp.size()));
    }
    HIPCK(hipMemcpy(h->v8_copies_dev, cp.data(), cp.size() * sizeof(NarrowLdsCopy), hipMemcpyHostToDevice));
    h->v8_ncopies = (int)cp.size();
    return 0;
}

// the pack descriptor table: ONE grouped launch (k_pack_grouped) re-packs every tensor into the arena after each optimizer step; and
// the blocks' rows of the time table (k_time_table).  Returns the number of workgroups the table asks for.
long long build_pack_table(dsg_handle* h, std::vector<PackDesc>& pd, std::vector<TimeBlockDesc>& td) {
    const Param* P = h->params.data();
    float* A = h->arena;
    long long blk = 0;
    auto push = [&](int kind, const float* a, const float* b, size_t off, int N, int Ktot, int w0, int w1, int T, long long total) {
        PackDesc d;
        d.a = a; d.b = b; d.dst = A + off; d.kind = kind; d.N = N; d.Ktot = Ktot; d.w0 = w0; d.w1 = w1; d.T = T; d.total = total;
        d.blk_begin = blk;
        blk += (total + kPackPerBlock - 1) / kPackPerBlock;
        pd.push_back(d);
    };
    auto pack = [&](const LinearP& l, int w0, int w1, size_t off) {
        const int NT = cdiv(l.N, 32);
        push(0, P[l.w].ptr, nullptr, off, l.N, l.K, w0, w1, NT, (long long)NT * (groups_of(w0) + groups_of(w1)) * 256);
    };
    auto packT = [&](const LinearP& l, int w0, int w1, size_t off) {
        const int OT = cdiv(groups_of(w0) + groups_of(w1), 4);
        push(1, P[l.w].ptr, nullptr, off, l.N, l.K, w0, w1, OT, (long long)OT * groups_of(l.N) * 256);
    };
    auto padv = [&](const float* a, const float* b, int w0, int w1, size_t off, int npad) { push(2, a, b, off, 0, 0, w0, w1, 0, npad); };
    td.resize(h->res.size());
    for (size_t i = 0; i < h->res.size(); ++i) {
        const ResP& r = h->res[i];
        const int NT = cdiv(r.N, 32), KG = groups_of(r.in0) + groups_of(r.in1);
        pack(r.l1, r.in0, r.in1, r.W1p);
        padv(P[r.n1.w].ptr, nullptr, r.in0, r.in1, r.g1p, KG * 8 + 32);
        padv(P[r.n1.b].ptr, nullptr, r.in0, r.in1, r.b1p, KG * 8 + 32);
        pack(r.l2, r.N, 0, r.W2p);
        padv(P[r.n2.w].ptr, nullptr, r.N, 0, r.g2p, NT * 32);
        padv(P[r.n2.b].ptr, nullptr, r.N, 0, r.b2p, NT * 32);
        padv(P[r.l2.b].ptr, P[r.ce.b].ptr, r.N, 0, r.c2p, NT * 32);
        pack(r.ce, h->d.cond_dim, 0, r.Wcp);
        pack(r.l3, r.N, 0, r.W3p);
        padv(P[r.n3.w].ptr, nullptr, r.N, 0, r.g3p, NT * 32);
        padv(P[r.n3.b].ptr, nullptr, r.N, 0, r.b3p, NT * 32);
        padv(P[r.l3.b].ptr, r.sclin ? P[r.sc.b].ptr : nullptr, r.N, 0, r.c3p, NT * 32);
        if (r.sclin) { pack(r.sc, r.in0, r.in1, r.Wscp); packT(r.sc, r.in0, r.in1, r.WscT); }
        packT(r.l1, r.in0, r.in1, r.W1T);
        packT(r.l2, r.N, 0, r.W2T);
        packT(r.l3, r.N, 0, r.W3T);
        td[i] = TimeBlockDesc{P[r.te.w].ptr, P[r.te.b].ptr, P[r.l1.b].ptr, r.N, r.tb_off};
    }
    for (const LinOpP& l : h->lin) {
        const int NT = cdiv(l.l.N, 32), KG = groups_of(l.l.K);
        pack(l.l, l.l.K, 0, l.Wp);
        packT(l.l, l.l.K, 0, l.WT);
        padv(P[l.l.b].ptr, nullptr, l.l.N, 0, l.bp, NT * 32);
        if (l.lnact) {
            padv(P[l.ln.w].ptr, nullptr, l.l.K, 0, l.gp, KG * 8 + 32);
            padv(P[l.ln.b].ptr, nullptr, l.l.K, 0, l.betap, KG * 8 + 32);
        }
    }
    for (const AttnP& t : h->attn) {
        const int NT = cdiv(t.N, 32), NG = groups_of(t.N);
        const long long d = t.N, tot = (long long)NT * NG * 256;
        const float* Wv = P[t.proj.w].ptr + 2 * d * d;
        push(0, Wv, nullptr, t.Wvp, t.N, t.N, t.N, 0, NT, tot);
        push(1, Wv, nullptr, t.WvT, t.N, t.N, t.N, 0, NT, tot);
        padv(P[t.proj.b].ptr + 2 * d, nullptr, t.N, 0, t.bvp, NT * 32);
        pack(t.out, t.N, 0, t.Wop);
        packT(t.out, t.N, 0, t.WoT);
        padv(P[t.out.b].ptr, nullptr, t.N, 0, t.bop, NT * 32);
    }
    return blk;
}

// fp16-split planes (k_pack_h) and the max|W| words they are scaled by (k_maxabs): descriptor tables, uploaded synchronously
int build_plane_tables(dsg_handle* h) {
    const Param* P = h->params.data();
    float* A = h->arena;
    std::vector<const float*> mp; std::vector<long long> mn; std::vector<PackHDesc> hd;
    h->mx_param.clear();
    long long hb = 0;
    auto want = [&](const LinearP& l) {
        for (size_t i = 0; i < h->mx_param.size(); ++i) if (h->mx_param[i] == l.w) return;
        h->mx_param.push_back(l.w); mp.push_back(P[l.w].ptr); mn.push_back(P[l.w].numel);
    };
    // planes of W (transposed = 0: NT = out tiles, steps over the inputs) or of W^T (data gradients: NT = tiles of the inputs, steps over N)
    auto push_planes = [&](int transposed, const LinearP& l, const LinearP* pair, int role, int w0, int w1, size_t off) {
        PackHDesc d;
        const int NT = transposed ? cdiv(groups_of(w0) + groups_of(w1), 4) : cdiv(l.N, 32);
        const int KS = transposed ? (groups_of(l.N) + 1) / 2 : (groups_of(w0) + 1) / 2 + (groups_of(w1) + 1) / 2;
        d.W = P[l.w].ptr; d.dst = reinterpret_cast<uint4*>(A + off); d.m_self = h->maxabs + l.w; d.m_pair = pair ? h->maxabs + pair->w : nullptr;
        d.role = role; d.N = l.N; d.Ktot = l.K; d.w0 = w0; d.w1 = w1; d.NT = NT; d.total = (long long)NT * KS * 128; d.blk_begin = hb;
        d.transposed = transposed;
        hb += (d.total + 255) / 256;
        hd.push_back(d);
    };
    auto pushh = [&](const LinearP& l, const LinearP* pair, int role, int w0, int w1, size_t off) { push_planes(0, l, pair, role, w0, w1, off); };
    auto pushhT = [&](const LinearP& l, const LinearP* pair, int role, int w0, int w1, size_t off) { push_planes(1, l, pair, role, w0, w1, off); };
    for (const ResP& r : h->res) {
        if (!r.split) continue;
        want(r.l1); want(r.l2); want(r.l3); want(r.ce);
        pushh(r.ce, nullptr, 0, h->d.cond_dim, 0, r.Wch);
        if (r.sclin) want(r.sc);
        pushh(r.l1, nullptr, 0, r.in0, r.in1, r.W1h);
        pushh(r.l2, nullptr, 0, r.N, 0, r.W2h);
        if (r.sclin) { pushh(r.l3, &r.sc, 1, r.N, 0, r.W3h); pushh(r.sc, &r.l3, 2, r.in0, r.in1, r.Wsch); }
        else pushh(r.l3, nullptr, 0, r.N, 0, r.W3h);
        pushhT(r.l1, nullptr, 0, r.in0, r.in1, r.W1Th);
        pushhT(r.l2, nullptr, 0, r.N, 0, r.W2Th);
        if (r.sclin) { pushhT(r.l3, &r.sc, 1, r.N, 0, r.W3Th); pushhT(r.sc, &r.l3, 2, r.in0, r.in1, r.WscTh); }
        else pushhT(r.l3, nullptr, 0, r.N, 0, r.W3Th);
    }
    for (const LinOpP& l : h->lin) { want(l.l); pushh(l.l, nullptr, 0, l.l.K, 0, l.Wh); }
    for (const AttnP& t : h->attn) {
        if (t.N < 64) continue;
        // Wv = rows 2d:3d of projection.weight, scaled by max| | of the WHOLE tensor (the word k_attn_h reads): one [d][d] matrix
        want(t.proj); want(t.out);
        LinearP lo = t.out;
        pushh(lo, nullptr, 0, t.N, 0, t.Woh);
        pushh(lo, nullptr, 0, t.N, 0, t.Wvh);
        PackHDesc& dv = hd.back();
        dv.W = P[t.proj.w].ptr + 2 * (size_t)t.N * t.N; dv.m_self = h->maxabs + t.proj.w;
    }
    // the weight-side envelope (dsg_split.hpp, EnvDesc): every Linear listed above, and every LayerNorm that feeds a split product --
    // their max|gamma| and max|beta| are two more words of the same k_maxabs launch.  Conservative in one place: the 8-wide blocks are
    // listed too, although with DSG_OPT_NARROW_VALU8 on they run in exact float32 on the vector unit -- a large gamma there alone sends
    // the model to the exact path without need (the option can be switched off at any time, the word is per bind).  Not covered: k_maxabs
    // reduces with fmaxf, which drops a NaN, so a NaN gamma or weight does not raise the word (the outputs are NaN on either path).
    std::vector<EnvDesc> env;
    for (int w : h->mx_param) env.push_back(EnvDesc{w, -1, 0.f});
    auto want_norm = [&](const NormP& n) {
        if (n.w < 0 || n.b < 0) return;
        for (int p : {n.w, n.b}) { h->mx_param.push_back(p); mp.push_back(P[p].ptr); mn.push_back(P[p].numel); }
        env.push_back(EnvDesc{n.w, n.b, sqrtf((float)P[n.w].numel)});
    };
    for (const ResP& r : h->res) { want_norm(r.n1); want_norm(r.n2); want_norm(r.n3); }
    for (const LinOpP& l : h->lin) if (l.lnact) want_norm(l.ln);
    h->env_n = (int)env.size();
    h->mx_n = (int)mp.size(); h->packh_n = (int)hd.size(); h->packh_blocks = hb;
    if (h->mx_n) {
        if (!h->env_dev) HIPCK(h->env_dev.alloc(env.size()));
        HIPCK(hipMemcpy(h->env_dev, env.data(), env.size() * sizeof(EnvDesc), hipMemcpyHostToDevice));
        if (!h->mx_ptrs_dev) {
            HIPCK(h->mx_ptrs_dev.alloc(mp.size()));
            HIPCK(h->mx_numel_dev.alloc(mn.size()));
            HIPCK(h->packh_dev.alloc(hd.size()));
            HIPCK(h->mx_idx_dev.alloc(mp.size()));
        }
        HIPCK(hipMemcpy(h->mx_idx_dev, h->mx_param.data(), mp.size() * sizeof(int), hipMemcpyHostToDevice));
        HIPCK(hipMemcpy(h->mx_ptrs_dev, mp.data(), mp.size() * sizeof(float*), hipMemcpyHostToDevice));
        HIPCK(hipMemcpy(h->mx_numel_dev, mn.data(), mn.size() * sizeof(long long), hipMemcpyHostToDevice));
        HIPCK(hipMemcpy(h->packh_dev, hd.data(), hd.size() * sizeof(PackHDesc), hipMemcpyHostToDevice));
    }

    return 0;
}

// time_emb.weight row tables (training time-path backward)
int build_time_rows(dsg_handle* h) {
    const Param* P = h->params.data();
    std::vector<long long> dst; std::vector<const float*> src;
    for (const ResP& r : h->res)
        for (int n = 0; n < r.N; ++n) { dst.push_back(P[r.te.w].off + (long long)n * h->td); src.push_back(P[r.te.w].ptr + (size_t)n * h->td); }
    h->tw_rows = (int)dst.size();
    if (!h->tw_dst_dev) {
        HIPCK(h->tw_dst_dev.alloc(dst.size()));
        HIPCK(h->tw_src_dev.alloc(src.size()));
    }
    HIPCK(hipMemcpy(h->tw_dst_dev, dst.data(), dst.size() * sizeof(long long), hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(h->tw_src_dev, src.data(), src.size() * sizeof(float*), hipMemcpyHostToDevice));

    return 0;
}

}  // namespace
