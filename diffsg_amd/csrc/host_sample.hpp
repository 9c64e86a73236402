// Part of the ONE translation unit dsg_api.hip (included from there, after the kernel headers and `using namespace dsg`): not a
// stand-alone header.  The reverse loop: one step (enqueue_step) and a sampling call with its cached step graphs (sample_impl).
#pragma once

namespace {

// The form of a call's steps, built once by sample_impl: one call or `chunks` independent ones of `chunk_n` elements (0: one call), with
// per-chunk settings (`var`, chunk variants) or without, and the renorm partial sums -- one call: the handle's two partial rows; chunked:
// [chunks][kRedBlocks] twice, one grid row per chunk.  `sched`: the handle holds a guidance schedule (dsg_set_step_guidance): the update
// is the scheduled form, and a step is two-pass or one-pass (StepKind).  `hist`: the handle holds a step history (dsg_set_step_history):
// the update is the history form (dsg_multistep.hpp), never together with `var`.  `clip`: the handle holds an x0 clip (dsg_set_xstart_clip):
// the update is the clip form of whichever of those it would be (dsg_clip.hpp).
struct StepForm { int chunks; size_t chunk_n; bool var; double *p1, *p2; bool sched; bool hist; bool clip; };

// The two contexts of a call: ctx[0] two passes (unconditional tiles first), ctx[1] the one pass of an unguided step, with the resident
// table set of each (dsg_handle::tabs).  Only a call whose schedule has a zero builds and prepares ctx[1].
struct StepCtxs { RunCtx ctx[2]; };

// ev: DSG_SAMPLE_PROFILE's event pairs, or null.  use_hook: take the renorm hook's host callback on this step.  Never while capturing:
// the callback enqueues a real collective (a rank whose graphs are already cached would not issue it: the all-reduces would pair up
// wrongly or hang) and the caller's `renorm_stats` pointer would be baked into the cached graph and outlive the hook.
// one_pass: an unguided step of a scheduled call -- the one-pass context and its table set; the update reads plane 0 of eps alone.
int enqueue_step(dsg_handle* h, const StepCtxs& cs, bool one_pass, const UpdateArgs& u, const StepForm& f, bool renorm, hipStream_t s, const Event* ev,
                 bool use_hook) {
    const RunCtx& c = cs.ctx[one_pass ? 1 : 0];
    if (ev) {
        // DSG_SAMPLE_PROFILE: one event pair per operator.  A launch that covers several operators (the fused narrow run, a pair) is
        // booked on its first operator, the others read ~0.  f32_pairs = false preserves what this loop did before it shared the walk
        // with run_unet: it never tried the exact path's pair kernels (nor the one-launch tile step), so a profile of the exact path
        // times the per-operator launches.  Whether that was meant is not recorded; it is kept, not decided.
        if (walk_ops(h, c, s, /*f32_pairs=*/false,
                     [&](int i) { HIPCK(hipEventRecord(ev[2 * i], s)); return 0; },
                     [&](int i) { HIPCK(hipEventRecord(ev[2 * i + 1], s)); return 0; })) return 1;
    } else {
        run_unet(h, c, s);
    }
    const unsigned ublocks = (unsigned)(((u.n + 3) / 4 + 255) / 256 < 2048 ? ((u.n + 3) / 4 + 255) / 256 : 2048);
    UpdateArgs ua = u;
    ua.record_y = renorm ? 0 : 1;
    const float* const* gpp = h->guid_call;
    const float* const* hpp = h->hist_call;
    const ClipParams* clpp = h->clip_call;
    if (f.clip && f.hist && f.sched) hipLaunchKernelGGL(k_update_clip_hist_sched, dim3(ublocks), dim3(256), 0, s, ua, gpp, h->fw.hist.get(), hpp, clpp);
    else if (f.clip && f.hist) hipLaunchKernelGGL(k_update_clip_hist, dim3(ublocks), dim3(256), 0, s, ua, h->fw.hist.get(), hpp, clpp);
    else if (f.clip && f.var && f.sched) hipLaunchKernelGGL(k_update_clip_var_sched, dim3(ublocks), dim3(256), 0, s, ua, (const VarParams*)h->var_call, gpp, clpp);
    else if (f.clip && f.var) hipLaunchKernelGGL(k_update_clip_var, dim3(ublocks), dim3(256), 0, s, ua, (const VarParams*)h->var_call, clpp);
    else if (f.clip && f.sched) hipLaunchKernelGGL(k_update_clip_sched, dim3(ublocks), dim3(256), 0, s, ua, gpp, clpp);
    else if (f.clip) hipLaunchKernelGGL(k_update_clip, dim3(ublocks), dim3(256), 0, s, ua, clpp);
    else if (f.hist && f.sched) hipLaunchKernelGGL(k_update_hist_sched, dim3(ublocks), dim3(256), 0, s, ua, gpp, h->fw.hist.get(), (const float* const*)h->hist_call);
    else if (f.hist) hipLaunchKernelGGL(k_update_hist, dim3(ublocks), dim3(256), 0, s, ua, h->fw.hist.get(), (const float* const*)h->hist_call);
    else if (f.var && f.sched) hipLaunchKernelGGL(k_update_var_sched, dim3(ublocks), dim3(256), 0, s, ua, (const VarParams*)h->var_call, gpp);
    else if (f.var) hipLaunchKernelGGL(k_update_var, dim3(ublocks), dim3(256), 0, s, ua, (const VarParams*)h->var_call);
    else if (f.sched) hipLaunchKernelGGL(k_update_sched, dim3(ublocks), dim3(256), 0, s, ua, gpp);
    else hipLaunchKernelGGL(k_update, dim3(ublocks), dim3(256), 0, s, ua);
    if (renorm && f.var) {   // chunk variants (never with a hook): every chunk's sums, then the apply of the chunks whose count covers this step
        hipLaunchKernelGGL(k_renorm_sum, dim3(kRedBlocks, f.chunks), dim3(256), 0, s, (const float*)u.y, u.n, f.p1, f.p2, f.chunk_n);
        hipLaunchKernelGGL(k_renorm_apply_var, dim3(kRedBlocks, f.chunks), dim3(256), 0, s, u.y, u.n, (const double*)f.p1, (const double*)f.p2, f.chunk_n,
                           (const CallParams*)u.cp, (const int*)u.step_ptr, (const VarParams*)h->var_call);
    } else if (renorm && h->renorm_fn && use_hook) {
        // sharded call that standardises with the statistics of the WHOLE batch (MSR.py:136-137 on the concatenation of all
        // ranks' rows): local moments -> the caller's all-reduce of 3 doubles (enqueued on this stream) -> apply
        hipLaunchKernelGGL(k_renorm_moments, dim3(kRedBlocks), dim3(256), 0, s, u.y, u.n, h->red, h->red + kRedBlocks);
        hipLaunchKernelGGL(k_renorm_moments_final, dim3(1), dim3(1), 0, s, h->red, h->red + kRedBlocks, u.n, h->renorm_stats);
        h->renorm_fn(h->renorm_user);
        hipLaunchKernelGGL(k_renorm_apply_stats, dim3(kRedBlocks), dim3(256), 0, s, u.y, u.n, h->renorm_stats);
        hipLaunchKernelGGL(k_record, dim3(ublocks), dim3(256), 0, s, u.y, u.n, u.cp, u.step_ptr);
    } else if (renorm) {   // the record is of the renormalised y (MSR.py:136-141): separate launches on these (at most 4) steps
        hipLaunchKernelGGL(k_renorm_sum, dim3(kRedBlocks, f.chunks), dim3(256), 0, s, (const float*)u.y, u.n, f.p1, f.p2, f.chunk_n);
        hipLaunchKernelGGL(k_renorm_apply, dim3(kRedBlocks, f.chunks), dim3(256), 0, s, u.y, u.n, (const double*)f.p1, (const double*)f.p2, f.chunk_n,
                           (const CallParams*)u.cp, (const int*)u.step_ptr);      // + the trajectory record of the renormalised y
    }
    HIPCK(hipGetLastError());
    if (ev) {
        HIPCK(hipStreamSynchronize(s));
        for (size_t i = 0; i < h->ops.size(); ++i) {
            float ms = 0.f;
            HIPCK(hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]));
            h->op_ms[i] += ms;
            h->op_calls[i] += 1;
        }
    }
    return 0;
}

// chunk_rows = 0: one call over B rows.  Otherwise the batch is ceil(B / chunk_rows) independent calls (own seed, own renorm
// statistics), chunk_rows a multiple of 32 so that every chunk starts on a row tile.
int sample_impl(dsg_handle* h, const float* cond, const float* y_T, const float* noise, unsigned long long seed, const unsigned long long* seeds_host,
                int chunk_rows, float omega, const float* coef, int T, float* out, int B, int flags, float* rec_y, float* rec_eps, hipStream_t s) {
    if (check_bound(h)) return 1;
    if (B < 1 || T < 1) return fail("B and T must be >= 1");
    if (!coef || !cond || !out) return fail("dsg_sample: null pointer argument");
    if (h->grid_n && T != h->grid_n) return fail("dsg_sample: the handle's step grid (dsg_set_step_grid) has %d steps, the call has T = %d", h->grid_n, T);
    if (h->guid_n && T != h->guid_n)
        return fail("dsg_sample: the handle's guidance schedule (dsg_set_step_guidance) has %d weights, the call has T = %d", h->guid_n, T);
    if (h->hist_n && T != h->hist_n)
        return fail("dsg_sample: the handle's step history (dsg_set_step_history) has %d rows, the call has T = %d", h->hist_n, T);
    if (h->clip_n && T != h->clip_n)
        return fail("dsg_sample: the handle's x0 clip (dsg_set_xstart_clip) has %d rows, the call has T = %d", h->clip_n, T);
    const bool sched = h->guid_n > 0, hist = h->hist_n > 0, clip = h->clip_n > 0;
    // step k of the call (step index T-1-k) is unguided: one denoiser pass
    auto unguided = [&](int k) { return sched && h->guid_host[(size_t)(T - 1 - k)] == 0.f; };
    bool any_one_pass = false;
    for (int k = 0; k < T && !any_one_pass; ++k) any_one_pass = unguided(k);
    const int chunks = chunk_rows > 0 ? cdiv(B, chunk_rows) : 1;
    if (chunk_rows > 0 && (chunk_rows % 32 != 0)) return fail("dsg_sample_chunked: chunk_rows must be a multiple of 32 (a row tile)");
    if (chunks > 1 && h->renorm_fn) return fail("dsg_sample_chunked: a renorm hook (sharded global renorm) and chunking exclude each other");
    if (chunks > 1 && !seeds_host && !(y_T && (noise || T <= 2))) return fail("dsg_sample_chunked: per-chunk seeds are required");
    // chunk variants (dsg_set_chunk_variants): every check before anything is enqueued or allocated
    const bool var = h->var_chunks > 0;
    const int n_default = h->grid_n ? h->grid_renorm : (T < 4 ? T : 4);  // steps i > T-5 (MSR.py:136), or dsg_set_step_grid's count
    int n_renorm = n_default;
    if (var && hist)
        return fail("dsg_sample_chunked: the handle holds chunk variants (dsg_set_chunk_variants) and a step history (dsg_set_step_history): "
                    "the variant form of the update has no history, remove one of them");
    if (var) {
        if (chunk_rows <= 0)
            return fail("dsg_sample: the handle holds chunk variants (dsg_set_chunk_variants) for %d chunk(s): call dsg_sample_chunked, or remove them", h->var_chunks);
        if (chunks != h->var_chunks)
            return fail("dsg_sample_chunked: the handle holds variants for %d chunk(s) (dsg_set_chunk_variants), the call has %d", h->var_chunks, chunks);
        if (h->renorm_fn) return fail("dsg_sample_chunked: a renorm hook (sharded global renorm) and chunk variants exclude each other");
        if (h->var_has_renorm) {
            n_renorm = 0;
            for (int c = 0; c < chunks; ++c) {
                const int r = h->var_renorm_host[c];
                if (r > T) return fail("dsg_sample_chunked: chunk %d has a renorm count of %d (dsg_set_chunk_variants), the call has T = %d steps", c, r, T);
                if (r > n_renorm) n_renorm = r;
            }
        }
    }
    if (ensure_workspace(h, B, T)) return 1;
    // the history tensor: sized like ywork, on the first call under a history of this workspace (no graph of a history kind exists yet:
    // free_workspace drops tensor and graphs together)
    if (hist && !h->fw.hist) HIPCK(h->fw.hist.alloc((size_t)h->cap_rows * h->d.input_dim));
    const int D = h->d.input_dim, CG = groups_of(h->d.cond_dim), tpp = cdiv(B, 32);
    const size_t n = (size_t)B * D;
    const size_t chunk_n = chunks > 1 ? (size_t)chunk_rows * D : 0;
    if (chunks > 1) {
        if (chunks > h->seeds_cap) {
            HIPCK(hipStreamSynchronize(s));
            HIPCK(h->seeds_dev.alloc((size_t)chunks));
            h->seeds_cap = chunks;
        }
        if (chunks > h->red_chunks_cap) {
            HIPCK(hipStreamSynchronize(s));
            HIPCK(h->red_chunks.alloc((size_t)2 * chunks * kRedBlocks));
            h->red_chunks_cap = chunks;
            free_graphs(h);                        // the captured renorm kernels hold the old buffer
        }
        std::vector<unsigned long long> sd(chunks, 0ull);
        if (seeds_host) sd.assign(seeds_host, seeds_host + chunks);
        HIPCK(hipMemcpyAsync(h->seeds_dev, sd.data(), (size_t)chunks * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
        HIPCK(hipStreamSynchronize(s));            // `sd` is pageable host memory
    }

    // per-call setup: time table for all T steps, condition fragments, start state, step counter
    if (h->grid_n) hipLaunchKernelGGL(k_grid_t, dim3(cdiv(T, 256)), dim3(256), 0, s, h->fw.tvals, (const float*)h->grid_dev, T);
    else hipLaunchKernelGGL(k_linspace_t, dim3(cdiv(T, 256)), dim3(256), 0, s, h->fw.tvals, T);
    run_time_path(h, T, s);
    hipLaunchKernelGGL(k_cond_frag, dim3(cdiv(tpp * CG * 256, 256)), dim3(256), 0, s, cond, (const float*)nullptr, B,
                       h->d.cond_dim, CG, h->fw.condfrag, tpp, h->use_split ? h->range_flag : nullptr, kCondLimit);
    // condition embeddings of every block, once per call: cond is the same in all T steps (MSR.py:126-127)
    run_cond_embed(h, B, s);
    if (y_T) HIPCK(hipMemcpyAsync(h->fw.ywork, y_T, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    else if (chunks > 1) hipLaunchKernelGGL(k_randn_chunked, dim3(2048), dim3(256), 0, s, h->fw.ywork, n, (const unsigned long long*)h->seeds_dev, chunk_n / 4, 0xFFFFFFFFu);
    else hipLaunchKernelGGL(k_randn, dim3(2048), dim3(256), 0, s, h->fw.ywork, n, seed, 0xFFFFFFFFu);
    // step counter (every step's first operator decrements it before anything reads it: step T-1 first) and the call block go
    // to the device as kernel arguments: no pageable copy, no synchronise - consecutive calls pipeline on the stream
    const CallParams cp{noise, coef, omega, T, seed, rec_y, rec_eps, chunk_n / 4, chunks > 1 ? h->seeds_dev : nullptr};
    hipLaunchKernelGGL(k_set_call, dim3(1), dim3(64), 0, s, h->step_dev, h->call_dev.get(), cp, T);
    if (var) {   // with variants `coef` is [tables][T][4] and `omega` is not read
        const VarParams vp{h->var_omega, h->var_has_renorm ? h->var_renorm.get() : nullptr, h->var_has_table ? h->var_table.get() : nullptr, n_default};
        hipLaunchKernelGGL(k_set_var, dim3(1), dim3(64), 0, s, h->var_call.get(), vp);
    }
    if (sched) hipLaunchKernelGGL(k_set_guidance, dim3(1), dim3(64), 0, s, h->guid_call.get(), (const float*)h->guid_dev);
    if (hist) hipLaunchKernelGGL(k_set_guidance, dim3(1), dim3(64), 0, s, h->hist_call.get(), (const float*)h->hist_dev);   // (the same one-word store)
    if (clip) {
        const ClipParams clp{h->clip_bounds.get(), h->clip_bounds.get() + h->d.input_dim, h->clip_rows.get(), h->d.input_dim};
        hipLaunchKernelGGL(k_set_clip, dim3(1), dim3(64), 0, s, h->clip_call.get(), clp);
    }

    StepCtxs cs{{RunCtx{B, 2, tpp, h->fw.ywork, h->fw.eps, h->step_dev, nullptr, false, true},
                 RunCtx{B, 1, 0, h->fw.ywork, h->fw.eps, h->step_dev, nullptr, false, true}}};
    cs.ctx[1].set = 1;
    cs.ctx[0].advance_step = cs.ctx[1].advance_step = h->step_dev;
    cs.ctx[0].share_proj = split_ctx(h, cs.ctx[0]);       // one pass has nobody to share feature_proj with
    if (any_one_pass) {
        // the one-pass context's own resident set: allocated on first use, prepared (and then found current) beside set 0
        dsg_handle::InferTables& t1 = h->tabs[1];
        if (!t1.fusedh_dev) HIPCK(t1.fusedh_dev.alloc(h->ops.size() + 1));
        if (!t1.tileops_dev) HIPCK(t1.tileops_dev.alloc(h->ops.size() + 1));
        if (!t1.fused_dev) HIPCK(t1.fused_dev.alloc(2 * (h->ops.size() + 1)));
        if (prepare_fused(h, cs.ctx[1], s)) return 1;
    }
    if (prepare_fused(h, cs.ctx[0], s)) return 1;
    const StepForm form{chunks, chunk_n, var, chunks > 1 ? h->red_chunks : h->red,
                        chunks > 1 ? h->red_chunks + (size_t)chunks * kRedBlocks : h->red + kRedBlocks, sched, hist, clip};
    UpdateArgs u;
    u.eps = h->fw.eps; u.y = h->fw.ywork; u.cp = h->call_dev; u.step_ptr = h->step_dev; u.n = n; u.record_y = 0;

    if (flags & DSG_SAMPLE_PROFILE) {
        const size_t nops = h->ops.size();
        h->op_ms.assign(nops, 0.0);
        h->op_calls.assign(nops, 0);
        std::vector<Event> ev(2 * nops);
        for (auto& e : ev) HIPCK(hipEventCreate(e.put()));
        for (int k = 0; k < T; ++k)
            if (enqueue_step(h, cs, unguided(k), u, form, k < n_renorm, s, ev.data(), true)) return 1;
    } else if (flags & DSG_SAMPLE_NO_GRAPH) {
        for (int k = 0; k < T; ++k)
            if (enqueue_step(h, cs, unguided(k), u, form, k < n_renorm, s, nullptr, true)) return 1;
    } else {
        // The step index is a device counter and everything per call sits in device memory, so a captured step depends only on
        // the workspace (rows, chunk count) -- not on T, the seed or the schedule.  Captured once per workspace: one early
        // (renorm) step and runs of 1, 2, 4 ... 32 later steps; a call replays min(T, 4) early steps and the binary
        // decomposition of the rest (the shipped T = 20: 4 + one 16-step graph = 5 launches for the whole reverse loop).
        // two sets, one per form of the step (plain / chunk variants), each under its own key: a change of shape drops its own set only
        StepGraphs& G = var ? h->graphs_var : h->graphs;
        if (!(G.rows == B && G.chunks == chunks && G.chunk_rows == chunk_rows)) {
            G.reset();
            G.rows = B; G.chunks = chunks; G.chunk_rows = chunk_rows;
        }
        // Under a guidance schedule the set has three kinds of step (StepKind): the scheduled update with two passes or with one.  The
        // call is cut into runs of equal kind; none of the graphs depends on the weights, only the host's choice among them does.
        // captured lazily: only the run lengths a call replays (a one-off batch size pays for its own decomposition, not for
        // 64 steps of nodes)
        // under a step history the same three with the history form of the update (STEP_HIST ...): the rows {m, p, q} are read on the device
        // under an x0 clip the same six with the clip form of the update (STEP_CLIP ...): bounds and rows are read on the device
        auto kind_of = [&](int k) {
            return (clip ? (int)STEP_CLIP : 0) + (hist ? (int)STEP_HIST : 0) + (!sched ? STEP_PLAIN : unguided(k) ? STEP_ONEPASS : STEP_SCHED);
        };
        auto graph_of = [&](int kind, int variant) -> int {
            GraphExec& ge = G.exec[kind][variant];
            if (ge) return 0;
            const int run = variant == 0 ? 1 : 1 << (variant - 1);
            hipGraph_t g = nullptr;
            HIPCK(hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeThreadLocal));
            int rc = 0;
            for (int k = 0; k < run && !rc; ++k)
                rc = enqueue_step(h, cs, kind % 3 == STEP_ONEPASS, u, form, variant == 0, h->cap_stream, nullptr, /*use_hook=*/false);
            hipError_t e = hipStreamEndCapture(h->cap_stream, &g);
            if (rc) return 1;
            if (e != hipSuccess) return fail("hipStreamEndCapture: %s", hipGetErrorString(e));
            e = hipGraphInstantiate(ge.put(), g, nullptr, nullptr, 0);
            (void)hipGraphDestroy(g);
            if (e != hipSuccess) return fail("hipGraphInstantiate: %s", hipGetErrorString(e));
            return 0;
        };
        for (int k = 0; k < n_renorm; ++k) {
            if (h->renorm_fn) {                           // the hook calls back into the host: these (<= 4) steps run eagerly
                if (enqueue_step(h, cs, unguided(k), u, form, true, s, nullptr, true)) return 1;
            } else {
                const int kind = kind_of(k);
                if (graph_of(kind, 0)) return 1;
                HIPCK(hipGraphLaunch(G.exec[kind][0], s));
            }
        }
        for (int k = n_renorm; k < T;) {
            const int kind = kind_of(k);
            int left = 1;
            while (k + left < T && kind_of(k + left) == kind) ++left;
            k += left;
            while (left > 0) {                      // the binary decomposition of the run
                int v = kStepRunGraphs - 1;
                while ((1 << v) > left) --v;
                if (graph_of(kind, 1 + v)) return 1;
                HIPCK(hipGraphLaunch(G.exec[kind][1 + v], s));
                left -= 1 << v;
            }
        }
    }
    HIPCK(hipMemcpyAsync(out, h->fw.ywork, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}

}  // namespace
