// Part of the ONE translation unit dsg_api.hip (included from there, after the kernel headers and `using namespace dsg`): not a
// stand-alone header.  The evaluators' and the baselines' side: argument checks, LDS plans and the launch helper of the entry points outside the UNet.
#pragma once

namespace {

// ---- decoders / evaluators (dsg_eval.hpp)
int eval_args(const void* a, const void* b, long long rows, int D, const char* who) {
    if (!a || !b || rows < 0 || D < 1) return fail("%s: bad arguments", who);
    return 0;
}
// part[0] <- (min, max) of columns [c0, c1) of the whole tensor; stream-ordered scratch, released when the caller's `part` goes out of
// scope, behind its consumer
int minmax_global(const float* y, long long rows, int D, int c0, int c1, StreamScratch<float2>& part, hipStream_t s) {
    const int w = c1 - c0, lpr = w >= 64 ? 64 : (w >= 16 ? 16 : (w >= 4 ? 4 : 1));
    const long long want = (rows + 4LL * (64 / lpr) - 1) / (4LL * (64 / lpr));   // one trip of k_minmax_partial per block if it fits
    const int nparts = (int)(want < kEvalParts ? want : kEvalParts);
    HIPCK(part.alloc((size_t)1 + nparts, s));
    hipLaunchKernelGGL(k_minmax_partial, dim3(nparts), dim3(256), 0, s, y, rows, D, c0, c1, part.get());
    hipLaunchKernelGGL(k_minmax_final, dim3(1), dim3(256), 0, s, part.get(), nparts);
    return 0;
}
template <int MODE>
int softmax_rows(const float* y, float* out, long long rows, int D, hipStream_t s, int c0, int c1) {
    if (rows == 0) return 0;
    StreamScratch<float2> scratch;
    if (MODE == 1 && minmax_global(y, rows, D, c0, c1, scratch, s)) return 1;
    const float2* part = scratch;
    auto blocks = [&](int lpr) { const long long rpb = 4LL * (64 / lpr); return dim3((unsigned)((rows + rpb - 1) / rpb)); };
    if (D <= kSoftEpl) hipLaunchKernelGGL((k_row_softmax<MODE, 1>), blocks(1), dim3(256), 0, s, y, out, rows, D, part);
    else if (D <= 4 * kSoftEpl) hipLaunchKernelGGL((k_row_softmax<MODE, 4>), blocks(4), dim3(256), 0, s, y, out, rows, D, part);
    else if (D <= 16 * kSoftEpl) hipLaunchKernelGGL((k_row_softmax<MODE, 16>), blocks(16), dim3(256), 0, s, y, out, rows, D, part);
    else if (D <= 64 * kSoftEpl) hipLaunchKernelGGL((k_row_softmax<MODE, 64>), blocks(64), dim3(256), 0, s, y, out, rows, D, part);
    else hipLaunchKernelGGL((k_row_softmax_wide<MODE>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, y, out, rows, D, part);
    HIPCK(hipGetLastError());
    return 0;
}

// ---- the small-net baselines: MTFNN (dsg_mlp.hpp) and PPO (dsg_ppo.hpp)
// One net's part of a plan, from its widths w[0 .. L]: the weight / bias offsets in the flat vector from *off on, and from activation
// a0 on the odd row strides and the offsets within ONE tile row from *row on (plan_tile scales them by the tile height).
void net_layout(int L, const int* w, int* woff, int* boff, int a0, int* aoff, int* astr, int* off, int* row) {
    for (int l = 0; l < L; ++l) {
        woff[l] = *off; *off += w[l + 1] * w[l];
        boff[l] = *off; *off += w[l + 1];
    }
    for (int l = a0; l <= L; ++l) { astr[l] = w[l] | 1; aoff[l] = *row; *row += astr[l]; }
}
// Completes a plan whose P, strides and per-row offsets are in, for `scal` scalar slots and tile rows of `row` floats.  The tile height
// is 64 rows, or 32 or 16 where the slots, the parameters and the tile exceed the LDS (false: 16 rows do too); gradient and both Adam
// moments go behind the tile when the call is an epoch and they fit.  Both depend on the descriptor alone, so that the loss_grad and
// the train_epoch call of a baseline sum a batch's rows in the same order.
template <typename Plan>
bool plan_tile(Plan* p, int scal, int row, bool epoch) {
    int TR = 64;
    while (TR > 16 && scal + p->P + TR * row > kMlpLdsFloats) TR >>= 1;
    if (scal + p->P + TR * row > kMlpLdsFloats) return false;
    p->TR = TR;
    p->tr_shift = TR == 64 ? 6 : (TR == 32 ? 5 : 4);
    int* aoff = reinterpret_cast<int*>(p->aoff);        // one net's offsets, or both nets' (the unused entries are zero)
    for (size_t i = 0; i < sizeof p->aoff / sizeof(int); ++i) aoff[i] *= TR;
    p->yoff *= TR;
    p->act_floats = TR * row;
    p->lds_floats = scal + p->P + p->act_floats;
    p->onchip = epoch && p->lds_floats + 3 * p->P <= kMlpLdsFloats;
    if (p->onchip) p->lds_floats += 3 * p->P;
    return true;
}
// Validates the descriptor and lays the workgroup's LDS out: scalar slots | parameters | tile area (activations of every layer, targets)
// [| gradient | exp_avg | exp_avg_sq].
int mlp_plan(const dsg_mlp_desc* d, MlpPlan* p, bool epoch, const char* who) {
    if (!d) return fail("%s: null descriptor", who);
    const int L = d->n_layers;
    if (L < 2 || L > kMlpMaxLayers) return fail("%s: %d Linear layers (2 .. %d)", who, L, kMlpMaxLayers);
    for (int l = 0; l <= L; ++l) {
        const int lim = (l == 0 || l == L) ? kMlpMaxIO : kMlpMaxHidden;
        if (d->widths[l] < 1 || d->widths[l] > lim)
            return fail("%s: widths[%d] = %d (%s width 1 .. %d)", who, l, d->widths[l], (l == 0 || l == L) ? "input / output" : "hidden", lim);
    }
    if (d->n_sig < 0 || d->n_sig > d->widths[L]) return fail("%s: n_sig = %d with %d output columns", who, d->n_sig, d->widths[L]);
    memset(p, 0, sizeof *p);
    p->L = L;
    p->n_sig = d->n_sig;
    for (int l = 0; l <= L; ++l) p->w[l] = d->widths[l];
    int row = 0;
    net_layout(L, p->w, p->woff, p->boff, 0, p->aoff, p->astr, &p->P, &row);
    p->yoff = row; p->ystr = p->w[L] | 1; row += p->ystr;      // the targets
    if (!plan_tile(p, kMlpScal, row, epoch)) return fail("%s: the net does not fit in LDS", who);     // not reachable within the width limits
    return 0;
}
// Validates the descriptor and lays the workgroup's LDS out: scalar slots | parameters | tile area (the state tile, every layer's
// activations of both nets, the targets) [| gradient | exp_avg | exp_avg_sq].
int ppo_plan(const dsg_ppo_desc* d, PpoPlan* p, bool epoch, const char* who, bool need_env = true) {
    if (!d) return fail("%s: null descriptor", who);
    if (d->state_dim < 1 || d->state_dim > kMlpMaxIO) return fail("%s: state_dim = %d (1 .. %d)", who, d->state_dim, kMlpMaxIO);
    if (d->action_dim < 1 || d->action_dim > kMlpMaxIO) return fail("%s: action_dim = %d (1 .. %d)", who, d->action_dim, kMlpMaxIO);
    for (int l = 0; l < 3; ++l)
        if (d->hidden[l] < 1 || d->hidden[l] > kMlpMaxHidden) return fail("%s: hidden[%d] = %d (1 .. %d)", who, l, d->hidden[l], kMlpMaxHidden);
    const int S = d->state_dim, A = d->action_dim;
    switch (d->env) {
        case kPpoCO: if (S != 3 * A) return fail("%s: CO wants state_dim = 3 * action_dim, got %d and %d", who, S, A); break;
        case kPpoMSR: if (S != A) return fail("%s: MSR wants state_dim = action_dim, got %d and %d", who, S, A); break;
        case kPpoNU:
            if (A < 3 || A - 2 > kNuMaxUsers || S != 2 * (A - 2))
                return fail("%s: NU wants action_dim = K + 2, state_dim = 2 K with 1 <= K <= %d, got %d and %d", who, kNuMaxUsers, A, S);
            break;
        case DSG_PPO_NONE: if (need_env) return fail("%s: env = DSG_PPO_NONE; the call needs an environment (0 CO, 1 MSR, 2 NU)", who); break;
        default: return fail("%s: env = %d (0 CO, 1 MSR, 2 NU)", who, d->env);
    }
    memset(p, 0, sizeof *p);
    p->S = S; p->A = A; p->env = d->env;
    p->lo = (float)d->scaler_min; p->span = (float)(d->scaler_max - d->scaler_min); p->W = (float)d->W;
    p->width = (float)d->width; p->height = (float)d->height; p->p_sum = (float)d->P_sum;
    p->P = A;                                           // log_std[A] leads the flat vector
    int row = S | 1;                                    // the state tile, at offset 0, is activation 0 of both nets
    for (int n = 0; n < 2; ++n) {
        p->w[n][0] = S; p->w[n][1] = d->hidden[0]; p->w[n][2] = d->hidden[1]; p->w[n][3] = d->hidden[2]; p->w[n][4] = n == 0 ? 1 : A;
        p->astr[n][0] = S | 1;
        net_layout(4, p->w[n], p->woff[n], p->boff[n], 1, p->aoff[n], p->astr[n], &p->P, &row);
    }
    p->yoff = row; p->ystr = A | 1; row += p->ystr;     // the targets
    if (!plan_tile(p, kPpoScal, row, epoch)) return fail("%s: the two nets (%d parameters) do not fit in LDS", who, p->P);
    return 0;
}
// The batch buffer ([rows][2A + 2]) goes behind everything else in LDS where it fits (its offset), else into a workspace (-1).
int ppo_buf_off(const PpoPlan& p, long long rows) {
    return p.lds_floats + rows * (2 * p.A + 2) <= kMlpLdsFloats ? p.lds_floats : -1;
}
// What the two epoch entry points check alike; cols: the widest row the kernel indexes with an int.
int epoch_args(const char* who, int N, int batch, int R, long long step0, int cols) {
    if (N < 0 || batch < 1 || R < 1 || step0 < 0) return fail("%s: N = %d, batch = %d, R = %d, step0 = %lld", who, N, batch, R, step0);
    if (N > 2147483647 / cols) return fail("%s: N = %d rows (at most %d)", who, N, 2147483647 / cols);
    return 0;
}
// One launch of a baseline kernel: `grid` workgroups of kMlpThreads with `bytes` of dynamic LDS (above 64 KiB the kernel's limit is
// raised first).  The stream-ordered scratch the launch reads is released behind it; the launch error is reported before a release error.
template <typename K, typename... Args>
int baseline_launch(K kernel, long long grid, int bytes, hipStream_t s, std::initializer_list<StreamScratch<float>*> scratch, Args... args) {
    if (bytes > 65536) HIPCK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kMlpThreads), bytes, s, args...);
    hipError_t err = hipGetLastError();
    for (StreamScratch<float>* ws : scratch) {
        const hipError_t freed = ws->release();
        if (err == hipSuccess) err = freed;
    }
    HIPCK(err);
    return 0;
}

}  // namespace
