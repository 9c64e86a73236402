// Repeated sampling: of n candidate rows per condition keep the best one, on the device ("Best of n").
//
// Y[n][B][D] holds n rounds of raw sampler output, round-major.  Every round is decoded as the problem's decoder decodes a
// [B][D] tensor (MSR / NU: min-max over THAT round) and scored with the problem's objective; per condition the round with the
// strictly best finite objective wins, the lowest round on equal objectives.  One statistics pass (per-round min / max), then
// one selection launch that reads Y once, keeps the running best row in registers and writes the winner once: decoded
// candidates never reach memory, there are no atomics, and every store is a plain vector store.
//
// The per-round values are the ones dsg_*_decode / dsg_msr_rate / dsg_co_cost / dsg_nu_rate return, bit for bit: the row
// bodies are the __device__ functions of dsg_eval.hpp, a row sits in the lanes exactly as in k_row_softmax, and the MSR
// rate is summed in k_msr_rate's order for that D (see k_best_msr).
#pragma once
#include "dsg_eval.hpp"

namespace dsg {

// A decoded value as the two-call path sees it: rounded to float32 and opaque to the optimiser, so that no multiply of the
// decoder contracts into an add of the evaluator (the separate kernels cannot fuse across memory either).
__device__ __forceinline__ float as_stored(float x) {
    asm volatile("" : "+v"(x));
    return x;
}

// per-round (min, max) over columns [c0, c1): k_minmax_partial / k_minmax_final with the round on the grid's y / x axis.
// part[n][nparts], mm[n].  Min and max are exact in any order, so mm[r] is minmax_global's pair of round r.
__global__ __launch_bounds__(256) void k_best_minmax_partial(const float* __restrict__ y, int n, long long rows, int D, int c0, int c1,
                                                             float2* __restrict__ part) {
    __shared__ float smin[4], smax[4];
    const int lane = threadIdx.x & 63;
    const int w = c1 - c0;
    const int lpr = w >= 64 ? 64 : (w >= 16 ? 16 : (w >= 4 ? 4 : 1)), rpw = 64 / lpr;
    const int sub = lane & (lpr - 1), rsub = lane / lpr;
    for (int k = blockIdx.y; k < n; k += gridDim.y) {
        const float* yk = y + (long long)k * rows * D;
        float lo = INFINITY, hi = -INFINITY;
        for (long long r = (blockIdx.x * 4LL + (threadIdx.x >> 6)) * rpw + rsub; r < rows; r += (long long)gridDim.x * 4 * rpw)
            for (int c = c0 + sub; c < c1; c += lpr) {
                const float v = yk[r * D + c];
                lo = fminf(lo, v); hi = fmaxf(hi, v);
            }
        lo = wave_min_f(lo); hi = wave_max_f(hi);
        __syncthreads();                              // the previous round's partial has been read
        if (lane == 0) { smin[threadIdx.x >> 6] = lo; smax[threadIdx.x >> 6] = hi; }
        __syncthreads();
        if (threadIdx.x == 0)
            part[(long long)k * gridDim.x + blockIdx.x] =
                make_float2(fminf(fminf(smin[0], smin[1]), fminf(smin[2], smin[3])), fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3])));
    }
}
__global__ __launch_bounds__(256) void k_best_minmax_final(const float2* __restrict__ part, int n, int nparts, float2* __restrict__ mm) {
    __shared__ float smin[4], smax[4];
    for (int k = blockIdx.x; k < n; k += gridDim.x) {
        float lo = INFINITY, hi = -INFINITY;
        for (int i = threadIdx.x; i < nparts; i += 256) { const float2 p = part[(long long)k * nparts + i]; lo = fminf(lo, p.x); hi = fmaxf(hi, p.y); }
        lo = wave_min_f(lo); hi = wave_max_f(hi);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) { smin[threadIdx.x >> 6] = lo; smax[threadIdx.x >> 6] = hi; }
        __syncthreads();
        if (threadIdx.x == 0)
            mm[k] = make_float2(fminf(fminf(smin[0], smin[1]), fminf(smin[2], smin[3])), fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3])));
    }
}

// Candidate (o, round) against the running best (bobj, bidx): a non-finite objective never wins, any finite one replaces
// "none yet" (bidx < 0), otherwise only a strictly better one does -- so equal objectives keep the lower round.
template <bool MAXIMISE>
__device__ __forceinline__ bool best_wins(float o, float bobj, int bidx) {
    return isfinite(o) && (bidx < 0 || (MAXIMISE ? o > bobj : o < bobj));
}

// MSR: solution = W * msr_decode(Y[r]) row, objective = msr_rate(solution, gains), maximised.
// L lanes hold a row as k_row_softmax<1, L> does (column sub + k * L in slot k).  k_msr_rate sums the row with R = L * Q lanes
// (1 up to D = 8, 16 up to 160, 64 above): lane i adds columns i, i + R, ... in turn, then an xor butterfly over the R lanes.
// Here virtual lane i = sub + L * q lives in slot q of real lane sub: its columns are the slots k = q, q + Q, ... (same
// order), the butterfly's steps >= L pair slots q and q ^ h inside the lane, the steps below L are the real shuffles.
template <int L, int Q>
__global__ __launch_bounds__(256) void k_best_msr(const float* __restrict__ Y, const float* __restrict__ G, int n, long long B, int D, float W,
                                                  const float2* __restrict__ mm, float* __restrict__ sol, float* __restrict__ obj,
                                                  int* __restrict__ rnd, float* __restrict__ objs, int accumulate, int round0) {
    constexpr int RPW = 64 / L;
    const int lane = threadIdx.x & 63, sub = lane % L;
    const long long b = (blockIdx.x * 4LL + (threadIdx.x >> 6)) * RPW + lane / L;
    const bool live = b < B;
    const long long bb = live ? b : 0;               // idle lanes shadow row 0: they take part in the shuffles, never store
    float g[kSoftEpl], best[kSoftEpl];
#pragma unroll
    for (int k = 0; k < kSoftEpl; ++k) {
        const int c = sub + k * L;
        g[k] = c < D ? G[bb * D + c] : 0.f;
        best[k] = 0.f;
    }
    float bobj = 0.f;
    int bidx = -1;
    bool changed = !accumulate;
    if (accumulate) { bobj = obj[bb]; bidx = rnd[bb]; }
    for (int r = 0; r < n; ++r) {
        const float2 m2 = mm[r];
        float v[kSoftEpl];
        bool dead;
        const float s = softmax_row_regs<1, L>(Y + ((long long)r * B + bb) * D, sub, D, m2.x, m2.y - m2.x, v, dead);
        float part[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) part[q] = 0.f;
#pragma unroll
        for (int k = 0; k < kSoftEpl; ++k) {
            v[k] = as_stored(W * as_stored(v[k] / s));
            if (sub + k * L < D) part[k % Q] += msr_term(v[k], g[k]);
        }
#pragma unroll
        for (int h = Q / 2; h > 0; h >>= 1)
#pragma unroll
            for (int q = 0; q < h; ++q) part[q] += part[q + h];
        const float o = group_sum<L>(part[0]);
        if (objs && live && sub == 0) objs[(long long)r * B + b] = o;
        if ((r == 0 && !accumulate) || best_wins<true>(o, bobj, bidx)) {
#pragma unroll
            for (int k = 0; k < kSoftEpl; ++k) best[k] = v[k];
            bobj = o;
            if (isfinite(o)) bidx = round0 + r;
            changed = true;
        }
    }
    if (live && changed) {
#pragma unroll
        for (int k = 0; k < kSoftEpl; ++k) {
            const int c = sub + k * L;
            if (c < D) sol[b * D + c] = best[k];
        }
        if (sub == 0) { obj[b] = bobj; rnd[b] = bidx; }
    }
}

// CO: solution = co_decode(Y[r]) row, objective = co_cost(X, solution), minimised.  One thread per row, as k_co_cost and
// k_row_softmax<2, 1> (D <= kSoftEpl nodes).
__global__ __launch_bounds__(256) void k_best_co(const float* __restrict__ Y, const float* __restrict__ X, int n, long long B, int D,
                                                 float* __restrict__ sol, float* __restrict__ obj, int* __restrict__ rnd,
                                                 float* __restrict__ objs, int accumulate, int round0) {
    const long long b = blockIdx.x * 256LL + threadIdx.x;
    if (b >= B) return;
    const float* x = X + b * 3 * D;
    float best[kSoftEpl];
#pragma unroll
    for (int k = 0; k < kSoftEpl; ++k) best[k] = 0.f;
    float bobj = 0.f;
    int bidx = -1;
    bool changed = !accumulate;
    if (accumulate) { bobj = obj[b]; bidx = rnd[b]; }
    for (int r = 0; r < n; ++r) {
        float v[kSoftEpl], yd[kSoftEpl];
        bool dead;
        const float s = softmax_row_regs<2, 1>(Y + ((long long)r * B + b) * D, 0, D, 0.f, 1.f, v, dead);
#pragma unroll
        for (int k = 0; k < kSoftEpl; ++k) yd[k] = as_stored(dead ? 0.f : v[k] / s);
        const float o = co_cost_row(x, yd, D);
        if (objs) objs[(long long)r * B + b] = o;
        if ((r == 0 && !accumulate) || best_wins<false>(o, bobj, bidx)) {
#pragma unroll
            for (int k = 0; k < kSoftEpl; ++k) best[k] = yd[k];
            bobj = o;
            if (isfinite(o)) bidx = round0 + r;
            changed = true;
        }
    }
    if (changed) {
#pragma unroll
        for (int k = 0; k < kSoftEpl; ++k)
            if (k < D) sol[b * D + k] = best[k];
        obj[b] = bobj;
        rnd[b] = bidx;
    }
}

// NU: solution = nu_decode(Y[r]) row (position min-max over round r), objective = nu_rate(solution, X), maximised.
// One thread per row, as k_nu_decode and k_nu_rate (K = D - 2 <= kNuMaxUsers).
__global__ __launch_bounds__(256) void k_best_nu(const float* __restrict__ Y, const float* __restrict__ X, int n, long long B, int D,
                                                 float width, float height, float p_sum, const float2* __restrict__ mm,
                                                 float* __restrict__ sol, float* __restrict__ obj, int* __restrict__ rnd,
                                                 float* __restrict__ objs, int accumulate, int round0) {
    const long long b = blockIdx.x * 256LL + threadIdx.x;
    if (b >= B) return;
    const float* x = X + b * 2 * (D - 2);
    float best[kNuMaxUsers + 2];
    float bobj = 0.f;
    int bidx = -1;
    bool changed = !accumulate;
    if (accumulate) { bobj = obj[b]; bidx = rnd[b]; }
    for (int r = 0; r < n; ++r) {
        float yd[kNuMaxUsers + 2];
        nu_decode_row(Y + ((long long)r * B + b) * D, yd, D, width, height, p_sum, mm[r]);
        for (int c = 0; c < D; ++c) yd[c] = as_stored(yd[c]);
        const float o = nu_rate_row(yd, x, D - 2);
        if (objs) objs[(long long)r * B + b] = o;
        if ((r == 0 && !accumulate) || best_wins<true>(o, bobj, bidx)) {
            for (int c = 0; c < D; ++c) best[c] = yd[c];
            bobj = o;
            if (isfinite(o)) bidx = round0 + r;
            changed = true;
        }
    }
    if (changed) {
        for (int c = 0; c < D; ++c) sol[b * D + c] = best[c];
        obj[b] = bobj;
        rnd[b] = bidx;
    }
}

}  // namespace dsg
