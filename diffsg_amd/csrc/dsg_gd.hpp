// The gradient-descent baseline (reference: baselines/GD.py) on the device, float64 like the reference's numpy.
//
// One launch runs ALL `iters` iterations of a row: the row's condition and its state are loaded once into registers, the
// iterations run there, and the state is written once.  Nothing touches global memory in between but the optional record
// (rec [k][B][D]: the state after iterations rec_every, 2 * rec_every, ...).  No LDS, no atomics, no scratch: every register
// array below is indexed by unrolled loop counters only, and sizes that are not known at compile time are handled by
// wave-uniform `if (i < n)` around whole slots.
//
// Arithmetic: contraction is off inside every function, each expression keeps the reference's left-to-right order, division
// is the IEEE one and `** 2` is x * x as in numpy.  There are no clamps: a zero allocation gives the inf / NaN numpy gives.
// The CO iteration is chaotic, so the order is what keeps a row on the reference's own branch.
//
//   k_gd_co  <NMAX>   one row per lane, n <= NMAX nodes         (GD.py:12-36)
//   k_gd_msr <LPR>    one row per LPR lanes, 8 slots per lane   (GD.py:62-83); the row sum is a butterfly over the group
//   k_gd_nu  <KMAX>   one row per lane, K <= KMAX users         (GD.py:100-117, written there for K = 3)
#pragma once
#include <hip/hip_runtime.h>

namespace dsg {

constexpr int kGdThreads = 256;
constexpr int kGdCoMaxNodes = 16;     // dsg_best_of's limit for CO
constexpr int kGdMsrMax = 128;        // the widest input_dim of the package
constexpr int kGdNuMaxUsers = 32;     // dsg_nu_rate's limit
constexpr int kGdMsrSlots = 8;        // state entries per lane in k_gd_msr
constexpr int kGdMsrLanes = 16;       // lanes per row in the wide variant: 16 * 8 = 128
constexpr double kGdLn2 = 0.6931471805599453;   // np.log(2)

// Where the state goes after iteration `it` (1-based) if it is a recorded one, else nullptr.  rec [k][B][D].
struct GdRec {
    double* rec;
    int every;
    __device__ __forceinline__ double* slot(int it, long long B, int D, long long row) const {
        if (!rec || it % every != 0) return nullptr;
        return rec + ((long long)(it / every - 1) * B + row) * D;
    }
};

// ---- CO: x [B][3n] = (local cost, transition cost, execution cost) per node, y [B][2n] = decisions | allocations
template <int NMAX>
__global__ __launch_bounds__(kGdThreads) void k_gd_co(const double* __restrict__ X, double* __restrict__ Y, long long B, int n, int iters,
                                                      double lr, double lambda1, double lambda2, GdRec rec) {
#pragma clang fp contract(off)
    const long long row = (long long)blockIdx.x * kGdThreads + threadIdx.x;
    if (row >= B) return;
    const double* x = X + row * 3 * n;
    double* y = Y + row * 2 * n;
    double xl[NMAX], xt[NMAX], xe[NMAX], dec[NMAX], al[NMAX];
#pragma unroll
    for (int i = 0; i < NMAX; ++i)
        if (i < n) {
            xl[i] = x[3 * i]; xt[i] = x[3 * i + 1]; xe[i] = x[3 * i + 2];
            dec[i] = y[i]; al[i] = y[n + i];
        }
    for (int it = 1; it <= iters; ++it) {
        double S = 0.0;     // the allocations of the state BEFORE this update, left to right
#pragma unroll
        for (int i = 0; i < NMAX; ++i)
            if (i < n) S = i == 0 ? al[0] : S + al[i];
        const double pen = (S * 2 - 1) * lambda2;
#pragma unroll
        for (int i = 0; i < NMAX; ++i)
            if (i < n) {
                const double gd = -xl[i] + xt[i] + xe[i] / al[i] + (1 - 2 * dec[i]) * lambda1;
                const double ga = -xe[i] / (al[i] * al[i]) * dec[i] + pen;
                dec[i] = dec[i] - gd * lr;
                al[i] = al[i] - ga * lr;
            }
        if (double* r = rec.slot(it, B, 2 * n, row)) {
#pragma unroll
            for (int i = 0; i < NMAX; ++i)
                if (i < n) { r[i] = dec[i]; r[n + i] = al[i]; }
        }
    }
    if (iters > 0) {
#pragma unroll
        for (int i = 0; i < NMAX; ++i)
            if (i < n) { y[i] = dec[i]; y[n + i] = al[i]; }
    }
}

// ---- MSR: x [B][M] = channel gains, y [B][M] = the allocation.  Entry j of a row lives in lane j % LPR of the row's group, slot
// j / LPR; slots past the row's end are skipped whole (wave-uniform), the ragged last slot is masked per lane.  Lanes of rows past
// B run along on zeros (the group's shuffles need every lane) and store nothing.
template <int LPR>
__global__ __launch_bounds__(kGdThreads) void k_gd_msr(const double* __restrict__ X, double* __restrict__ Y, long long B, int M, int iters,
                                                       double lr, GdRec rec) {
#pragma clang fp contract(off)
    const long long t = (long long)blockIdx.x * kGdThreads + threadIdx.x;
    const long long row = t / LPR;
    const int sub = (int)(t % LPR);
    const bool live = row < B;
    const double* x = X + row * M;
    double* y = Y + row * M;
    double gs[kGdMsrSlots], s[kGdMsrSlots];
#pragma unroll
    for (int e = 0; e < kGdMsrSlots; ++e) {
        const int j = e * LPR + sub;
        const bool has = live && j < M;
        gs[e] = has ? x[j] : 0.0;
        s[e] = has ? y[j] : 0.0;
    }
    for (int it = 1; it <= iters; ++it) {
        double sum = 0.0;
#pragma unroll
        for (int e = 0; e < kGdMsrSlots; ++e)
            if (e * LPR < M) sum = e == 0 ? s[0] : sum + s[e];       // masked entries are 0.0
#pragma unroll
        for (int m = 1; m < LPR; m <<= 1) sum = sum + __shfl_xor(sum, m, LPR);
        const double pen = 1.0 / ((sum - 1) * (sum - 1));
#pragma unroll
        for (int e = 0; e < kGdMsrSlots; ++e)
            if (e * LPR < M) {
                const double g = gs[e] / ((gs[e] * s[e] + 1.0) * kGdLn2) - pen;
                s[e] = e * LPR + sub < M ? s[e] + g * lr : 0.0;
            }
        if (double* r = live ? rec.slot(it, B, M, row) : nullptr) {
#pragma unroll
            for (int e = 0; e < kGdMsrSlots; ++e)
                if (e * LPR + sub < M) r[e * LPR + sub] = s[e];
        }
    }
    if (live && iters > 0) {
#pragma unroll
        for (int e = 0; e < kGdMsrSlots; ++e)
            if (e * LPR + sub < M) y[e * LPR + sub] = s[e];
    }
}

// ---- NU: x [B][2K] = user coordinates (as the loader leaves them: divided by width / height), y [B][2 + K] = UAV position in metres |
// powers.  Two quirks of the reference are kept: the x gradient's second term reads the user's Y coordinate, and the coordinates
// and the position are on different scales.
template <int KMAX>
__global__ __launch_bounds__(kGdThreads) void k_gd_nu(const double* __restrict__ X, double* __restrict__ Y, long long B, int K, int iters,
                                                      double lr, double p_ref, GdRec rec) {
#pragma clang fp contract(off)
    const long long row = (long long)blockIdx.x * kGdThreads + threadIdx.x;
    if (row >= B) return;
    const double* x = X + row * 2 * K;
    double* y = Y + row * (2 + K);
    double cx[KMAX], cy[KMAX], p[KMAX], tmp[KMAX];
    double px = y[0], py = y[1];
#pragma unroll
    for (int i = 0; i < KMAX; ++i)
        if (i < K) { cx[i] = x[2 * i]; cy[i] = x[2 * i + 1]; p[i] = y[2 + i]; }
    for (int it = 1; it <= iters; ++it) {
        double D = 0.0, P = 0.0;
#pragma unroll
        for (int i = 0; i < KMAX; ++i)
            if (i < K) {
                const double d = (px - cx[i]) * (px - cx[i]) + (py - cy[i]) * (py - cy[i]);
                tmp[i] = 6 + 11.0 / 6.0 * (22500 + d);
                D = i == 0 ? d : D + d;
                P = i == 0 ? p[0] : P + p[i];
            }
        const double DD = D * D;
        const double pen = 1 / ((P - p_ref) * (P - p_ref));
        double gx = 0.0, gy = 0.0;
#pragma unroll
        for (int i = 0; i < KMAX; ++i)
            if (i < K) {
                const double q = 1 + p[i] / tmp[i], tt = tmp[i] * tmp[i];
                gx = gx + (-p[i] * (px - cx[i]) * 11 / 3 / tt / q / kGdLn2 + 2 * (cy[i] - px) / DD);
                gy = gy + (-p[i] * (py - cy[i]) * 11 / 3 / tt / q / kGdLn2 + 2 * (cy[i] - py) / DD);
                const double gp = -1 / tmp[i] / q / kGdLn2 + pen;
                p[i] = p[i] + gp * lr;
            }
        px = px + gx * lr;
        py = py + gy * lr;
        if (double* r = rec.slot(it, B, 2 + K, row)) {
            r[0] = px; r[1] = py;
#pragma unroll
            for (int i = 0; i < KMAX; ++i)
                if (i < K) r[2 + i] = p[i];
        }
    }
    if (iters > 0) {
        y[0] = px; y[1] = py;
#pragma unroll
        for (int i = 0; i < KMAX; ++i)
            if (i < K) y[2 + i] = p[i];
    }
}

}  // namespace dsg
