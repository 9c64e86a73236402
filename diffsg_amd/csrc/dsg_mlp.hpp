// dsg_mlp.hpp -- the MTFNN baseline (reference: baselines/MTFNN.py): a plain MLP of 2..5 Linear layers, ReLU between them, and a head
// that applies a sigmoid to the first n_sig output columns and one softmax over the rest; inference, MSE loss + full gradient, and a
// whole training epoch (every mini-batch's forward, backward and Adam step) in ONE launch.  DESIGN.md section 11.
//
// The nets have 2.5 - 8.5 k parameters: a whole model sits in the LDS of one compute unit.  One workgroup (256 threads) owns one
// model.  It walks a batch in tiles of TR rows (64; 32 / 16 for the widest nets the limits allow); the tile's activations of every
// layer stay in LDS (row stride odd: lanes are rows, so the 32 banks are hit once each; a weight is one broadcast address per wave):
//   forward   lane = row, a wave-uniform group of 4 output columns per thread, k innermost                 (mlp_layer_fwd)
//   head      one thread per row: sigmoid / softmax, the row's squared error, and d loss / d z in place      (mlp_head)
//   wgrad     one thread per (4 output columns, 1 input column | bias): sum over the tile's rows in row order, then added to the
//             batch's gradient -- tiles in tile order                                                       (mlp_layer_wgrad)
//   dgrad     lane = row, 4 input columns per thread, ReLU mask from the stored activation, written over it  (mlp_layer_dgrad)
// No atomics and no cross-workgroup reduction: every sum over rows has ONE order, fixed by (TR, batch), which depend on the net's
// shape only.  dsg_mlp_loss_grad is the same device function (mlp_batch_grad) in a workgroup of its own, and the epoch kernel's update
// is adam_one of k_adam with the bias corrections formed by the same expressions: the epoch kernel is bit-identical to
// dsg_mlp_loss_grad + dsg_adam_step per batch (tests/test_gpu_mtfnn.py holds it to that).  The device functions below switch floating-point
// contraction off: a product and a sum fuse only where fmaf says so, so a function computes the same bits in every kernel it is inlined into.
// The PPO baseline (dsg_ppo.hpp) is built from the same pieces: the layer functions take the activation (ReLU here, tanh there) as a
// template argument, and mlp_layer_wgrad, mlp_load_tile, mlp_head_row, mlp_clamp_row, MlpAdam and mlp_adam_step serve both.
#pragma once
#include "dsg_kernels.hpp"

namespace dsg {

constexpr int kMlpMaxLayers = 5, kMlpMaxIO = 128, kMlpMaxHidden = 64, kMlpThreads = 256;
constexpr int kMlpScal = 80;                    // LDS floats in front of the parameters: [0] the batch's squared-error sum, [16 + r] row r's
constexpr int kMlpLdsFloats = 163840 / 4;       // one workgroup may hold the whole LDS of a gfx950 CU

// Layout worked out on the host (mlp_plan in dsg_api.hip) and read from the kernel arguments (uniform indices: scalar loads).
struct MlpPlan {
    int L, n_sig, P;            // Linear layers, sigmoid columns, parameter count
    int TR, tr_shift;           // rows per tile (a power of two <= 64) and its log2
    int w[kMlpMaxLayers + 1];   // widths: w[0] inputs ... w[L] outputs
    int woff[kMlpMaxLayers], boff[kMlpMaxLayers];     // weight / bias offsets in the flat state-dict-order vector
    int aoff[kMlpMaxLayers + 1], astr[kMlpMaxLayers + 1];   // activation l of the tile: offset in the tile area (floats) and row stride (odd)
    int yoff, ystr;             // the tile's targets
    int act_floats;             // size of the tile area
    int onchip;                 // epoch kernel: gradient and both Adam moments in LDS beside the parameters
    int lds_floats;             // dynamic LDS of the launch
};

// The activation between the layers, a template argument of the two layer functions that apply it: ReLU (MTFNN) or tanh (PPO).
constexpr int kMlpRelu = 0, kMlpTanh = 1;

template <int ACT>
__device__ __forceinline__ float mlp_act(float z) {
    return ACT == kMlpTanh ? tanhf(z) : (z > 0.f ? z : 0.f);
}

// d act / d z times g, from the stored activation s = act(z): the ReLU mask, or 1 - s^2.
template <int ACT>
__device__ __forceinline__ float mlp_act_bwd(float s, float g) {
#pragma clang fp contract(off)
    return ACT == kMlpTanh ? (1.f - s * s) * g : (s > 0.f ? g : 0.f);
}

// a_out[r][j] = (act)(b[j] + sum_k W[j][k] a_in[r][k]) for the tile's TR rows
template <int ACT = kMlpRelu>
__device__ __forceinline__ void mlp_layer_fwd(const float* __restrict__ W, const float* __restrict__ b, const float* __restrict__ ain, int sin,
                                              float* __restrict__ aout, int sout, int in, int out, int TR, int tr_shift, bool act) {
#pragma clang fp contract(off)
    const int r = threadIdx.x & (TR - 1), jg = threadIdx.x >> tr_shift, NG = kMlpThreads >> tr_shift;
    const float* ar = ain + r * sin;
    for (int jb = 4 * jg; jb < out; jb += 4 * NG) {
        const int j1 = min(jb + 1, out - 1), j2 = min(jb + 2, out - 1), j3 = min(jb + 3, out - 1);      // clamped: read, not stored
        const float *w0 = W + jb * in, *w1 = W + j1 * in, *w2 = W + j2 * in, *w3 = W + j3 * in;
        float a0 = b[jb], a1 = b[j1], a2 = b[j2], a3 = b[j3];
        for (int k = 0; k < in; ++k) {
            const float x = ar[k];
            a0 = fmaf(w0[k], x, a0); a1 = fmaf(w1[k], x, a1); a2 = fmaf(w2[k], x, a2); a3 = fmaf(w3[k], x, a3);
        }
        if (act) { a0 = mlp_act<ACT>(a0); a1 = mlp_act<ACT>(a1); a2 = mlp_act<ACT>(a2); a3 = mlp_act<ACT>(a3); }
        float* o = aout + r * sout + jb;
        o[0] = a0;
        if (jb + 1 < out) o[1] = a1;
        if (jb + 2 < out) o[2] = a2;
        if (jb + 3 < out) o[3] = a3;
    }
}

// The head on one row, in place: sigmoid on columns [0, n_sig), softmax (torch.softmax(dim=1)) over [n_sig, out).
__device__ __forceinline__ void mlp_head_row(float* __restrict__ z, int out, int n_sig) {
#pragma clang fp contract(off)
    for (int j = 0; j < n_sig; ++j) z[j] = 1.f / (1.f + expf(-z[j]));
    if (n_sig < out) {
        float mx = z[n_sig];
        for (int j = n_sig + 1; j < out; ++j) mx = fmaxf(mx, z[j]);
        float s = 0.f;
        for (int j = n_sig; j < out; ++j) { const float e = expf(z[j] - mx); z[j] = e; s += e; }
        for (int j = n_sig; j < out; ++j) z[j] = z[j] / s;
    }
}

// Head, the row's squared error and d(mean squared error)/d(pre-activation) of the last layer, one thread per row, in place.
// gscale = 2 / (batch rows * out): d mean((y - o)^2) / d o = gscale * (o - y).
__device__ __forceinline__ void mlp_head(float* __restrict__ aL, int sL, const float* __restrict__ yb, int sy, int out, int n_sig, int nrows,
                                         float gscale, float* __restrict__ rowloss) {
#pragma clang fp contract(off)
    const int r = threadIdx.x;
    if (r >= nrows) return;
    float* z = aL + r * sL;
    const float* y = yb + r * sy;
    mlp_head_row(z, out, n_sig);
    float se = 0.f, dot = 0.f;
    for (int j = 0; j < out; ++j) { const float d = y[j] - z[j]; se = fmaf(d, d, se); }
    rowloss[r] = se;
    for (int j = n_sig; j < out; ++j) dot = fmaf(gscale * (z[j] - y[j]), z[j], dot);
    for (int j = 0; j < n_sig; ++j) { const float s = z[j]; z[j] = gscale * (s - y[j]) * s * (1.f - s); }
    for (int j = n_sig; j < out; ++j) { const float p = z[j]; z[j] = p * (gscale * (p - y[j]) - dot); }
}

// g_W[j][k] (+)= sum_r delta[r][j] a_in[r][k],  g_b[j] (+)= sum_r delta[r][j]: rows in row order, then one add to the batch's gradient.
__device__ __forceinline__ void mlp_layer_wgrad(const float* __restrict__ delta, int sd, const float* __restrict__ ain, int sin, int in, int out,
                                                int nrows, float* gW, float* gb, bool first) {
#pragma clang fp contract(off)
    const int K1 = in + 1, nitems = ((out + 3) >> 2) * K1;
    for (int item = threadIdx.x; item < nitems; item += kMlpThreads) {
        const int q = item / K1, k = item - q * K1, jb = 4 * q;
        const int j1 = min(jb + 1, out - 1), j2 = min(jb + 2, out - 1), j3 = min(jb + 3, out - 1);
        const bool bias = k == in;
        const float* ac = ain + (bias ? 0 : k);
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        for (int r = 0; r < nrows; ++r) {
            const float a = bias ? 1.f : ac[r * sin];
            const float* d = delta + r * sd;
            s0 = fmaf(d[jb], a, s0); s1 = fmaf(d[j1], a, s1); s2 = fmaf(d[j2], a, s2); s3 = fmaf(d[j3], a, s3);
        }
        const float s[4] = {s0, s1, s2, s3};
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            if (jb + jj >= out) break;
            float* dst = bias ? gb + jb + jj : gW + (jb + jj) * in + k;
            *dst = first ? s[jj] : *dst + s[jj];
        }
    }
}

// a_in[r][k] <- act'(a_in[r][k]) * sum_j W[j][k] delta[r][j]   (the activation in front of this layer, from the stored activation; every
// thread touches its own elements)
template <int ACT = kMlpRelu>
__device__ __forceinline__ void mlp_layer_dgrad(const float* __restrict__ W, const float* __restrict__ delta, int sd, float* ain, int sin, int in,
                                                int out, int TR, int tr_shift) {
#pragma clang fp contract(off)
    const int r = threadIdx.x & (TR - 1), kg = threadIdx.x >> tr_shift, NG = kMlpThreads >> tr_shift;
    const float* d = delta + r * sd;
    for (int kb = 4 * kg; kb < in; kb += 4 * NG) {
        const int k1 = min(kb + 1, in - 1), k2 = min(kb + 2, in - 1), k3 = min(kb + 3, in - 1);
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        for (int j = 0; j < out; ++j) {
            const float dj = d[j];
            const float* wj = W + j * in;
            a0 = fmaf(wj[kb], dj, a0); a1 = fmaf(wj[k1], dj, a1); a2 = fmaf(wj[k2], dj, a2); a3 = fmaf(wj[k3], dj, a3);
        }
        float* o = ain + r * sin + kb;
        o[0] = mlp_act_bwd<ACT>(o[0], a0);
        if (kb + 1 < in) o[1] = mlp_act_bwd<ACT>(o[1], a1);
        if (kb + 2 < in) o[2] = mlp_act_bwd<ACT>(o[2], a2);
        if (kb + 3 < in) o[3] = mlp_act_bwd<ACT>(o[3], a3);
    }
}

// A row index clamped into [0, N): a permutation entry out of range reads a row of the dataset, never past it.
__device__ __forceinline__ long long mlp_clamp_row(long long idx, long long N) { return idx < 0 ? 0 : (idx >= N ? N - 1 : idx); }

// Rows [row0, row0 + nrows) of src (through perm, if given; indices clamped into [0, N)) into the tile, the other tile rows zeroed.
__device__ __forceinline__ void mlp_load_tile(const float* __restrict__ src, const int* __restrict__ perm, long long N, long long row0, int nrows,
                                              int width, float* __restrict__ dst, int stride, int TR) {
    for (int e = threadIdx.x; e < TR * width; e += kMlpThreads) {
        const int r = e / width, c = e - r * width;
        float v = 0.f;
        if (r < nrows) {
            const long long idx = perm ? (long long)perm[row0 + r] : row0 + r;
            v = src[(size_t)mlp_clamp_row(idx, N) * width + c];
        }
        dst[r * stride + c] = v;
    }
}

__device__ __forceinline__ void mlp_tile_forward(const MlpPlan& p, const float* __restrict__ wl, float* __restrict__ act) {
    for (int l = 0; l < p.L; ++l) {
        mlp_layer_fwd(wl + p.woff[l], wl + p.boff[l], act + p.aoff[l], p.astr[l], act + p.aoff[l + 1], p.astr[l + 1], p.w[l], p.w[l + 1], p.TR,
                      p.tr_shift, l + 1 < p.L);
        __syncthreads();
    }
}

// One batch: loss = mean((Y - net(X))^2) over the rows perm[row0 .. row0 + brows) and its gradient for every parameter (flat layout) into
// g; *loss_dst receives the loss.  wl: the parameters in LDS; act / scal: the workgroup's tile area and scalar slots.  Called by all
// threads; ends with a barrier, after which g and *loss_dst are complete.
__device__ __forceinline__ void mlp_batch_grad(const MlpPlan& p, const float* __restrict__ wl, float* __restrict__ act, float* __restrict__ scal,
                                               const float* __restrict__ X, const float* __restrict__ Y, const int* __restrict__ perm, long long N,
                                               long long row0, int brows, float* g, float* loss_dst) {
#pragma clang fp contract(off)
    const int L = p.L, out = p.w[L], TR = p.TR;
    const float gscale = 2.0f / (float)((long long)brows * out);
    if (threadIdx.x == 0) scal[0] = 0.f;
    for (int t0 = 0; t0 < brows; t0 += TR) {
        const int nrows = min(TR, brows - t0);
        mlp_load_tile(X, perm, N, row0 + t0, nrows, p.w[0], act + p.aoff[0], p.astr[0], TR);
        mlp_load_tile(Y, perm, N, row0 + t0, nrows, out, act + p.yoff, p.ystr, TR);
        __syncthreads();
        mlp_tile_forward(p, wl, act);
        mlp_head(act + p.aoff[L], p.astr[L], act + p.yoff, p.ystr, out, p.n_sig, nrows, gscale, scal + 16);
        __syncthreads();
        if (threadIdx.x == 0) {
            float s = scal[0];
            for (int r = 0; r < nrows; ++r) s += scal[16 + r];
            scal[0] = s;
        }
        for (int l = L - 1; l >= 0; --l) {
            mlp_layer_wgrad(act + p.aoff[l + 1], p.astr[l + 1], act + p.aoff[l], p.astr[l], p.w[l], p.w[l + 1], nrows, g + p.woff[l], g + p.boff[l],
                            t0 == 0);
            __syncthreads();
            if (l > 0) {
                mlp_layer_dgrad(wl + p.woff[l], act + p.aoff[l + 1], p.astr[l + 1], act + p.aoff[l], p.astr[l], p.w[l], p.w[l + 1], TR, p.tr_shift);
                __syncthreads();
            }
        }
    }
    if (threadIdx.x == 0) *loss_dst = scal[0] / (float)((long long)brows * out);
    __syncthreads();
}

// out[rows][w[L]] = net(x[rows][w[0]]): one tile per workgroup trip.
__global__ __launch_bounds__(kMlpThreads) void k_mlp_forward(MlpPlan p, const float* __restrict__ params, const float* __restrict__ x,
                                                             float* __restrict__ out, long long rows) {
    extern __shared__ float mlp_lds[];
    float* wl = mlp_lds + kMlpScal;
    float* act = wl + p.P;
    for (int i = threadIdx.x; i < p.P; i += kMlpThreads) wl[i] = params[i];
    const int L = p.L, od = p.w[L], TR = p.TR;
    const long long ntiles = (rows + TR - 1) / TR;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long row0 = tile * TR;
        const int nrows = (int)(rows - row0 < TR ? rows - row0 : TR);
        __syncthreads();                        // the parameters are in; the previous trip's readers are done
        mlp_load_tile(x, nullptr, rows, row0, nrows, p.w[0], act + p.aoff[0], p.astr[0], TR);
        __syncthreads();
        mlp_tile_forward(p, wl, act);
        if ((int)threadIdx.x < nrows) mlp_head_row(act + p.aoff[L] + threadIdx.x * p.astr[L], od, p.n_sig);
        __syncthreads();
        for (int e = threadIdx.x; e < nrows * od; e += kMlpThreads) {
            const int r = e / od, c = e - r * od;
            out[(size_t)(row0 + r) * od + c] = act[p.aoff[L] + r * p.astr[L] + c];
        }
    }
}

// loss and gradient of ONE batch of `rows` rows (no update): mlp_batch_grad in a workgroup of its own.
__global__ __launch_bounds__(kMlpThreads) void k_mlp_loss_grad(MlpPlan p, const float* __restrict__ params, const float* __restrict__ x,
                                                               const float* __restrict__ y, int rows, float* __restrict__ loss_out,
                                                               float* __restrict__ grad) {
    extern __shared__ float mlp_lds[];
    float* wl = mlp_lds + kMlpScal;
    for (int i = threadIdx.x; i < p.P; i += kMlpThreads) wl[i] = params[i];
    __syncthreads();
    mlp_batch_grad(p, wl, wl + p.P, mlp_lds, x, y, nullptr, rows, 0, rows, grad, loss_out);
}

// Adam's hyper-parameters and the number of steps taken before the epoch: the tail of both epoch kernels' arguments (k_ppo_epoch too).
struct MlpAdam {
    double lr, beta1, beta2, eps;
    long long step0;
};

// What adam_one needs for step number `step` over P parameters, the bias corrections formed as k_adam forms them.
struct MlpAdamStep {
    AdamArgs a;
    float bias_correction1, bias_correction2_sqrt;
};
__device__ __forceinline__ MlpAdamStep mlp_adam_step(int P, MlpAdam h, long long step) {
    const AdamArgs a{nullptr, nullptr, nullptr, nullptr, (size_t)P, h.lr, h.beta1, h.beta2, 0.0, h.eps, (float)step, 0, nullptr, nullptr};
    const double bc1 = 1 - pow(a.beta1, (double)a.step), bc2 = 1 - pow(a.beta2, (double)a.step);
    return {a, (float)bc1, (float)sqrt(bc2)};
}

struct MlpEpochArgs {
    float* params; float* m; float* v;      // [R][P]
    float* gws;                             // [R][P] gradient workspace when the net's gradient and moments do not fit in LDS, else null
    const float* X; const float* Y;         // [N][w[0]], [N][w[L]]
    const int* perm;                        // [R][N]
    float* batch_loss;                      // [R][nb]
    int N, batch, nb;
    MlpAdam adam;
};

// One epoch of one model per workgroup: for every batch mlp_batch_grad, then Adam (adam_one with mlp_adam_step) on the parameters held in
// LDS.  Parameters (and, where they fit, the moments) are read once and written back once.
__global__ __launch_bounds__(kMlpThreads) void k_mlp_epoch(MlpPlan p, MlpEpochArgs e) {
    extern __shared__ float mlp_lds[];
    const int P = p.P;
    const size_t rep = blockIdx.x;
    float* wl = mlp_lds + kMlpScal;
    float* act = wl + P;
    float *g, *m, *v;
    if (p.onchip) {
        g = act + p.act_floats; m = g + P; v = m + P;
        for (int i = threadIdx.x; i < P; i += kMlpThreads) { m[i] = e.m[rep * P + i]; v[i] = e.v[rep * P + i]; }
    } else {
        g = e.gws + rep * P; m = e.m + rep * P; v = e.v + rep * P;
    }
    for (int i = threadIdx.x; i < P; i += kMlpThreads) wl[i] = e.params[rep * P + i];
    __syncthreads();
    for (int k = 0; k < e.nb; ++k) {
        const long long row0 = (long long)k * e.batch;
        const int brows = (int)(e.N - row0 < e.batch ? e.N - row0 : e.batch);
        mlp_batch_grad(p, wl, act, mlp_lds, e.X, e.Y, e.perm + rep * e.N, e.N, row0, brows, g, e.batch_loss + rep * e.nb + k);
        const MlpAdamStep t = mlp_adam_step(P, e.adam, e.adam.step0 + k + 1);
        for (int i = threadIdx.x; i < P; i += kMlpThreads) adam_one(wl[i], g[i], m[i], v[i], t.a, t.bias_correction1, t.bias_correction2_sqrt);
        __syncthreads();
    }
    for (int i = threadIdx.x; i < P; i += kMlpThreads) e.params[rep * P + i] = wl[i];
    if (p.onchip)
        for (int i = threadIdx.x; i < P; i += kMlpThreads) { e.m[rep * P + i] = m[i]; e.v[rep * P + i] = v[i]; }
}

}  // namespace dsg
