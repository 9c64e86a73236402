// dsg_ppo.hpp -- the PPO baseline (reference: baselines/PPO.py): an actor and a critic, each a 4-layer tanh MLP state -> h1 -> h2 -> h3 ->
// {A | 1}, a state-independent log_std, and one environment step of CO, MSR or NU as the reward.  Inference of both nets, one batch's
// losses + full gradient, and a whole training epoch (every mini-batch's forward, Gaussian action, log-probability, reward, clipped
// surrogate and value losses, both backward passes and the Adam step) in ONE launch.  DESIGN.md section 12.
//
// The shape is k_mlp_epoch's (dsg_mlp.hpp): one workgroup (256 threads) owns one model, its parameters sit in LDS for the whole epoch,
// a batch is walked in tiles of TR rows whose activations (both nets, row stride odd) stay in LDS, weights are wave-uniform broadcasts.
// Shared with dsg_mlp.hpp, not copied: the layer functions (mlp_layer_fwd / mlp_layer_dgrad with the tanh activation, mlp_layer_wgrad),
// mlp_load_tile, mlp_head_row, the row clamp, and Adam's arguments and bias corrections (MlpAdam, mlp_adam_step).
// A batch takes three passes, because the NU decoder needs the (min, max) of the WHOLE batch's softmaxed actions before any reward exists:
//   pass 1  per tile: forward of both nets; per row: a = noise * std + mu, new_logp, softmax(a), value  -> the batch buffer
//   pass 2  NU: workgroup-wide (min, max) of the buffer's columns 0, 1; per tile: X / Y rows again, one thread per row: reward, then the
//           row's sum of min(ratio adv, clamp(ratio) adv); then ONE thread sums the rows in row order: actor loss, critic loss, reward sum
//   pass 3  per tile: the forward again (the same function on the same inputs: the same bits), d loss / d mu and d loss / d value per
//           row, then layer by layer wgrad (mlp_layer_wgrad: rows in row order, tiles in tile order) and dgrad (1 - a^2 of the stored a)
// The batch buffer is [rows][2A + 2]: softmaxed action | new_logp | value | reward (slot 0 is reused for the row's surrogate sum once
// the reward exists); in LDS where it fits, else in a global workspace.  No atomics; every sum over rows has ONE order.  The advantage is
// NOT detached (PPO.py:148-152): the critic receives d actor_loss / d value as well.  log_std is read, never differentiated or updated.
// Contraction is off inside the device functions below, as in dsg_mlp.hpp -- but the pragma does not reach into the objective functions of
// dsg_eval.hpp that ppo_reward_row inlines (co_cost_row, msr_term, nu_decode_row, nu_rate_row; they are shared with the evaluators and
// carry none): whether `1 + p * g` or `H * H + dx * dx + dy * dy` fuses there is the backend's choice, made from the same inlined body in
// k_ppo_loss_grad and k_ppo_epoch.  The bit-identity of the two kernels rests on that choice being the same in both (the hazard
// dsg_kernels.hpp describes at adam_one); tests/test_gpu_ppo.py's composition test is what holds it.
#pragma once
#include "dsg_eval.hpp"
#include "dsg_mlp.hpp"

namespace dsg {

constexpr int kPpoScal = 160;       // LDS floats in front of the parameters: [4], [5] NU's (min, max), [8 + 2 w], [9 + 2 w] wave w's
                                    // (min, max), [96, 160) zeros (NU: every user at the origin); the rest is unused (the sums go to out3)
constexpr int kPpoZero = 96;
constexpr int kPpoCO = 0, kPpoMSR = 1, kPpoNU = 2;

// Layout worked out on the host (ppo_plan in dsg_api.hip).  Net 0 is the critic, net 1 the actor.
struct PpoPlan {
    int S, A, P, env;
    int TR, tr_shift;
    int w[2][5];                    // widths of net n: w[n][0] = S ... w[n][4] = 1 | A
    int woff[2][4], boff[2][4];     // offsets in the flat vector (log_std[A] first, then the critic, then the actor)
    int aoff[2][5], astr[2][5];     // activation l of net n in the tile area; aoff[.][0] is the shared state tile
    int yoff, ystr;                 // the tile's targets (pass 2)
    int act_floats;
    int onchip;                     // epoch kernel: gradient and both Adam moments in LDS
    int lds_floats;                 // scalar slots + parameters + tile area [+ gradient and moments]; the batch buffer goes behind it
    float lo, span, W, width, height, p_sum;        // scaler_min, (float)(scaler_max - scaler_min), W | NU's area and power
};

// Both nets on the tile whose states are in place: layer l of the critic and of the actor, then one barrier.
__device__ __forceinline__ void ppo_tile_forward(const PpoPlan& p, const float* __restrict__ wl, float* __restrict__ act) {
    for (int l = 0; l < 4; ++l) {
#pragma unroll
        for (int n = 0; n < 2; ++n)
            mlp_layer_fwd<kMlpTanh>(wl + p.woff[n][l], wl + p.boff[n][l], act + p.aoff[n][l], p.astr[n][l], act + p.aoff[n][l + 1], p.astr[n][l + 1],
                                    p.w[n][l], p.w[n][l + 1], p.TR, p.tr_shift, l < 3);
        __syncthreads();
    }
}

// The dataset row of position pos (through perm, if given), clamped into [0, N).
__device__ __forceinline__ long long ppo_row(const int* __restrict__ perm, long long N, long long pos) {
    const long long idx = perm ? (long long)perm[pos] : pos;
    return mlp_clamp_row(idx, N);
}

constexpr float kPpoLogSqrt2Pi = (float)0.9189385332046727;     // math.log(math.sqrt(2 * math.pi))
constexpr float kPpoReturn = (float)(0.99 * 3.8);               // calc_advantage's gamma * 3.8, rounded to float32 once

// a = noise * std + mu (a product, then a sum) and Normal(mu, std).log_prob(a) in torch's order of operations.
__device__ __forceinline__ float ppo_action(float noise, float mu, float log_std, float& logp, float& d_over_var) {
#pragma clang fp contract(off)
    const float sd = expf(log_std);
    const float ns = noise * sd;
    const float a = ns + mu;
    const float d = a - mu, var = sd * sd;
    logp = -(d * d) / (2.f * var) - logf(sd) - kPpoLogSqrt2Pi;
    d_over_var = d / var;
    return a;
}

// The reward of one row.  act: the row's softmaxed action (buffer); xs: the row's state in the tile (CO: scaled in place); y: the
// row's target; dec: A floats of the row's own (NU: the decoded action); mm: NU's batch-wide (min, max); zeros: >= 64 zeros.
__device__ __forceinline__ float ppo_reward_row(const PpoPlan& p, const float* __restrict__ act, float* __restrict__ xs, const float* __restrict__ y,
                                                float* __restrict__ dec, float2 mm, const float* __restrict__ zeros) {
#pragma clang fp contract(off)
    const int A = p.A;
    float c, gt, offset;
    if (p.env == kPpoCO) {
        for (int k = 0; k < p.S; ++k) { const float t = xs[k] * p.span; xs[k] = t + p.lo; }
        c = co_cost_row(xs, act, A);
        gt = co_cost_row(xs, y, A);
        offset = 0.1f;
    } else if (p.env == kPpoMSR) {
        c = 0.f; gt = 0.f;
        for (int j = 0; j < A; ++j) {
            const float t = xs[j] * p.span;
            const float g = t + p.lo;
            c += msr_term(act[j] * p.W, g);
            gt += msr_term(y[j] * p.W, g);
        }
        offset = 0.01f;
    } else {
        nu_decode_row(act, dec, A, p.width, p.height, p.p_sum, mm);
        float rate[2];
#pragma unroll 1
        for (int t = 0; t < 2; ++t) rate[t] = nu_rate_row(t ? y : dec, zeros, A - 2);   // one copy of the rate's body (registers)
        c = rate[0]; gt = rate[1];
        offset = 0.1f;
    }
    return 1.0f / (fabsf(c - gt) + offset);
}

struct PpoBatchIO {
    const float* X; const float* Y;         // [N][S], [N][A]
    const float* old_logp;                  // [N][A], by dataset row
    const float* noise;                     // [N][A], by position
    const int* perm;                        // [N] or null (identity)
    float* logp_dst;                        // [N][A], by dataset row: this batch's new_logp (may be old_logp itself)
    float* reward_dst;                      // [N] by position, or null
    long long N;
};

// One batch of brows rows at positions [row0, row0 + brows): out3 = {actor loss, critic loss, sum of rewards}, the gradient of
// (actor loss + critic loss) for the critic and actor range of g (flat layout; the log_std slots are not touched), new_logp to
// io.logp_dst.  wl: the parameters in LDS; act / scal: the workgroup's tile area and scalar slots; buf: the batch buffer
// [brows][2A + 2].  Called by all threads; ends with a barrier, after which everything is complete.
__device__ __forceinline__ void ppo_batch(const PpoPlan& p, const float* __restrict__ wl, float* __restrict__ act, float* __restrict__ scal,
                                          float* __restrict__ buf, const PpoBatchIO& io, long long row0, int brows, float* g, float* out3) {
#pragma clang fp contract(off)
    const int A = p.A, TR = p.TR, bs = 2 * A + 2;
    const int tid = threadIdx.x;
    const float inv_ba = 1.0f / (float)((long long)brows * A), inv_b = 1.0f / (float)brows;
    float* mu_t = act + p.aoff[1][4];
    float* val_t = act + p.aoff[0][4];
    const int smu = p.astr[1][4], sval = p.astr[0][4];

    // ---- pass 1: forward, action, log-probability, softmax, value
    for (int t0 = 0; t0 < brows; t0 += TR) {
        const int nrows = min(TR, brows - t0);
        mlp_load_tile(io.X, io.perm, io.N, row0 + t0, nrows, p.S, act + p.aoff[0][0], p.astr[0][0], TR);
        __syncthreads();
        ppo_tile_forward(p, wl, act);
        if (tid < nrows) {
            float* mu = mu_t + tid * smu;
            const float* nz = io.noise + (size_t)(row0 + t0 + tid) * A;
            float* b = buf + (size_t)(t0 + tid) * bs;
            for (int j = 0; j < A; ++j) {
                float lp, dv;
                mu[j] = ppo_action(nz[j], mu[j], wl[j], lp, dv);
                b[A + j] = lp;
            }
            mlp_head_row(mu, A, 0);                       // torch.softmax(actions, dim=1)
            for (int j = 0; j < A; ++j) b[j] = mu[j];
            b[2 * A] = val_t[tid * sval];
        }
        __syncthreads();
    }

    // ---- pass 2: (NU: the batch's min / max,) rewards, the rows' surrogate sums, the three sums of the batch
    if (p.env == kPpoNU) {
        float lo = INFINITY, hi = -INFINITY;
        for (int r = tid; r < brows; r += kMlpThreads) {
            const float u = buf[(size_t)r * bs], v = buf[(size_t)r * bs + 1];
            lo = fminf(lo, fminf(u, v)); hi = fmaxf(hi, fmaxf(u, v));
        }
        lo = wave_min_f(lo); hi = wave_max_f(hi);
        if ((tid & 63) == 0) { scal[8 + 2 * (tid >> 6)] = lo; scal[9 + 2 * (tid >> 6)] = hi; }
        __syncthreads();
        if (tid == 0) {
            scal[4] = fminf(fminf(scal[8], scal[10]), fminf(scal[12], scal[14]));
            scal[5] = fmaxf(fmaxf(scal[9], scal[11]), fmaxf(scal[13], scal[15]));
        }
        __syncthreads();
    }
    for (int t0 = 0; t0 < brows; t0 += TR) {
        const int nrows = min(TR, brows - t0);
        mlp_load_tile(io.X, io.perm, io.N, row0 + t0, nrows, p.S, act + p.aoff[0][0], p.astr[0][0], TR);
        mlp_load_tile(io.Y, io.perm, io.N, row0 + t0, nrows, A, act + p.yoff, p.ystr, TR);
        __syncthreads();
        if (tid < nrows) {
            float* b = buf + (size_t)(t0 + tid) * bs;
            const float reward = ppo_reward_row(p, b, act + p.aoff[0][0] + tid * p.astr[0][0], act + p.yoff + tid * p.ystr, mu_t + tid * smu,
                                                make_float2(scal[4], scal[5]), scal + kPpoZero);
            b[2 * A + 1] = reward;
            const float ret = reward + kPpoReturn;
            const float adv = ret - b[2 * A];
            const float* old = io.old_logp + (size_t)ppo_row(io.perm, io.N, row0 + t0 + tid) * A;
            float ms = 0.f;
            for (int j = 0; j < A; ++j) {
                const float ratio = expf(b[A + j] - old[j]);
                const float u = ratio * adv, c = fminf(fmaxf(ratio, 0.8f), 1.2f) * adv;
                ms += fminf(u, c);
            }
            b[0] = ms;
        }
        __syncthreads();
    }
    if (tid == 0) {
        float sa = 0.f, sc = 0.f, sr = 0.f;
        for (int r = 0; r < brows; ++r) {
            const float* b = buf + (size_t)r * bs;
            const float reward = b[2 * A + 1];
            const float ret = reward + kPpoReturn;
            const float d = b[2 * A] - ret;
            sa += b[0];
            sc = fmaf(d, d, sc);
            sr += reward;
        }
        out3[0] = -(sa * inv_ba);
        out3[1] = sc * inv_b;
        out3[2] = sr;
    }

    // ---- pass 3: the forward again, d loss / d (mu, value), backward of both nets
    for (int t0 = 0; t0 < brows; t0 += TR) {
        const int nrows = min(TR, brows - t0);
        mlp_load_tile(io.X, io.perm, io.N, row0 + t0, nrows, p.S, act + p.aoff[0][0], p.astr[0][0], TR);
        __syncthreads();
        ppo_tile_forward(p, wl, act);
        if (tid < nrows) {
            float* mu = mu_t + tid * smu;
            const float* nz = io.noise + (size_t)(row0 + t0 + tid) * A;
            const float* b = buf + (size_t)(t0 + tid) * bs;
            const float* old = io.old_logp + (size_t)ppo_row(io.perm, io.N, row0 + t0 + tid) * A;
            const float value = val_t[tid * sval];
            const float ret = b[2 * A + 1] + kPpoReturn;
            const float adv = ret - value;
            float dadv = 0.f;
            for (int j = 0; j < A; ++j) {
                float lp, dv;
                ppo_action(nz[j], mu[j], wl[j], lp, dv);
                const float ratio = expf(lp - old[j]);
                const float cr = fminf(fmaxf(ratio, 0.8f), 1.2f);
                const float u = ratio * adv, c = cr * adv;
                // torch.min's backward: the smaller argument takes the gradient, equal arguments half each; clamp passes it inside
                // [0.8, 1.2], the bounds included
                const float wu = u < c ? 1.f : (u == c ? 0.5f : 0.f), wc = 1.f - wu;
                const bool pass = ratio >= 0.8f && ratio <= 1.2f;
                const float dr = wu * adv + (pass ? wc * adv : 0.f);
                dadv += wu * ratio + wc * cr;
                mu[j] = -inv_ba * dr * ratio * dv;
            }
            val_t[tid * sval] = inv_ba * dadv + 2.0f * inv_b * (value - ret);
        }
        __syncthreads();
        for (int l = 3; l >= 0; --l) {
#pragma unroll
            for (int n = 0; n < 2; ++n)
                mlp_layer_wgrad(act + p.aoff[n][l + 1], p.astr[n][l + 1], act + p.aoff[n][l], p.astr[n][l], p.w[n][l], p.w[n][l + 1], nrows,
                                g + p.woff[n][l], g + p.boff[n][l], t0 == 0);
            __syncthreads();
            if (l > 0) {
#pragma unroll
                for (int n = 0; n < 2; ++n)
                    mlp_layer_dgrad<kMlpTanh>(wl + p.woff[n][l], act + p.aoff[n][l + 1], p.astr[n][l + 1], act + p.aoff[n][l], p.astr[n][l],
                                              p.w[n][l], p.w[n][l + 1], TR, p.tr_shift);
                __syncthreads();
            }
        }
    }
    // every read of old_logp is behind the barrier above: new_logp may now replace it
    for (int e = tid; e < brows * A; e += kMlpThreads) {
        const int r = e / A, j = e - r * A;
        io.logp_dst[(size_t)ppo_row(io.perm, io.N, row0 + r) * A + j] = buf[(size_t)r * bs + A + j];
    }
    if (io.reward_dst)
        for (int r = tid; r < brows; r += kMlpThreads) io.reward_dst[row0 + r] = buf[(size_t)r * bs + 2 * A + 1];
    __syncthreads();
}

__device__ __forceinline__ void ppo_lds_init(const PpoPlan& p, float* __restrict__ lds, const float* __restrict__ params) {
    for (int i = threadIdx.x; i < kPpoScal; i += kMlpThreads) lds[i] = 0.f;
    for (int i = threadIdx.x; i < p.P; i += kMlpThreads) lds[kPpoScal + i] = params[i];
}

// mu[rows][A] = actor(x), value[rows] = critic(x): one tile per workgroup trip.
__global__ __launch_bounds__(kMlpThreads) void k_ppo_forward(PpoPlan p, const float* __restrict__ params, const float* __restrict__ x,
                                                             float* __restrict__ mu_out, float* __restrict__ value_out, long long rows) {
    extern __shared__ float ppo_lds[];
    float* wl = ppo_lds + kPpoScal;
    float* act = wl + p.P;
    ppo_lds_init(p, ppo_lds, params);
    const int A = p.A, TR = p.TR;
    const long long ntiles = (rows + TR - 1) / TR;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long row0 = tile * TR;
        const int nrows = (int)(rows - row0 < TR ? rows - row0 : TR);
        __syncthreads();                        // the parameters are in; the previous trip's readers are done
        mlp_load_tile(x, nullptr, rows, row0, nrows, p.S, act + p.aoff[0][0], p.astr[0][0], TR);
        __syncthreads();
        ppo_tile_forward(p, wl, act);
        for (int e = threadIdx.x; e < nrows * A; e += kMlpThreads) {
            const int r = e / A, c = e - r * A;
            mu_out[(size_t)(row0 + r) * A + c] = act[p.aoff[1][4] + r * p.astr[1][4] + c];
        }
        if ((int)threadIdx.x < nrows) value_out[row0 + threadIdx.x] = act[p.aoff[0][4] + threadIdx.x * p.astr[0][4]];
    }
}

// ONE batch of `rows` rows, no update: ppo_batch in a workgroup of its own.  buf_off: the batch buffer's offset in LDS, or -1 (ws).
__global__ __launch_bounds__(kMlpThreads) void k_ppo_loss_grad(PpoPlan p, const float* __restrict__ params, PpoBatchIO io, int rows, int buf_off,
                                                               float* ws, float* __restrict__ out3, float* __restrict__ grad) {
    extern __shared__ float ppo_lds[];
    float* wl = ppo_lds + kPpoScal;
    ppo_lds_init(p, ppo_lds, params);
    for (int i = threadIdx.x; i < p.A; i += kMlpThreads) grad[i] = 0.f;
    __syncthreads();
    ppo_batch(p, wl, wl + p.P, ppo_lds, buf_off >= 0 ? ppo_lds + buf_off : ws, io, 0, rows, grad, out3);
}

struct PpoEpochArgs {
    float* params; float* m; float* v;      // [R][P]
    float* gws;                             // [R][P] gradient workspace when gradient and moments do not fit in LDS, else null
    float* bufws;                           // [R][bufrows][2A + 2] batch buffer when it does not fit in LDS, else null
    const float* X; const float* Y;         // [N][S], [N][A]
    float* old_logp;                        // [R][N][A] by dataset row: read, then overwritten with this epoch's new_logp
    const float* noise;                     // [R][N][A] by position in the epoch
    const int* perm;                        // [R][N]
    float* batch_out;                       // [R][nb][3]
    int N, batch, nb, bufrows, buf_off;
    MlpAdam adam;
};

// One epoch of one agent per workgroup: for every batch ppo_batch, then Adam (adam_one with mlp_adam_step) over the critic and actor range
// of the parameters held in LDS.
__global__ __launch_bounds__(kMlpThreads) void k_ppo_epoch(PpoPlan p, PpoEpochArgs e) {
    extern __shared__ float ppo_lds[];
    const int P = p.P, A = p.A;
    const size_t rep = blockIdx.x;
    float* wl = ppo_lds + kPpoScal;
    float* act = wl + P;
    float *g, *m, *v;
    ppo_lds_init(p, ppo_lds, e.params + rep * P);
    if (p.onchip) {
        g = act + p.act_floats; m = g + P; v = m + P;
        for (int i = threadIdx.x; i < P; i += kMlpThreads) { m[i] = e.m[rep * P + i]; v[i] = e.v[rep * P + i]; }
    } else {
        g = e.gws + rep * P; m = e.m + rep * P; v = e.v + rep * P;
    }
    float* buf = e.buf_off >= 0 ? ppo_lds + e.buf_off : e.bufws + rep * (size_t)e.bufrows * (2 * A + 2);
    float* old = e.old_logp + rep * (size_t)e.N * A;
    const PpoBatchIO io{e.X, e.Y, old, e.noise + rep * (size_t)e.N * A, e.perm + rep * e.N, old, nullptr, e.N};
    __syncthreads();
    for (int k = 0; k < e.nb; ++k) {
        const long long row0 = (long long)k * e.batch;
        const int brows = (int)(e.N - row0 < e.batch ? e.N - row0 : e.batch);
        ppo_batch(p, wl, act, ppo_lds, buf, io, row0, brows, g, e.batch_out + (rep * e.nb + k) * 3);
        const MlpAdamStep t = mlp_adam_step(P, e.adam, e.adam.step0 + k + 1);
        for (int i = A + threadIdx.x; i < P; i += kMlpThreads) adam_one(wl[i], g[i], m[i], v[i], t.a, t.bias_correction1, t.bias_correction2_sqrt);
        __syncthreads();
    }
    for (int i = A + threadIdx.x; i < P; i += kMlpThreads) e.params[rep * P + i] = wl[i];
    if (p.onchip)
        for (int i = A + threadIdx.x; i < P; i += kMlpThreads) { e.m[rep * P + i] = m[i]; e.v[rep * P + i] = v[i]; }
}

}  // namespace dsg
