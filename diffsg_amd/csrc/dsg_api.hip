// Host side of libdiffsg_hip.so: builds the operator plan of UNet1D (UNetCF.py:262-356), owns the packed-weight
// arena and the fragment-layout workspaces, and enqueues the kernels of dsg_kernels.hpp / dsg_train.hpp.
// C ABI: include/diffsg.h.
#include "dsg_kernels.hpp"
#include "dsg_train.hpp"
#include "dsg_split.hpp"
#include "dsg_wide.hpp"
#include "dsg_panel.hpp"
#include "dsg_res64.hpp"
#include "dsg_tile.hpp"
#include "dsg_attn.hpp"
#include "dsg_train_split.hpp"
#include "dsg_eval.hpp"
#include "dsg_best.hpp"
#include "dsg_labelgen.hpp"
#include "dsg_cogen.hpp"
#include "dsg_nugen.hpp"
#include "dsg_mlp.hpp"
#include "dsg_ppo.hpp"
#include "dsg_gd.hpp"
#include "dsg_multistep.hpp"
#include "dsg_clip.hpp"
#include "dsg_own.hpp"
#include "../../include/diffsg.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <algorithm>
#include <type_traits>
#include <utility>
#include <vector>

using namespace dsg;

#include "host_net.hpp"
#include "host_dispatch.hpp"
#include "host_forward.hpp"
#include "host_bind.hpp"
#include "host_train.hpp"
#include "host_sample.hpp"
#include "host_aux.hpp"

extern "C" {

const char* dsg_last_error(void) { return g_err.c_str(); }

#ifndef DSG_BUILD_ID_STR
#define DSG_BUILD_ID_STR "unknown"
#endif
// "DSG_BUILD_ID=<sha256 of the sources>": _lib.py compares it with the tree before loading (a stale binary must not pass tests)
const char* dsg_build_id(void) {
    static const char id[] = "DSG_BUILD_ID=" DSG_BUILD_ID_STR;
    return id + 13;
}

dsg_handle* dsg_create(const dsg_unet_desc* desc) { return create_impl(desc, nullptr, 0); }

dsg_handle* dsg_create_attn(const dsg_unet_desc* desc, const int* is_attn, int middle_attn) {
    if (desc && !is_attn && desc->n_res > 0) { fail("dsg_create_attn: null is_attn"); return nullptr; }
    return create_impl(desc, is_attn, middle_attn);
}

void dsg_destroy(dsg_handle* h) {
    if (!h) return;
    (void)hipDeviceSynchronize();
    delete h;
}

int dsg_param_count(const dsg_handle* h) { return h ? (int)h->params.size() : 0; }
unsigned long long dsg_generation(const dsg_handle* h) { return h ? h->generation : 0ull; }
const char* dsg_param_name(const dsg_handle* h, int i) {
    return (h && i >= 0 && i < (int)h->params.size()) ? h->params[i].name.c_str() : "";
}
long long dsg_param_numel(const dsg_handle* h, int i) {
    return (h && i >= 0 && i < (int)h->params.size()) ? h->params[i].numel : -1;
}
long long dsg_param_total(const dsg_handle* h) { return h ? h->total_params : 0; }

int dsg_bind_weights(dsg_handle* h, const float* const* ptrs, int n, void* stream) {
    if (!h) return fail("null handle");
    if (n != (int)h->params.size()) return fail("dsg_bind_weights: got %d pointers, the model has %d tensors", n, (int)h->params.size());
    for (int i = 0; i < n; ++i)
        if (!ptrs[i]) return fail("dsg_bind_weights: null pointer for %s", h->params[i].name.c_str());
    hipStream_t s = (hipStream_t)stream;
    const bool same = h->bound && h->bound_ptrs.size() == (size_t)n && memcmp(h->bound_ptrs.data(), ptrs, n * sizeof(float*)) == 0;
    if (!same) {
        // (re)build the pack descriptor table: ONE grouped launch re-packs everything after each optimizer step.
        // The tables below are rewritten with synchronous copies: kernels of an earlier call on `s` (a non-blocking stream
        // does not order with them) may still be reading the old ones
        HIPCK(hipStreamSynchronize(s));
        for (int i = 0; i < n; ++i) h->params[i].ptr = ptrs[i];
        h->bound_ptrs.assign(ptrs, ptrs + n);
        if (h->v8_lo >= 0 && bind_v8_image(h)) return 1;
        std::vector<PackDesc> pd;
        std::vector<TimeBlockDesc> td;
        const long long blk = build_pack_table(h, pd, td);
        if (build_plane_tables(h) || build_time_rows(h)) return 1;
        if (!h->pack_dev) HIPCK(h->pack_dev.alloc(pd.size()));
        h->pack_n = (int)pd.size();
        h->pack_blocks = blk;
        HIPCK(hipMemcpyAsync(h->pack_dev, pd.data(), pd.size() * sizeof(PackDesc), hipMemcpyHostToDevice, s));
        HIPCK(hipMemcpyAsync(h->tdesc_dev, td.data(), td.size() * sizeof(TimeBlockDesc), hipMemcpyHostToDevice, s));
        HIPCK(hipStreamSynchronize(s));  // pd / td are host temporaries
    }
    // (k_pack_grouped also clears the max|W| words for k_maxabs, and behind them the word "weights outside the split envelope" of the
    // previous bind; its grid of >= (params + 1) / 256 blocks covers them)
    if ((long long)h->pack_blocks * 256 < (long long)h->params.size() + 1) return fail("internal: pack grid smaller than the parameter table");
    hipLaunchKernelGGL(k_pack_grouped, dim3((unsigned)h->pack_blocks), dim3(256), 0, s, h->pack_dev, h->pack_n, h->maxabs, (int)h->params.size() + 1);
    if (h->mx_n) {
        // max|W| of every split-packed weight -> maxabs[param index]; the pack and the block kernels derive the same
        // power-of-two scale from it on the device (no host round trip); k_pack_h also writes the operators' un-scale constants
        hipLaunchKernelGGL(k_maxabs, dim3(h->mx_n, kMaxabsSlices), dim3(256), 0, s, h->mx_ptrs_dev, h->mx_numel_dev, h->mx_idx_dev, h->maxabs);
        const int nopc = (int)(h->res.size() + h->lin.size());
        if ((long long)h->packh_blocks * 256 < nopc || (long long)h->packh_blocks * 256 < h->env_n)
            return fail("internal: plane-pack grid smaller than the operator table");
        hipLaunchKernelGGL(k_pack_h, dim3((unsigned)h->packh_blocks), dim3(256), 0, s, h->packh_dev, h->packh_n, (const float*)h->maxabs,
                           (const OpConstDesc*)h->opc_desc_dev, nopc, h->opc_dev, (const EnvDesc*)h->env_dev, h->env_n, h->env_word());
    }
    // the LDS image of the narrow run (k_fused_narrow_lds) is a COPY of arena pieces: re-gather it from the planes packed above,
    // into the same buffer (cached graphs keep its pointer) -- otherwise sample() after an optimizer step, load_state_dict or an
    // EMA swap would run the narrow run on the previous weights while every other block uses the new ones
    if (h->v8_ncopies > 0)      // first: the LDS image below takes the section from this buffer
        hipLaunchKernelGGL(k_narrow_image_build, dim3((unsigned)h->v8_ncopies), dim3(64), 0, s, (const NarrowLdsCopy*)h->v8_copies_dev,
                           reinterpret_cast<uint4*>(h->v8_image.get()));
    for (auto& t : h->tabs)     // both resident sets (the one-pass context's image is a copy of its own)
        if (t.nlds_image && t.nlds_ncopies > 0)
            hipLaunchKernelGGL(k_narrow_image_build, dim3((unsigned)t.nlds_ncopies), dim3(256), 0, s, (const NarrowLdsCopy*)t.nlds_copies_dev, t.nlds_image);
    HIPCK(hipGetLastError());
    h->bound = true;
    return 0;
}

// The settings / status entry points synchronise and free graphs on the HANDLE's device, whatever device is current in the calling
// thread (a model on cuda:1 queried while cuda:0 was current synchronised the wrong device and could read the range
// flag before the sampling kernels had finished).
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(const dsg_handle* h) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != h->device) (void)hipSetDevice(h->device); else prev = -1;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

int dsg_set_precision(dsg_handle* h, int mode) {
    if (!h) return fail("null handle");
    DeviceGuard dg(h);
    if (mode != DSG_PRECISION_SPLIT_F16 && mode != DSG_PRECISION_F32_MFMA) return fail("unknown precision mode %d", mode);
    const bool split = mode == DSG_PRECISION_SPLIT_F16;
    if (split != h->use_split) { (void)hipDeviceSynchronize(); free_graphs(h); h->use_split = split; ++h->generation; }
    return 0;
}

int dsg_set_renorm_hook(dsg_handle* h, double* stats3, void (*reduce)(void*), void* user) {
    if (!h) return fail("null handle");
    if (reduce && !stats3) return fail("dsg_set_renorm_hook: a reduce function needs the 3-double device buffer");
    // the cached step graphs never contain the hook branch (enqueue_step is captured with use_hook = false and neither the
    // callback nor `stats3` is baked into a node), so they stay valid across installs and removals: no synchronise, no re-capture
    h->renorm_stats = stats3; h->renorm_fn = reduce; h->renorm_user = user;
    return 0;
}

int dsg_set_step_grid(dsg_handle* h, const float* t_host, int n, int renorm_steps) {
    if (!h) return fail("null handle");
    if (n < 0) return fail("dsg_set_step_grid: n = %d is negative", n);
    if (!t_host || n == 0) { h->grid_n = 0; return 0; }     // nothing is overwritten: an enqueued call keeps reading the buffer
    if (renorm_steps < -1 || renorm_steps > n) return fail("dsg_set_step_grid: renorm_steps = %d is outside -1 .. n = %d", renorm_steps, n);
    DeviceGuard dg(h);
    // an enqueued call may still copy the old grid; the step graphs do not depend on it and stay
    HIPCK(hipDeviceSynchronize());
    if (n > h->grid_cap) {
        h->grid_n = 0; h->grid_cap = 0;
        HIPCK(h->grid_dev.alloc((size_t)n));
        h->grid_cap = n;
    }
    HIPCK(hipMemcpy(h->grid_dev, t_host, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    h->grid_n = n;
    h->grid_renorm = renorm_steps < 0 ? (n < 4 ? n : 4) : renorm_steps;
    return 0;
}

int dsg_set_step_guidance(dsg_handle* h, const float* g_host, int n) {
    if (!h) return fail("null handle");
    if (n < 0) return fail("dsg_set_step_guidance: n = %d is negative", n);
    if (!g_host || n == 0) { h->guid_n = 0; return 0; }     // nothing is overwritten: an enqueued call keeps reading the buffer
    for (int j = 0; j < n; ++j)
        if (!(g_host[j] >= 0.f && g_host[j] <= 3.402823466e38f))     // NaN fails the first comparison, +inf the second
            return fail("dsg_set_step_guidance: weight %d is %g: the weights are finite and >= 0", j, (double)g_host[j]);
    DeviceGuard dg(h);
    // an enqueued call may still read the old weights; the step graphs hold neither the buffer nor the values and stay
    HIPCK(hipDeviceSynchronize());
    if (!h->guid_call) HIPCK(h->guid_call.alloc(1));
    if (n > h->guid_cap) {      // the new buffer first: a failed allocation leaves the schedule the handle holds as it was
        DevBuf<float> grown;
        HIPCK(grown.alloc((size_t)n));
        h->guid_dev = std::move(grown);
        h->guid_cap = n;
    }
    HIPCK(hipMemcpy(h->guid_dev, g_host, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    h->guid_host.assign(g_host, g_host + n);
    h->guid_n = n;
    return 0;
}

int dsg_set_step_history(dsg_handle* h, const float* hist_host, int n) {
    if (!h) return fail("null handle");
    if (n < 0) return fail("dsg_set_step_history: n = %d is negative", n);
    if (!hist_host || n == 0) { h->hist_n = 0; return 0; }     // nothing is overwritten: an enqueued call keeps reading the buffer
    for (int j = 0; j < 3 * n; ++j)
        if (!(fabsf(hist_host[j]) <= 3.402823466e38f))            // NaN and the infinities fail the comparison
            return fail("dsg_set_step_history: row %d holds %g: the rows {m, p, q} are finite", j / 3, (double)hist_host[j]);
    auto stores = [&](int j) { return hist_host[3 * j + 1] != 0.f || hist_host[3 * j + 2] != 0.f; };
    if (hist_host[3 * (n - 1)] != 0.f)
        return fail("dsg_set_step_history: row %d, the first step of a call, has m = %g: there is no history to read yet", n - 1,
                    (double)hist_host[3 * (n - 1)]);
    for (int j = 0; j + 1 < n; ++j)
        if (hist_host[3 * j] != 0.f && !stores(j + 1))
            return fail("dsg_set_step_history: row %d reads the history (m = %g) but row %d, the step before it, stores none (p = q = 0)", j,
                        (double)hist_host[3 * j], j + 1);
    DeviceGuard dg(h);
    // an enqueued call may still read the old rows; the step graphs hold neither the buffer nor the values and stay
    HIPCK(hipDeviceSynchronize());
    if (!h->hist_call) HIPCK(h->hist_call.alloc(1));
    if (n > h->hist_cap) {      // the new buffer first: a failed allocation leaves the table the handle holds as it was
        DevBuf<float> grown;
        HIPCK(grown.alloc((size_t)3 * n));
        h->hist_dev = std::move(grown);
        h->hist_cap = n;
    }
    HIPCK(hipMemcpy(h->hist_dev, hist_host, (size_t)3 * n * sizeof(float), hipMemcpyHostToDevice));
    h->hist_n = n;
    return 0;
}

int dsg_set_xstart_clip(dsg_handle* h, const float* lo_host, const float* hi_host, int D, const float* x0_host, int n) {
    if (!h) return fail("null handle");
    if (n < 0) return fail("dsg_set_xstart_clip: n = %d is negative", n);
    if (!lo_host || !hi_host || n == 0) { h->clip_n = 0; return 0; }     // nothing is overwritten: an enqueued call keeps reading the buffers
    if (D != h->d.input_dim) return fail("dsg_set_xstart_clip: D = %d bounds, the net has input_dim = %d", D, h->d.input_dim);
    if (!x0_host) return fail("dsg_set_xstart_clip: null pointer to the rows {s, ia, a, is}");
    for (int f = 0; f < D; ++f) {
        if (lo_host[f] != lo_host[f] || hi_host[f] != hi_host[f])
            return fail("dsg_set_xstart_clip: feature %d has the bounds [%g, %g]: a bound is a number or an infinity, not a NaN", f, (double)lo_host[f],
                        (double)hi_host[f]);
        if (lo_host[f] > hi_host[f])
            return fail("dsg_set_xstart_clip: feature %d has lo = %g above hi = %g", f, (double)lo_host[f], (double)hi_host[f]);
    }
    for (int j = 0; j < 4 * n; ++j)
        if (!(x0_host[j] > 0.f && x0_host[j] <= 3.402823466e38f))     // NaN fails the first comparison, +inf the second
            return fail("dsg_set_xstart_clip: row %d holds %g: the rows {s, ia, a, is} are finite and > 0", j / 4, (double)x0_host[j]);
    DeviceGuard dg(h);
    // an enqueued call may still read the old bounds and rows; the step graphs hold neither the buffers nor the values and stay
    HIPCK(hipDeviceSynchronize());
    // staged in buffers of their own and swapped in whole (D + n floats, on a call that synchronises anyway): a failed allocation or copy
    // leaves the clip the handle holds as it was
    DevBuf<ClipParams> call;
    DevBuf<float> bounds, rows;
    if (!h->clip_call) HIPCK(call.alloc(1));
    HIPCK(bounds.alloc((size_t)2 * D));
    HIPCK(rows.alloc((size_t)4 * n));
    HIPCK(hipMemcpy(bounds, lo_host, (size_t)D * sizeof(float), hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(bounds.get() + D, hi_host, (size_t)D * sizeof(float), hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(rows, x0_host, (size_t)4 * n * sizeof(float), hipMemcpyHostToDevice));
    if (call) h->clip_call = std::move(call);
    h->clip_bounds = std::move(bounds);
    h->clip_rows = std::move(rows);
    h->clip_n = n;
    return 0;
}

int dsg_set_train_law(dsg_handle* h, const unsigned* cdf24_host, const float* weight_host, int T) {
    if (!h) return fail("null handle");
    if (T < 0) return fail("dsg_set_train_law: T = %d is negative", T);
    if ((!cdf24_host && !weight_host) || T == 0) {     // nothing is overwritten: an enqueued step keeps reading the buffers
        if (h->law_T) { h->law_T = 0; h->law_has_cdf = h->law_has_w = false; ++h->generation; }
        return 0;
    }
    if (cdf24_host) {
        for (int k = 1; k < T; ++k)
            if (cdf24_host[k] < cdf24_host[k - 1])
                return fail("dsg_set_train_law: the CDF decreases at step %d (%u after %u)", k, cdf24_host[k], cdf24_host[k - 1]);
        if (cdf24_host[T - 1] != (1u << 24))
            return fail("dsg_set_train_law: the last CDF entry is %u, not 2^24 = %u", cdf24_host[T - 1], 1u << 24);
    }
    if (weight_host)
        for (int k = 0; k < T; ++k)
            if (!(weight_host[k] >= 0.f && weight_host[k] <= 3.402823466e38f))     // NaN fails the first comparison, +inf the second
                return fail("dsg_set_train_law: weight %d is %g: the weights are finite and >= 0", k, (double)weight_host[k]);
    DeviceGuard dg(h);
    // an enqueued step may still read the old law
    HIPCK(hipDeviceSynchronize());
    if (T > h->law_cap) {       // the new buffers first: a failed allocation leaves the law the handle holds as it was
        DevBuf<unsigned> c;
        DevBuf<float> w;
        HIPCK(c.alloc((size_t)T));
        HIPCK(w.alloc((size_t)T));
        h->law_cdf = std::move(c); h->law_w = std::move(w);
        h->law_cap = T;
    }
    if (cdf24_host) HIPCK(hipMemcpy(h->law_cdf, cdf24_host, (size_t)T * sizeof(unsigned), hipMemcpyHostToDevice));
    if (weight_host) HIPCK(hipMemcpy(h->law_w, weight_host, (size_t)T * sizeof(float), hipMemcpyHostToDevice));
    h->law_T = T; h->law_has_cdf = cdf24_host != nullptr; h->law_has_w = weight_host != nullptr;
    ++h->generation;            // a captured step holds the kernel forms and the buffers of the law it was captured under
    return 0;
}

int dsg_set_train_report(dsg_handle* h, double* sq_dev, long long* rows_dev, int T) {
    if (!h) return fail("null handle");
    if (T < 0) return fail("dsg_set_train_report: T = %d is negative", T);
    if (!sq_dev || T == 0) {
        if (h->rep_T) { h->rep_T = 0; h->rep_sq = nullptr; h->rep_rows = nullptr; ++h->generation; }
        return 0;
    }
    if (!rows_dev) return fail("dsg_set_train_report: sq_dev without rows_dev");
    if (h->rep_T != T || h->rep_sq != sq_dev || h->rep_rows != rows_dev) {
        h->rep_sq = sq_dev; h->rep_rows = rows_dev; h->rep_T = T;
        ++h->generation;        // a captured step holds the report launch and the caller's two addresses
    }
    return 0;
}

int dsg_set_chunk_variants(dsg_handle* h, const float* omega_host, const int* renorm_host, const int* table_host, int chunks, int tables) {
    if (!h) return fail("null handle");
    if (chunks < 0) return fail("dsg_set_chunk_variants: chunks = %d is negative", chunks);
    if (!omega_host || chunks == 0) { h->var_chunks = 0; return 0; }     // nothing is overwritten: an enqueued call keeps reading the buffers
    if (tables < 1) return fail("dsg_set_chunk_variants: tables = %d, at least one coefficient table is needed", tables);
    for (int c = 0; c < chunks; ++c) {
        if (table_host && (table_host[c] < 0 || table_host[c] >= tables))
            return fail("dsg_set_chunk_variants: chunk %d names table %d, outside 0 .. %d", c, table_host[c], tables - 1);
        if (renorm_host && renorm_host[c] < 0) return fail("dsg_set_chunk_variants: chunk %d has a negative renorm count (%d)", c, renorm_host[c]);
    }
    DeviceGuard dg(h);
    // an enqueued call may still read the old values; the step graphs of the variant form do not hold these buffers and stay
    HIPCK(hipDeviceSynchronize());
    if (!h->var_call) HIPCK(h->var_call.alloc(1));
    if (chunks > h->var_cap) {
        h->var_chunks = 0; h->var_cap = 0;
        HIPCK(h->var_omega.alloc((size_t)chunks));
        HIPCK(h->var_renorm.alloc((size_t)chunks));
        HIPCK(h->var_table.alloc((size_t)chunks));
        h->var_cap = chunks;
    }
    HIPCK(hipMemcpy(h->var_omega, omega_host, (size_t)chunks * sizeof(float), hipMemcpyHostToDevice));
    if (renorm_host) HIPCK(hipMemcpy(h->var_renorm, renorm_host, (size_t)chunks * sizeof(int), hipMemcpyHostToDevice));
    if (table_host) HIPCK(hipMemcpy(h->var_table, table_host, (size_t)chunks * sizeof(int), hipMemcpyHostToDevice));
    h->var_renorm_host.clear();
    if (renorm_host) h->var_renorm_host.assign(renorm_host, renorm_host + chunks);
    h->var_has_renorm = renorm_host != nullptr; h->var_has_table = table_host != nullptr;
    h->var_chunks = chunks; h->var_tables = tables;
    return 0;
}

int dsg_set_option(dsg_handle* h, int option, int value) {
    if (!h) return fail("null handle");
    DeviceGuard dg(h);
    switch (option) {
        case DSG_OPT_NARROW_VALU8:
            if ((value != 0) != h->opt_v8) {
                (void)hipDeviceSynchronize();
                free_graphs(h);                 // the captured narrow-run launches hold the plan made under the other setting
                for (auto& t : h->tabs) t.fused_sig.valid = false;
                h->opt_v8 = value != 0;
                ++h->generation;
            }
            return 0;
        case DSG_OPT_TRAIN_TIME_BESIDE:
            if ((value != 0) != h->opt_time_beside) { h->opt_time_beside = value != 0; ++h->generation; }
            return 0;
        case DSG_OPT_PANEL_HALF:
            if ((value != 0) != h->opt_panel_half) { (void)hipDeviceSynchronize(); free_graphs(h); h->opt_panel_half = value != 0; ++h->generation; }
            return 0;
        case DSG_OPT_CFG_SHARE:
            if ((value != 0) != h->opt_cfg_share) { (void)hipDeviceSynchronize(); free_graphs(h); h->opt_cfg_share = value != 0; ++h->generation; }
            return 0;
        case DSG_OPT_F32_PAIR:
            if ((value != 0) != h->opt_f32_pair) { (void)hipDeviceSynchronize(); free_graphs(h); h->opt_f32_pair = value != 0; ++h->generation; }
            return 0;
        case DSG_OPT_TILE_STEP:
            if ((value != 0) != h->opt_tile) { (void)hipDeviceSynchronize(); free_graphs(h); h->opt_tile = value != 0; ++h->generation; }
            return 0;
        case DSG_OPT_WGRAD_NARROW_PART:
            if ((value != 0) != h->opt_wg_narrow_part) { (void)hipDeviceSynchronize(); h->opt_wg_narrow_part = value != 0; h->td_valid = false; ++h->generation; }
            return 0;
        default: return fail("dsg_set_option: unknown option %d", option);
    }
}

int dsg_range_status(dsg_handle* h, int* exceeded) {
    if (!h || !exceeded) return fail("dsg_range_status: null argument");
    DeviceGuard dg(h);
    HIPCK(hipDeviceSynchronize());
    float env = 0.f;
    HIPCK(hipMemcpy(exceeded, h->range_flag, sizeof(int), hipMemcpyDeviceToHost));
    HIPCK(hipMemcpy(&env, h->env_word(), sizeof(float), hipMemcpyDeviceToHost));
    if (*exceeded) HIPCK(hipMemset(h->range_flag, 0, sizeof(int)));
    // (the weights matter to the split path alone: under DSG_PRECISION_F32_MFMA the handle has nothing to report about them)
    // (and before the first bind the word has not been written)
    *exceeded = (*exceeded ? DSG_RANGE_ACTIVATION : 0) | (env != 0.f && h->use_split && h->bound ? DSG_RANGE_WEIGHTS : 0);
    return 0;
}

int dsg_range_status_stream(dsg_handle* h, int* exceeded, void* stream) {
    if (!h || !exceeded) return fail("dsg_range_status_stream: null argument");
    DeviceGuard dg(h);
    hipStream_t s = (hipStream_t)stream;
    // Read AND clear in one step, on `s`: a one-thread kernel exchanges the flag with 0 and writes what it found into a pinned word (ADVICE r5:
    // "copy, then memset" lost a flag raised between the two by kernels of another stream -- twin handles, the side stream).  The pinned word
    // belongs to the handle; the copy is truly asynchronous and only `s` is waited for.
    if (!h->range_pinned) HIPCK(h->range_pinned.alloc(1));
    hipLaunchKernelGGL(k_flag_take, dim3(1), dim3(64), 0, s, h->range_flag, (const float*)h->env_word(), h->range_pinned);
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(s));
    *exceeded = *h->range_pinned & (h->use_split && h->bound ? ~0 : ~DSG_RANGE_WEIGHTS);     // as in dsg_range_status
    return 0;
}

int dsg_set_launch_policy(dsg_handle* h, int coop_max_tiles, int narrow_small_max_tiles) {
    if (!h) return fail("null handle");
    DeviceGuard dg(h);
    const int c = coop_max_tiles < 0 ? kCoopMaxTilesDefault : coop_max_tiles;
    const int n = narrow_small_max_tiles < 0 ? kNarrowSmallMaxTilesDefault : narrow_small_max_tiles;
    if (c != h->coop_max_tiles || n != h->narrow_small_max_tiles) {
        (void)hipDeviceSynchronize();
        free_graphs(h);                 // the captured step graphs hold the kernel forms chosen at capture time
        h->coop_max_tiles = c; h->narrow_small_max_tiles = n;
        h->panel_min_tiles = c == 0 ? 0 : kPanelMinTilesDefault;
        ++h->generation;
    }
    return 0;
}

int dsg_reserve(dsg_handle* h, int max_rows, int max_entries) {
    if (!h) return fail("null handle");
    return ensure_workspace(h, max_rows, max_entries);
}

int dsg_unet_forward(dsg_handle* h, const float* x, const float* t, const float* cond, const float* cond_mask, float* out,
                     int B, void* stream) {
    if (check_bound(h)) return 1;
    if (B < 1) return fail("B must be >= 1");
    if (ensure_workspace(h, B, B)) return 1;
    hipStream_t s = (hipStream_t)stream;
    HIPCK(hipMemcpyAsync(h->fw.tvals, t, (size_t)B * sizeof(float), hipMemcpyDeviceToDevice, s));
    run_time_path(h, B, s);
    const int tpp = cdiv(B, 32), CG = groups_of(h->d.cond_dim);
    hipLaunchKernelGGL(k_cond_frag, dim3(cdiv(tpp * CG * 256, 256)), dim3(256), 0, s, cond, cond_mask, B, h->d.cond_dim, CG,
                       h->fw.condfrag, tpp, h->use_split ? h->range_flag : nullptr, kCondLimit);
    // the handle's precision mode applies here as in dsg_sample / dsg_train_step: the split kernels take the condition embedding
    // Wc silu(cond * mask) precomputed (a masked row contributes exactly 0), the exact-f32 kernels compute it in the block
    if (h->use_split) run_cond_embed(h, B, s);
    RunCtx c{B, 1, 0, x, out, nullptr, h->fw.ts_ident, false, h->use_split};
    if (prepare_fused(h, c, s)) return 1;
    run_unet(h, c, s);
    HIPCK(hipGetLastError());
    return 0;
}

int dsg_sample_rec(dsg_handle* h, const float* cond, const float* y_T, const float* noise, unsigned long long seed, float omega,
                   const float* coef, int T, float* out, int B, int flags, float* rec_y, float* rec_eps, void* stream) {
    return sample_impl(h, cond, y_T, noise, seed, nullptr, 0, omega, coef, T, out, B, flags, rec_y, rec_eps, (hipStream_t)stream);
}

int dsg_sample(dsg_handle* h, const float* cond, const float* y_T, const float* noise, unsigned long long seed, float omega,
               const float* coef, int T, float* out, int B, int flags, void* stream) {
    return dsg_sample_rec(h, cond, y_T, noise, seed, omega, coef, T, out, B, flags, nullptr, nullptr, stream);
}

int dsg_sample_chunked(dsg_handle* h, const float* cond, const float* y_T, const float* noise, const unsigned long long* seeds, int chunk_rows,
                       float omega, const float* coef, int T, float* out, int B, int flags, void* stream) {
    if (chunk_rows < 1) return fail("dsg_sample_chunked: chunk_rows must be >= 1");
    return sample_impl(h, cond, y_T, noise, seeds ? seeds[0] : 0ull, seeds, chunk_rows, omega, coef, T, out, B, flags, nullptr, nullptr, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------------
// training step
// ------------------------------------------------------------------------------------------------------
int dsg_train_step(dsg_handle* h, const float* y, const float* cond, const int* ts, const float* noise, const float* cond_mask,
                   const float* sqrt_acp, const float* sqrt_1m_acp, int T, float* grads_flat, float* loss_out, int B, void* stream) {
    if (check_bound(h)) return 1;
    if (B < 1 || T < 1) return fail("B and T must be >= 1");
    if (!y || !cond || !ts || !noise || !sqrt_acp || !sqrt_1m_acp || !grads_flat || !loss_out)
        return fail("dsg_train_step: null pointer argument");
    if (train_law_refused(h, "dsg_train_step", T)) return 1;
    if (ensure_train_workspace(h, B, T)) return 1;
    return train_step_impl(h, y, cond, ts, noise, cond_mask, sqrt_acp, sqrt_1m_acp, T, grads_flat, loss_out, B, (hipStream_t)stream);
}

int dsg_train_draws(unsigned long long seed, unsigned long long call, int T, float keep_prob, int B, int D, int* ts, float* noise,
                    float* cond_mask, void* stream) {
    if (B < 1 || D < 1 || T < 1) return fail("dsg_train_draws: B, D and T must be >= 1");
    if (call >> 30) return fail("dsg_train_draws: call counter out of range (2^30)");
    const size_t blocks = (((size_t)B * D + 3) / 4 + 255) / 256;
    const unsigned grid = (unsigned)(blocks < 4096 ? blocks : 4096);
    hipLaunchKernelGGL(k_train_draws, dim3(grid), dim3(256), 0, (hipStream_t)stream, ts, noise, cond_mask, B, D, T, keep_prob, seed, (unsigned)call,
                       (const unsigned long long*)nullptr);
    HIPCK(hipGetLastError());
    return 0;
}

int dsg_train_step_seeded_dyn(dsg_handle* h, const float* y, const float* cond, unsigned long long seed, unsigned long long* call_dev,
                              float keep_prob, const float* sqrt_acp, const float* sqrt_1m_acp, int T, float* grads_flat, float* loss_out,
                              int B, void* stream) {
    if (check_bound(h)) return 1;
    if (B < 1 || T < 1) return fail("B and T must be >= 1");
    if (!y || !cond || !call_dev || !sqrt_acp || !sqrt_1m_acp || !grads_flat || !loss_out) return fail("dsg_train_step_seeded_dyn: null pointer argument");
    if (train_law_refused(h, "dsg_train_step_seeded_dyn", T)) return 1;
    if (ensure_train_workspace(h, B, T)) return 1;
    const int D = h->d.input_dim;
    if (ensure_train_draws(h)) return 1;
    hipStream_t s = (hipStream_t)stream;
    // every refusal of train_step_impl comes FIRST: a refused call enqueues nothing, so *call_dev stays where it was (the tables built here
    // are the ones train_step_impl then finds current)
    if (train_shape_refused(h) || build_train_descs(h, B, T, s)) return 1;
    launch_train_draws(h, B, D, T, keep_prob, seed, 0u, (const unsigned long long*)call_dev, s);
    hipLaunchKernelGGL(k_bump_u64, dim3(1), dim3(64), 0, s, call_dev);
    HIPCK(hipGetLastError());
    return train_step_impl(h, y, cond, h->tr.ts, h->tr.noise, h->tr.mask, sqrt_acp, sqrt_1m_acp, T, grads_flat, loss_out, B, s);
}

int dsg_train_step_seeded(dsg_handle* h, const float* y, const float* cond, unsigned long long seed, unsigned long long call,
                          float keep_prob, const float* sqrt_acp, const float* sqrt_1m_acp, int T, float* grads_flat, float* loss_out,
                          int B, void* stream) {
    if (check_bound(h)) return 1;
    if (B < 1 || T < 1) return fail("B and T must be >= 1");
    if (!y || !cond || !sqrt_acp || !sqrt_1m_acp || !grads_flat || !loss_out) return fail("dsg_train_step_seeded: null pointer argument");
    if (train_law_refused(h, "dsg_train_step_seeded", T)) return 1;
    if (ensure_train_workspace(h, B, T)) return 1;
    const int D = h->d.input_dim;
    if (ensure_train_draws(h)) return 1;
    // ts goes straight into the workspace copy the step reads (train_step_impl skips its own copy when handed that pointer)
    if (h->law_T && h->law_has_cdf) {       // the law's draw (dsg_set_train_law): the same refusal, then the second kernel
        if (call >> 30) return fail("dsg_train_draws: call counter out of range (2^30)");
        launch_train_draws(h, B, D, T, keep_prob, seed, (unsigned)call, nullptr, (hipStream_t)stream);
        HIPCK(hipGetLastError());
    } else if (dsg_train_draws(seed, call, T, keep_prob, B, D, h->tr.ts, h->tr.noise, h->tr.mask, stream)) return 1;
    return train_step_impl(h, y, cond, h->tr.ts, h->tr.noise, h->tr.mask, sqrt_acp, sqrt_1m_acp, T, grads_flat, loss_out, B, (hipStream_t)stream);
}

int dsg_train_profile_enable(dsg_handle* h, int on) {
    if (!h) return fail("null handle");
    if (on && !h->tev[0])
        for (auto& e : h->tev) HIPCK(hipEventCreate(e.put()));
    h->train_prof = on != 0;
    h->tev_valid = false;
    return 0;
}

int dsg_train_profile(dsg_handle* h, float* ms5) {
    if (!h || !ms5) return fail("dsg_train_profile: null argument");
    if (!h->tev_valid) return fail("dsg_train_profile: no profiled dsg_train_step yet (dsg_train_profile_enable first)");
    HIPCK(hipEventSynchronize(h->tev[5]));
    for (int i = 0; i < 5; ++i) HIPCK(hipEventElapsedTime(&ms5[i], h->tev[i], h->tev[i + 1]));
    return 0;
}

int dsg_adam_step(float* p, const float* g, float* exp_avg, float* exp_avg_sq, long long n, double lr, double beta1, double beta2, double eps,
                  double weight_decay, int maximize, long long step, void* stream) {
    if (!p || !g || !exp_avg || !exp_avg_sq || n < 0 || step < 1) return fail("dsg_adam_step: bad arguments");
    if (n == 0) return 0;
    if ((reinterpret_cast<unsigned long long>(p) | reinterpret_cast<unsigned long long>(g) | reinterpret_cast<unsigned long long>(exp_avg) |
         reinterpret_cast<unsigned long long>(exp_avg_sq)) & 15ull)
        return fail("dsg_adam_step: the four buffers must be 16-byte aligned");
    const AdamArgs a{p, g, exp_avg, exp_avg_sq, (size_t)n, lr, beta1, beta2, weight_decay, eps, (float)step, maximize, nullptr, nullptr};
    const long long pieces = (n / 4 + 255) / 256;
    const unsigned blocks = (unsigned)(pieces < 1 ? 1 : (pieces < 2048 ? pieces : 2048));
    hipLaunchKernelGGL(k_adam, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
    HIPCK(hipGetLastError());
    return 0;
}

int dsg_adam_step_dyn(float* p, const float* g, float* exp_avg, float* exp_avg_sq, long long n, const double* lr_dev, double beta1, double beta2,
                      double eps, double weight_decay, int maximize, float* step_dev, void* stream) {
    if (!p || !g || !exp_avg || !exp_avg_sq || !lr_dev || !step_dev || n < 0) return fail("dsg_adam_step_dyn: bad arguments");
    if (n == 0) return 0;
    if ((reinterpret_cast<unsigned long long>(p) | reinterpret_cast<unsigned long long>(g) | reinterpret_cast<unsigned long long>(exp_avg) |
         reinterpret_cast<unsigned long long>(exp_avg_sq)) & 15ull)
        return fail("dsg_adam_step_dyn: the four buffers must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_bump_f32, dim3(1), dim3(64), 0, s, step_dev);          // the count AFTER this update, as dsg_adam_step is handed it
    const AdamArgs a{p, g, exp_avg, exp_avg_sq, (size_t)n, 0.0, beta1, beta2, weight_decay, eps, 0.f, maximize, lr_dev, step_dev};
    const long long pieces = (n / 4 + 255) / 256;
    const unsigned blocks = (unsigned)(pieces < 1 ? 1 : (pieces < 2048 ? pieces : 2048));
    hipLaunchKernelGGL(k_adam, dim3(blocks), dim3(256), 0, s, a);
    HIPCK(hipGetLastError());
    return 0;
}

int dsg_ema_update(float* avg, const float* p, float decay, float one_minus_decay, long long n, void* stream) {
    if (!avg || !p || n < 0) return fail("dsg_ema_update: bad arguments");
    if (n == 0) return 0;
    const unsigned blocks = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(k_ema, dim3(blocks), dim3(256), 0, (hipStream_t)stream, avg, p, decay, one_minus_decay, (size_t)n);
    HIPCK(hipGetLastError());
    return 0;
}


int dsg_row_softmax(const float* y, float* out, long long rows, int D, void* stream) {
    if (eval_args(y, out, rows, D, "dsg_row_softmax")) return 1;
    return softmax_rows<0>(y, out, rows, D, (hipStream_t)stream, 0, D);
}
int dsg_msr_decode(const float* y, float* out, long long rows, int D, void* stream) {
    if (eval_args(y, out, rows, D, "dsg_msr_decode")) return 1;
    return softmax_rows<1>(y, out, rows, D, (hipStream_t)stream, 0, D);
}
int dsg_co_decode(const float* y, float* out, long long rows, int D, void* stream) {
    if (eval_args(y, out, rows, D, "dsg_co_decode")) return 1;
    return softmax_rows<2>(y, out, rows, D, (hipStream_t)stream, 0, D);
}
int dsg_msr_rate(const float* p, const float* gain, float* rate, long long rows, int D, void* stream) {
    if (eval_args(p, gain, rows, D, "dsg_msr_rate") || !rate) return fail("dsg_msr_rate: bad arguments");
    if (rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (D <= 8) hipLaunchKernelGGL((k_msr_rate<1>), dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, p, gain, rate, rows, D);
    else if (D <= 160) hipLaunchKernelGGL((k_msr_rate<16>), dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, s, p, gain, rate, rows, D);
    else hipLaunchKernelGGL((k_msr_rate<64>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, p, gain, rate, rows, D);
    HIPCK(hipGetLastError());
    return 0;
}
int dsg_co_cost(const float* X, const float* Y, float* cost, long long rows, int n, void* stream) {
    if (eval_args(X, Y, rows, n, "dsg_co_cost") || !cost) return fail("dsg_co_cost: bad arguments");
    if (rows == 0) return 0;
    hipLaunchKernelGGL(k_co_cost, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, X, Y, cost, rows, n);
    HIPCK(hipGetLastError());
    return 0;
}
int dsg_nu_decode(const float* y, float* out, long long rows, int D, float width, float height, float p_sum, void* stream) {
    if (eval_args(y, out, rows, D, "dsg_nu_decode")) return 1;
    if (D < 3) return fail("dsg_nu_decode: D = %d (two position columns and at least one power column)", D);
    if (rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    StreamScratch<float2> part;
    if (minmax_global(y, rows, D, 0, 2, part, s)) return 1;
    hipLaunchKernelGGL(k_nu_decode, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, y, out, rows, D, width, height, p_sum, part.get());
    HIPCK(hipGetLastError());
    return 0;
}
int dsg_nu_rate(const float* Yd, const float* X, float* rate, long long rows, int K, void* stream) {
    if (eval_args(Yd, X, rows, K, "dsg_nu_rate") || !rate) return fail("dsg_nu_rate: bad arguments");
    if (K > kNuMaxUsers) return fail("dsg_nu_rate: K = %d users (at most %d)", K, kNuMaxUsers);
    if (rows == 0) return 0;
    hipLaunchKernelGGL(k_nu_rate, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, Yd, X, rate, rows, K);
    HIPCK(hipGetLastError());
    return 0;
}

// Best of n rounds per condition (dsg_best.hpp): one statistics pass (MSR / NU), one selection launch.
int dsg_best_of(int problem, const float* Y, const float* X, int n, long long B, int D, const float* params, float* solution,
                float* objective, int* round, float* objectives, int accumulate, int round0, void* stream) {
    if (problem < DSG_PROBLEM_MSR || problem > DSG_PROBLEM_NU) return fail("dsg_best_of: problem = %d (DSG_PROBLEM_MSR / _CO / _NU)", problem);
    if (B < 0 || D < 1 || n < 0 || round0 < 0 || (problem != DSG_PROBLEM_CO && !params)) return fail("dsg_best_of: bad arguments");
    if ((long long)n * B > 2147483647LL) return fail("dsg_best_of: n * B = %lld candidate rows (at most 2^31 - 1)", (long long)n * B);
    if (problem == DSG_PROBLEM_NU && D < 3) return fail("dsg_best_of: NU with D = %d (two position columns and at least one power column)", D);
    if (problem == DSG_PROBLEM_NU && D - 2 > kNuMaxUsers) return fail("dsg_best_of: NU with K = %d users (at most %d)", D - 2, kNuMaxUsers);
    if (problem == DSG_PROBLEM_MSR && D > 64 * kSoftEpl) return fail("dsg_best_of: MSR rows of D = %d (at most %d)", D, 64 * kSoftEpl);
    if (problem == DSG_PROBLEM_CO && D > kSoftEpl) return fail("dsg_best_of: CO rows of D = %d nodes (at most %d)", D, kSoftEpl);
    if (B == 0 || n == 0) return 0;
    if (eval_args(Y, X, B, D, "dsg_best_of") || !solution || !objective || !round) return fail("dsg_best_of: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    StreamScratch<float2> scratch;                    // [n] per-round (min, max), then the partials [n][nparts]
    if (problem != DSG_PROBLEM_CO) {
        const int c0 = 0, c1 = problem == DSG_PROBLEM_MSR ? D : 2;
        const int w = c1 - c0, lpr = w >= 64 ? 64 : (w >= 16 ? 16 : (w >= 4 ? 4 : 1));
        const long long want = (B + 4LL * (64 / lpr) - 1) / (4LL * (64 / lpr));
        const int nparts = (int)(want < kEvalParts ? want : kEvalParts);
        HIPCK(scratch.alloc((size_t)n * (1 + nparts), s));
        const unsigned gy = (unsigned)(n < 65535 ? n : 65535);
        hipLaunchKernelGGL(k_best_minmax_partial, dim3(nparts, gy), dim3(256), 0, s, Y, n, B, D, c0, c1, scratch + n);
        hipLaunchKernelGGL(k_best_minmax_final, dim3(gy), dim3(256), 0, s, scratch + n, n, nparts, scratch.get());
    }
    auto grid = [&](int lpr) { const long long rpb = 4LL * (64 / lpr); return dim3((unsigned)((B + rpb - 1) / rpb)); };
#define DSG_BEST_MSR(L, Q) hipLaunchKernelGGL((k_best_msr<L, Q>), grid(L), dim3(256), 0, s, Y, X, n, B, D, params[0], scratch.get(), solution, \
                                              objective, round, objectives, accumulate, round0)
    if (problem == DSG_PROBLEM_MSR) {
        // lanes per row = k_row_softmax's for this D; Q = k_msr_rate's lanes per row over that (see k_best_msr)
        if (D <= 8) DSG_BEST_MSR(1, 1);
        else if (D <= kSoftEpl) DSG_BEST_MSR(1, 16);
        else if (D <= 4 * kSoftEpl) DSG_BEST_MSR(4, 4);
        else if (D <= 160) DSG_BEST_MSR(16, 1);
        else if (D <= 16 * kSoftEpl) DSG_BEST_MSR(16, 4);
        else DSG_BEST_MSR(64, 1);
    } else if (problem == DSG_PROBLEM_CO) {
        hipLaunchKernelGGL(k_best_co, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, Y, X, n, B, D, solution, objective, round, objectives,
                           accumulate, round0);
    } else {
        hipLaunchKernelGGL(k_best_nu, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, Y, X, n, B, D, params[0], params[1], params[2], scratch.get(),
                           solution, objective, round, objectives, accumulate, round0);
    }
#undef DSG_BEST_MSR
    HIPCK(hipGetLastError());
    return 0;
}

int dsg_sum_rate_gen(const double* gs, double* schemes, double* rates, long long rows, int M, double W, void* stream) {
    if (!gs || !schemes || !rates || rows < 0 || M < 1) return fail("dsg_sum_rate_gen: bad arguments");
    if (M > kSrMaxM) return fail("dsg_sum_rate_gen: M = %d channels (at most %d)", M, kSrMaxM);
    if (rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int kMaxIter = 149;                       // the reference leaves its loop when k reaches 150
    StreamScratch<int> flags;
    HIPCK(flags.alloc(kMaxIter + 3, s));
    HIPCK(hipMemsetAsync(flags, 0, (kMaxIter + 3) * sizeof(int), s));
    HIPCK(hipMemsetAsync(flags, 1, 1, s));          // flags[0] = 1 (low byte): the dry pass always runs
    const long long n = rows * M;
    hipLaunchKernelGGL(k_sumrate_init, dim3((unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096)), dim3(256), 0, s, schemes, n, W / M);
    const dim3 grid((unsigned)((rows + 3) / 4));
    const double eps = 0.001;
    double beta = 0.1;
    hipLaunchKernelGGL(k_sumrate_iter, grid, dim3(256), 0, s, gs, schemes, rows, M, 0.0, eps, flags.get(), flags + 1, 1);
    int k = 1;
    for (int it = 1; it <= kMaxIter; ++it) {
        hipLaunchKernelGGL(k_sumrate_iter, grid, dim3(256), 0, s, gs, schemes, rows, M, beta, eps, flags + it, flags + it + 1, 0);
        ++k;
        if (k % 20 == 0) beta *= 0.5;
        if (k == 150) break;
    }
    hipLaunchKernelGGL(k_sumrate_rates, grid, dim3(256), 0, s, gs, schemes, rates, rows, M);
    HIPCK(hipGetLastError());
    return 0;
}

int dsg_co_minlp_search(const double* params, const double* choices, int nch, double* Y, int* tolerable, long long rows, int n,
                        double F_t, double P_t, double P_I, double theta, void* stream) {
    if (!params || !choices || !Y || !tolerable) return fail("dsg_co_minlp_search: null pointer argument");
    if (n < 1 || n > kCoMaxNodes) return fail("dsg_co_minlp_search: node_num must be in [1, %d] (got %d)", kCoMaxNodes, n);
    if (nch < 1 || nch > 4096) return fail("dsg_co_minlp_search: bad grid size %d", nch);
    if (rows < 0 || rows > 0x7fffffffLL) return fail("dsg_co_minlp_search: bad row count");
    if (rows == 0) return 0;
    const CoGenConst cc{F_t, P_t, P_I, theta};
    hipLaunchKernelGGL(k_co_minlp, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, params, choices, nch, n, cc, Y, tolerable);
    HIPCK(hipGetLastError());
    return 0;
}

int dsg_noma_uav_search(const double* qs, const double* fs, int nfs, double* out, long long rows, double sigma_sq, double rou_0,
                        double H, void* stream) {
    if (!qs || !fs || !out) return fail("dsg_noma_uav_search: null pointer argument");
    if (nfs < 3 || nfs > kNuMaxSolutions) return fail("dsg_noma_uav_search: nfs = %d table rows (must be in [3, %d])", nfs, kNuMaxSolutions);
    if (rows < 0 || rows > 0x7fffffffLL) return fail("dsg_noma_uav_search: bad row count");
    if (rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    // small calls: short point runs, so that one sample still fills many CUs; large calls: long runs, fewer idle lanes at
    // the end of each workgroup's list
    const int tile_pts = rows < 64 ? 256 : kNuMaxTile;
    const int tiles = (kNuGridPts + tile_pts - 1) / tile_pts;
    const long long chunk = std::min<long long>(rows, 16384);   // pass-1 grid: chunk * tiles workgroups (< 2^32 work-items)
    StreamScratch<double> scratch;                   // [chunk * tiles] best rates, then as many keys
    HIPCK(scratch.alloc((size_t)chunk * tiles * 2, s));
    double* best_rate = scratch;
    unsigned long long* best_key = reinterpret_cast<unsigned long long*>(best_rate + chunk * tiles);
    const NuGenConst cc{sigma_sq, rou_0, H};
    for (long long r0 = 0; r0 < rows; r0 += chunk) {
        const long long n = std::min(chunk, rows - r0);
        hipLaunchKernelGGL(k_nu_tiles, dim3((unsigned)(n * tiles)), dim3(kNuThreads), 0, s, qs + r0 * 6, fs, nfs, cc, tile_pts, tiles,
                           best_rate, best_key);
        hipLaunchKernelGGL(k_nu_pick, dim3((unsigned)n), dim3(kNuThreads), 0, s, qs + r0 * 6, fs, cc, tiles, best_rate, best_key,
                           out + r0 * 6);
    }
    HIPCK(hipGetLastError());
    return 0;
}

int dsg_op_count(const dsg_handle* h) { return h ? (int)h->ops.size() : 0; }

int dsg_fused_range(const dsg_handle* h, int* lo, int* hi) {
    if (!h) return fail("null handle");
    const bool on = h->fuse_hi - h->fuse_lo >= 2;
    if (lo) *lo = on ? h->fuse_lo : 0;
    if (hi) *hi = on ? h->fuse_hi : 0;
    return 0;
}

int dsg_op_profile(const dsg_handle* h, int op, double* ms_total, int* calls) {
    if (!h || op < 0 || op >= (int)h->op_ms.size()) return fail("dsg_op_profile: no profile for op %d (run dsg_sample with DSG_SAMPLE_PROFILE)", op);
    if (ms_total) *ms_total = h->op_ms[op];
    if (calls) *calls = h->op_calls[op];
    return 0;
}

int dsg_op_info(const dsg_handle* h, int op, char* name, double* flops_per_row, double* bytes_per_row) {
    if (!h || op < 0 || op >= (int)h->ops.size()) return fail("bad op index");
    const Op& o = h->ops[op];
    double macs2 = 0, macs_cond = 0, bytes = 0;  // macs2: both passes; macs_cond: conditional pass only
    if (o.kind == OP_RES) {
        const ResP& r = h->res[o.p];
        const int in = r.in0 + r.in1;
        macs2 = (double)in * r.N + 2.0 * r.N * r.N + (r.sclin ? (double)in * r.N : 0.0);
        macs_cond = (double)h->d.cond_dim * r.N;
        bytes = 2.0 * 4.0 * (in + r.N);
    } else if (o.kind == OP_ATTN) {
        const double d = h->attn[o.p].N;
        macs2 = 2.0 * d * d;
        bytes = 2.0 * 4.0 * (d + d);
    } else {
        const LinOpP& l = h->lin[o.p];
        macs2 = (double)l.l.K * l.l.N;
        bytes = 2.0 * 4.0 * (l.l.K + l.l.N);
    }
    if (name) { strncpy(name, o.name.c_str(), 63); name[63] = 0; }
    (void)macs_cond;  // hoisted out of the step: the condition embeddings are computed once per dsg_sample call
    if (flops_per_row) *flops_per_row = 2.0 * (2.0 * macs2);
    if (bytes_per_row) *bytes_per_row = bytes;
    return 0;
}

int dsg_time_op(dsg_handle* h, int op, int B, int iters, float* ms_avg, void* stream) {
    if (check_bound(h)) return 1;
    if (op < 0 || op >= (int)h->ops.size() || iters < 1 || !ms_avg) return fail("dsg_time_op: bad arguments");
    if (ensure_workspace(h, B, 1)) return 1;
    hipStream_t s = (hipStream_t)stream;
    const int zero = 0;
    HIPCK(hipMemcpyAsync(h->step_dev, &zero, sizeof(int), hipMemcpyHostToDevice, s));
    RunCtx c{B, 2, cdiv(B, 32), h->fw.ywork, h->fw.eps, h->step_dev, nullptr, false, true};
    if (narrow_singles(h, c) && prepare_fused(h, c, s)) return 1;     // exact path: the single-operator table of this context
    Event e0, e1;
    HIPCK(hipEventCreate(e0.put()));
    HIPCK(hipEventCreate(e1.put()));
    launch_op(h, h->ops[op], c, s);  // warm-up
    HIPCK(hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i) launch_op(h, h->ops[op], c, s);
    HIPCK(hipEventRecord(e1, s));
    HIPCK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCK(hipEventElapsedTime(&ms, e0, e1));
    *ms_avg = ms / iters;
    return 0;
}

// ---- box calibration (bench.py `box`): the pool's MI355X boxes differ by up to 15 % on the same binary (clock under load), so a
// headline alone cannot tell a slow box from a slow tree.  Three fixed probes, timed with HIP events on `stream`, median of 5 launches
// of ~5 ms each (a 1-ms probe read 1 816 and 1 564 TFLOP/s on one box a second apart: the clock had not settled):
//   out[0] mfma_tflops  every SIMD issues dependent v_mfma_f32_32x32x16_f16 back to back on non-trivial operands (two waves per SIMD):
//                       the bare matrix pipe at the clock the box holds under it;
//   out[1] mix_gslots   the same loop with six vector instructions (one of them transcendental) behind every MFMA -- the instruction mix
//                       of the block kernels -- in 1e9 (MFMA + 6 vector) slots per second over the chip;
//   out[2] copy_gbs     a 256 MiB float4 copy inside a buffer allocated for the call (read + written bytes per second);
//   out[3] panel_gslots the frozen miniature of the panel kernels' load profile (k_calib_panel), 1e9 MFMA slots per second.
int dsg_box_calibrate(float* out3 /* four floats */, void* stream) {
    if (!out3) return fail("dsg_box_calibrate: null output");
    hipStream_t s = (hipStream_t)stream;
    hipDeviceProp_t prop;
    int devid = 0;
    HIPCK(hipGetDevice(&devid));
    HIPCK(hipGetDeviceProperties(&prop, devid));
    const int cus = prop.multiProcessorCount;
    Event e0, e1;           // owners: every early return below (a failed 512 MiB allocation beside a large batch) frees what exists
    DevBuf<float> sink;
    const size_t copy_bytes = (size_t)256 << 20;
    DevBuf<char> buf;
    HIPCK(hipEventCreate(e0.put()));
    HIPCK(hipEventCreate(e1.put()));
    HIPCK(sink.alloc((size_t)cus * 2 * 512));
    HIPCK(buf.alloc(2 * copy_bytes));
    hipLaunchKernelGGL(dsg::k_calib_fill, dim3(cus * 8), dim3(256), 0, s, reinterpret_cast<uint4*>(buf.get()), 2 * copy_bytes / 16);
    auto median5 = [&](auto&& launch, float& ms_out) -> int {
        float t[6];
        for (int rep = 0; rep < 6; ++rep) {      // the first launch is a warm-up
            HIPCK(hipEventRecord(e0, s));
            launch();
            HIPCK(hipEventRecord(e1, s));
            HIPCK(hipEventSynchronize(e1));
            HIPCK(hipEventElapsedTime(&t[rep], e0, e1));
        }
        std::sort(t + 1, t + 6);
        ms_out = t[3];
        return 0;
    };
    // two workgroups of four waves per CU = two waves per SIMD, as the block kernels run
    const int it0 = 3072, it6 = 1536;             // x 48 MFMAs: ~5 ms each at two waves per SIMD
    float ms0 = 0.f, ms6 = 0.f, msc = 0.f;
    if (median5([&] { hipLaunchKernelGGL(dsg::k_calib_mfma<0>, dim3(2 * cus), dim3(256), 0, s, it0, sink.get()); }, ms0)) return 1;
    if (median5([&] { hipLaunchKernelGGL(dsg::k_calib_mfma<6>, dim3(2 * cus), dim3(256), 0, s, it6, sink.get()); }, ms6)) return 1;
    if (median5([&] { hipLaunchKernelGGL(dsg::k_calib_copy, dim3(cus * 8), dim3(256), 0, s, reinterpret_cast<const uint4*>(buf.get()),
                                         reinterpret_cast<uint4*>(buf + copy_bytes), copy_bytes / 16); }, msc)) return 1;
    out3[0] = (float)((double)cus * 8 * it0 * 48 * 32768.0 / (ms0 * 1e-3) / 1e12);
    out3[1] = (float)((double)cus * 8 * it6 * 48 / (ms6 * 1e-3) / 1e9);
    out3[2] = (float)(2.0 * copy_bytes / (msc * 1e-3) / 1e9);
    // out3[3]: the frozen miniature of the panel kernels' load profile (dsg_panel.hpp, k_calib_panel): one workgroup per CU, ~10 ms per
    // launch -- long enough for the clock to settle under it -- 1e9 MFMA slots per second over the chip
    {
        const int panels = 1536;
        float msp = 0.f;
        if (median5([&] { hipLaunchKernelGGL(dsg::k_calib_panel, dim3(cus), dim3(512), 0, s, reinterpret_cast<const uint4*>(buf.get()),
                                             reinterpret_cast<const uint4*>(buf + copy_bytes), copy_bytes / 16 - 1, panels, sink); }, msp)) return 1;
        out3[3] = (float)((double)cus * 8 * panels * 48 / (msp * 1e-3) / 1e9);
    }
    return 0;
}


int dsg_mlp_param_total(const dsg_mlp_desc* desc) {
    MlpPlan p;
    if (mlp_plan(desc, &p, false, "dsg_mlp_param_total")) return -1;
    return p.P;
}

int dsg_mlp_forward(const dsg_mlp_desc* desc, const float* params, const float* x, float* out, long long rows, void* stream) {
    MlpPlan p;
    if (mlp_plan(desc, &p, false, "dsg_mlp_forward")) return 1;
    if (rows < 0) return fail("dsg_mlp_forward: rows = %lld", rows);
    if (rows == 0) return 0;
    if (!params || !x || !out) return fail("dsg_mlp_forward: null argument");
    const long long ntiles = (rows + p.TR - 1) / p.TR;
    return baseline_launch(k_mlp_forward, ntiles < 2048 ? ntiles : 2048, p.lds_floats * 4, (hipStream_t)stream, {}, p, params, x, out, rows);
}

int dsg_mlp_loss_grad(const dsg_mlp_desc* desc, const float* params, const float* x, const float* y, long long rows, float* loss_out,
                      float* grad_flat, void* stream) {
    MlpPlan p;
    if (mlp_plan(desc, &p, false, "dsg_mlp_loss_grad")) return 1;
    if (rows < 0 || rows > 2147483647LL / kMlpMaxIO) return fail("dsg_mlp_loss_grad: rows = %lld (0 .. %lld)", rows, 2147483647LL / kMlpMaxIO);
    if (rows == 0) return 0;
    if (!params || !x || !y || !loss_out || !grad_flat) return fail("dsg_mlp_loss_grad: null argument");
    return baseline_launch(k_mlp_loss_grad, 1, p.lds_floats * 4, (hipStream_t)stream, {}, p, params, x, y, (int)rows, loss_out, grad_flat);
}

int dsg_mlp_train_epoch(const dsg_mlp_desc* desc, float* params, float* exp_avg, float* exp_avg_sq, const float* X, const float* Y,
                        const int* perm, int N, int batch, double lr, double beta1, double beta2, double eps, long long step0, float* batch_loss,
                        int R, void* stream) {
    MlpPlan p;
    if (mlp_plan(desc, &p, true, "dsg_mlp_train_epoch")) return 1;
    if (epoch_args("dsg_mlp_train_epoch", N, batch, R, step0, kMlpMaxIO)) return 1;
    if (N == 0) return 0;
    if (!params || !exp_avg || !exp_avg_sq || !X || !Y || !perm || !batch_loss) return fail("dsg_mlp_train_epoch: null argument");
    hipStream_t s = (hipStream_t)stream;
    MlpEpochArgs e{params, exp_avg, exp_avg_sq, nullptr, X, Y, perm, batch_loss, N, batch, (int)(((long long)N + batch - 1) / batch),
                   {lr, beta1, beta2, eps, step0}};
    // nets whose gradient and moments do not fit in LDS: the gradient in stream-ordered scratch (as the evaluators' reductions)
    StreamScratch<float> gws;
    if (!p.onchip) { HIPCK(gws.alloc((size_t)R * p.P, s)); e.gws = gws; }
    return baseline_launch(k_mlp_epoch, R, p.lds_floats * 4, s, {&gws}, p, e);
}

int dsg_ppo_param_total(const dsg_ppo_desc* desc) {
    PpoPlan p;
    if (ppo_plan(desc, &p, false, "dsg_ppo_param_total", false)) return -1;
    return p.P;
}

int dsg_ppo_forward(const dsg_ppo_desc* desc, const float* params, const float* x, float* mu_out, float* value_out, long long rows,
                    void* stream) {
    PpoPlan p;
    if (ppo_plan(desc, &p, false, "dsg_ppo_forward", false)) return 1;
    if (rows < 0) return fail("dsg_ppo_forward: rows = %lld", rows);
    if (rows == 0) return 0;
    if (!params || !x || !mu_out || !value_out) return fail("dsg_ppo_forward: null argument");
    const long long ntiles = (rows + p.TR - 1) / p.TR;
    return baseline_launch(k_ppo_forward, ntiles < 2048 ? ntiles : 2048, p.lds_floats * 4, (hipStream_t)stream, {}, p, params, x, mu_out,
                           value_out, rows);
}

int dsg_ppo_loss_grad(const dsg_ppo_desc* desc, const float* params, const float* x, const float* y, const float* old_logp,
                      const float* noise, long long rows, float* out3, float* new_logp_out, float* reward_out, float* grad_flat,
                      void* stream) {
    PpoPlan p;
    if (ppo_plan(desc, &p, false, "dsg_ppo_loss_grad")) return 1;
    if (rows < 0 || rows > 2147483647LL / (2 * kMlpMaxIO + 2))
        return fail("dsg_ppo_loss_grad: rows = %lld (0 .. %lld)", rows, 2147483647LL / (2 * kMlpMaxIO + 2));
    if (rows == 0) return 0;
    if (!params || !x || !y || !old_logp || !noise || !out3 || !new_logp_out || !reward_out || !grad_flat)
        return fail("dsg_ppo_loss_grad: null argument");
    hipStream_t s = (hipStream_t)stream;
    const int buf_off = ppo_buf_off(p, rows);
    const int bytes = (buf_off >= 0 ? buf_off + (int)rows * (2 * p.A + 2) : p.lds_floats) * 4;
    StreamScratch<float> ws;
    if (buf_off < 0) HIPCK(ws.alloc((size_t)rows * (2 * p.A + 2), s));
    const PpoBatchIO io{x, y, old_logp, noise, nullptr, new_logp_out, reward_out, rows};
    return baseline_launch(k_ppo_loss_grad, 1, bytes, s, {&ws}, p, params, io, (int)rows, buf_off, ws.get(), out3, grad_flat);
}

int dsg_ppo_train_epoch(const dsg_ppo_desc* desc, float* params, float* exp_avg, float* exp_avg_sq, const float* X, const float* Y,
                        float* old_logp, const float* noise, const int* perm, int N, int batch, double lr, double beta1, double beta2,
                        double eps, long long step0, float* batch_out, int R, void* stream) {
    PpoPlan p;
    if (ppo_plan(desc, &p, true, "dsg_ppo_train_epoch")) return 1;
    if (epoch_args("dsg_ppo_train_epoch", N, batch, R, step0, 2 * kMlpMaxIO + 2)) return 1;
    if (N == 0) return 0;
    if (!params || !exp_avg || !exp_avg_sq || !X || !Y || !old_logp || !noise || !perm || !batch_out)
        return fail("dsg_ppo_train_epoch: null argument");
    hipStream_t s = (hipStream_t)stream;
    const int bufrows = batch < N ? batch : N;
    const int buf_off = ppo_buf_off(p, bufrows);
    PpoEpochArgs e{params, exp_avg, exp_avg_sq, nullptr, nullptr, X, Y, old_logp, noise, perm, batch_out, N, batch,
                   (int)(((long long)N + batch - 1) / batch), bufrows, buf_off, {lr, beta1, beta2, eps, step0}};
    const int bytes = (buf_off >= 0 ? buf_off + bufrows * (2 * p.A + 2) : p.lds_floats) * 4;
    // what does not fit in LDS lives in stream-ordered scratch: the gradient (with the moments in place) and / or the batch buffer
    StreamScratch<float> gws, bws;
    if (!p.onchip) { HIPCK(gws.alloc((size_t)R * p.P, s)); e.gws = gws; }
    if (buf_off < 0) { HIPCK(bws.alloc((size_t)R * bufrows * (2 * p.A + 2), s)); e.bufws = bws; }
    return baseline_launch(k_ppo_epoch, R, bytes, s, {&gws, &bws}, p, e);
}

}  // extern "C"

// ---- The gradient-descent baseline (dsg_gd.hpp): every iteration of a row in one launch.
namespace {
// What the three entry points check alike; D: state entries per row.
int gd_args(const char* who, const double* X, const double* Y, long long B, int iters, const double* rec, int rec_every) {
    if (B < 0 || B > 0x7fffffffLL) return fail("%s: B = %lld rows (0 .. 2^31 - 1)", who, B);
    if (iters < 0) return fail("%s: iters = %d", who, iters);
    if (rec_every < 0) return fail("%s: rec_every = %d", who, rec_every);
    if (rec && rec_every == 0) return fail("%s: a record buffer needs rec_every > 0", who);
    if (B > 0 && (!X || !Y)) return fail("%s: null argument", who);
    return 0;
}
long long gd_grid(long long lanes) { return (lanes + kGdThreads - 1) / kGdThreads; }
}  // namespace

extern "C" {

int dsg_gd_co(const double* X, double* Y, long long B, int n, int iters, double lr, double lambda1, double lambda2, double* rec,
              int rec_every, void* stream) {
    if (n < 1 || n > kGdCoMaxNodes) return fail("dsg_gd_co: n = %d nodes (1 .. %d)", n, kGdCoMaxNodes);
    if (gd_args("dsg_gd_co", X, Y, B, iters, rec, rec_every)) return 1;
    if (B == 0 || iters == 0) return 0;
    const GdRec r{rec, rec_every};
    hipStream_t s = (hipStream_t)stream;
    if (n <= 4) return baseline_launch(k_gd_co<4>, gd_grid(B), 0, s, {}, X, Y, B, n, iters, lr, lambda1, lambda2, r);
    if (n <= 8) return baseline_launch(k_gd_co<8>, gd_grid(B), 0, s, {}, X, Y, B, n, iters, lr, lambda1, lambda2, r);
    return baseline_launch(k_gd_co<16>, gd_grid(B), 0, s, {}, X, Y, B, n, iters, lr, lambda1, lambda2, r);
}

int dsg_gd_msr(const double* X, double* Y, long long B, int M, int iters, double lr, double* rec, int rec_every, void* stream) {
    if (M < 1 || M > kGdMsrMax) return fail("dsg_gd_msr: M = %d channels (1 .. %d)", M, kGdMsrMax);
    if (gd_args("dsg_gd_msr", X, Y, B, iters, rec, rec_every)) return 1;
    if (B == 0 || iters == 0) return 0;
    const GdRec r{rec, rec_every};
    hipStream_t s = (hipStream_t)stream;
    if (M <= kGdMsrSlots) return baseline_launch(k_gd_msr<1>, gd_grid(B), 0, s, {}, X, Y, B, M, iters, lr, r);
    return baseline_launch(k_gd_msr<kGdMsrLanes>, gd_grid(B * kGdMsrLanes), 0, s, {}, X, Y, B, M, iters, lr, r);
}

int dsg_gd_nu(const double* X, double* Y, long long B, int K, int iters, double lr, double p_ref, double* rec, int rec_every,
              void* stream) {
    if (K < 1 || K > kGdNuMaxUsers) return fail("dsg_gd_nu: K = %d users (1 .. %d)", K, kGdNuMaxUsers);
    if (gd_args("dsg_gd_nu", X, Y, B, iters, rec, rec_every)) return 1;
    if (B == 0 || iters == 0) return 0;
    const GdRec r{rec, rec_every};
    hipStream_t s = (hipStream_t)stream;
    if (K <= 4) return baseline_launch(k_gd_nu<4>, gd_grid(B), 0, s, {}, X, Y, B, K, iters, lr, p_ref, r);
    if (K <= 8) return baseline_launch(k_gd_nu<8>, gd_grid(B), 0, s, {}, X, Y, B, K, iters, lr, p_ref, r);
    if (K <= 16) return baseline_launch(k_gd_nu<16>, gd_grid(B), 0, s, {}, X, Y, B, K, iters, lr, p_ref, r);
    return baseline_launch(k_gd_nu<32>, gd_grid(B), 0, s, {}, X, Y, B, K, iters, lr, p_ref, r);
}

}  // extern "C"

#ifdef DSG_CYCLE_STAMPS
// measurement builds only (tools/cycle_stamps.sh): the stamps recorded since the last call, oldest first by slot
extern "C" int dsg_stamps_fetch(unsigned long long* out, int n) {
    int cnt = 0;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(&cnt, HIP_SYMBOL(dsg::dsg_stamp_n), sizeof(int)) != hipSuccess) return -1;
    if (cnt > 8192) cnt = 8192;
    if (cnt > n) cnt = n;
    if (cnt > 0 && hipMemcpyFromSymbol(out, HIP_SYMBOL(dsg::dsg_stamp_buf), (size_t)cnt * sizeof(unsigned long long)) != hipSuccess) return -1;
    const int zero = 0;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(dsg::dsg_stamp_n), &zero, sizeof(int));
    return cnt;
}
#endif

