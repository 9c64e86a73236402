// AttentionBlock of UNet1D (reference: ddpm_opt/UNetCF.py:98-157) on a sequence of length 1 -- gfx950 device code.
//
// The block is called on (batch, 1, d) with n_heads = 1, d_k = d.  The softmax runs over a single key and is identically 1, so
// q and k never reach the output; `norm` is registered but never called.  What remains, with Wv / bv = rows 2d:3d of
// `projection` and Wo / bo = `output`:
//
//     v   = Wv x + bv
//     out = Wo v + bo + x
//
// computed in exactly this order (two GEMMs, then the residual add; never a pre-multiplied I + Wo Wv, which rounds differently).
// In the fragment layout of dsg_kernels.hpp the accumulator of the first GEMM is, register for register, the B operand of the
// second, so v never leaves the registers; the residual comes from the input tile that was loaded for the first GEMM.  The
// epilogue is the Linear one (linear_store): the output tile and its LayerNorm statistics, which the next block's norm1 reads.
//
// Arithmetic (dsg_set_precision): >= 64 wide the default is the split-f16 three-MFMA form of dsg_split.hpp (k_attn_h: both operands of
// both products are RAW residual-stream values -- x from its producer's statistics, v from its own -- so both are range-checked exactly
// as the Linear shortcuts' operand is, and the handle's range flag is raised above fp16's range); DSG_PRECISION_F32_MFMA and every
// narrow width run k_attn on v_mfma_f32_32x32x2_f32 (exact float32), which is what the per-operator narrow Linears of the exact path
// use.  The backward kernel is exact float32 in both modes.
//
// Backward (training):  dv = Wo^T dy,  dx = dy + Wv^T dv.  dv is stored: the grouped weight-gradient launch reads it as the G
// operand of d projection.weight[2d:3d] = dv^T x, as it reads dy for d output.weight = dy^T v (v is saved by the training forward).
#pragma once
#include "dsg_kernels.hpp"
#include "dsg_split.hpp"

namespace dsg {

struct AttnArgs {
    LinArgs l;            // in (fragment), out / out_stats, out_width = in_width = d, ntiles, tiles_per_pass
    const float* Wv;      // packed [NT][KG][256]: rows 2d:3d of projection.weight
    const float* bv;      // padded NT*32
    const float* Wo;      // packed [NT][KG][256]
    const float* bo;      // padded NT*32
    float* save_v;        // training: v in fragment layout [tiles][KG][64][4], or null
    // split-f16 form (k_attn_h, >= 64 wide): hi / lo planes [NT][KG/2][2][64] and max|W| of the tensors they were scaled by
    const uint4* Wvh; const uint4* Woh;
    const float* mv;      // max|projection.weight| (the whole tensor: the pack scales the v rows by the same word)
    const float* mo;      // max|output.weight|
};

template <int NT>
__device__ __forceinline__ void attn_body(const AttnArgs& a, const int tile, const int lane) {
    const int h = lane >> 5;
    const int KG = a.l.in_groups;                 // d / 8 groups in and out
    const size_t nt_stride = (size_t)KG * 256;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);

    // the input tile: B operand of the first GEMM and the residual of the epilogue
    float4 x[NT * 4];
    const float* xp = a.l.in.data + (size_t)tile * KG * 256 + lane * 4;
#pragma unroll
    for (int G = 0; G < NT * 4; ++G) x[G] = G < KG ? ld4(xp + (size_t)G * 256) : z4;

    f32x16 v[NT];
    acc_init<NT>(v, a.bv, h);
    {
        float4 wn[NT];
        load_wfrag<NT>(wn, a.Wv + lane * 4, nt_stride);
#pragma unroll
        for (int G = 0; G < NT * 4; ++G) {
            if (G < KG) {
                float4 wc[NT];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) wc[nt] = wn[nt];
                if (G + 1 < KG) load_wfrag<NT>(wn, a.Wv + (size_t)(G + 1) * 256 + lane * 4, nt_stride);
                __builtin_amdgcn_sched_barrier(0);  // keep the prefetch ABOVE this group's MFMAs
                mfma_group<NT>(v, wc, x[G].x, x[G].y, x[G].z, x[G].w);
            }
        }
    }
    if (a.save_v) {
#pragma unroll
        for (int G = 0; G < NT * 4; ++G)
            if (G < KG)
                st4(a.save_v + ((size_t)tile * KG + G) * 256 + lane * 4,
                    make_float4(v[G >> 2][4 * (G & 3)], v[G >> 2][4 * (G & 3) + 1], v[G >> 2][4 * (G & 3) + 2], v[G >> 2][4 * (G & 3) + 3]));
    }

    f32x16 o[NT];
    acc_init<NT>(o, a.bo, h);
    {
        float4 wn[NT];
        load_wfrag<NT>(wn, a.Wo + lane * 4, nt_stride);
#pragma unroll
        for (int G = 0; G < NT * 4; ++G) {
            if (G < KG) {
                float4 wc[NT];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) wc[nt] = wn[nt];
                if (G + 1 < KG) load_wfrag<NT>(wn, a.Wo + (size_t)(G + 1) * 256 + lane * 4, nt_stride);
                __builtin_amdgcn_sched_barrier(0);
                mfma_group<NT>(o, wc, v[G >> 2][4 * (G & 3)], v[G >> 2][4 * (G & 3) + 1], v[G >> 2][4 * (G & 3) + 2], v[G >> 2][4 * (G & 3) + 3]);
            }
        }
    }
    // res += x (UNetCF.py:152): after both products
#pragma unroll
    for (int G = 0; G < NT * 4; ++G) {
        o[G >> 2][4 * (G & 3) + 0] += x[G].x; o[G >> 2][4 * (G & 3) + 1] += x[G].y;
        o[G >> 2][4 * (G & 3) + 2] += x[G].z; o[G >> 2][4 * (G & 3) + 3] += x[G].w;
    }
    linear_store<NT, OUT_FRAG>(a.l, tile, lane, o);
}

template <int NT>
__global__ __launch_bounds__(256, NT >= 4 ? 2 : 4) void k_attn(const AttnArgs a) {
    const int lane = threadIdx.x & 63;
    const int tile = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));  // wave-uniform: SGPR address math
    if (tile >= a.l.ntiles) return;
    attn_body<NT>(a, tile, lane);
}

// The same operator on the f16 matrix cores: x = hi + lo per operand, three MFMAs per k16-step, float32 accumulation (dsg_split.hpp).
// N = 32 NT in {64, 128}.  The products are un-scaled by 2^-e of the weight's pack scale with the bias added in the same fma.
template <int NT>
__global__ __launch_bounds__(256, 2) void k_attn_h(const AttnArgs a) {
    const int lane = threadIdx.x & 63, h = lane >> 5, j = lane & 31;
    const int tile = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    if (tile >= a.l.ntiles) return;
    const int KG = a.l.in_groups;                 // = 4 NT
    const size_t nt_stride = (size_t)((KG + 1) >> 1) * 128;
    {   // raw operand x: bounded by its producer's row statistics, as the Linear shortcuts do
        const float2 s = reinterpret_cast<const float2*>(a.l.in.stats)[(size_t)tile * 32 + j];
        range_check(a.l.range_flag, s.x, s.y);
    }
    f32x16 x[NT];
    const float* xp = a.l.in.data + (size_t)tile * KG * 256 + lane * 4;
#pragma unroll
    for (int G = 0; G < NT * 4; ++G) {
        const float4 t = ld4(xp + (size_t)G * 256);
        x[G >> 2][4 * (G & 3)] = t.x; x[G >> 2][4 * (G & 3) + 1] = t.y; x[G >> 2][4 * (G & 3) + 2] = t.z; x[G >> 2][4 * (G & 3) + 3] = t.w;
    }
    f32x16 v[NT];
    chain_raw_from_reg_h<NT, NT, true>(v, x, KG, a.Wvh, nt_stride, lane);
    acc_unscale_add<NT>(v, ldexpf(1.0f / kRawScale, -scale_exp(*a.mv)), a.bv, h);
    if (a.save_v) {
#pragma unroll
        for (int G = 0; G < NT * 4; ++G)
            st4(a.save_v + ((size_t)tile * KG + G) * 256 + lane * 4,
                make_float4(v[G >> 2][4 * (G & 3)], v[G >> 2][4 * (G & 3) + 1], v[G >> 2][4 * (G & 3) + 2], v[G >> 2][4 * (G & 3) + 3]));
    }
    {   // raw operand v: its own row statistics
        float vm, vq;
        acc_stats<NT * 32, NT>(v, h, vm, vq);
        range_check(a.l.range_flag, vm, vq);
    }
    f32x16 o[NT];
    chain_raw_from_reg_h<NT, NT, true>(o, v, KG, a.Woh, nt_stride, lane);
    acc_unscale_add<NT>(o, ldexpf(1.0f / kRawScale, -scale_exp(*a.mo)), a.bo, h);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) o[nt] += x[nt];        // res += x, after both products
    linear_store<NT, OUT_FRAG>(a.l, tile, lane, o);
}

struct AttnBwdArgs {
    const float* gout_a;     // [tiles][KG][256]: gradient of the block's output from the chain consumer
    const float* gout_b;     // ... from the skip consumer, or null
    const float* WoT;        // packed transposes [NT][KG][256]
    const float* WvT;
    float* dv;               // [tiles][KG][256]: Wo^T dy, the G operand of the projection's weight gradient
    float* gin;              // [tiles][KG][256]: gradient slot of the producer (the residual block in front)
    int groups;              // d / 8
    int ntiles;
};

template <int NT>
__global__ __launch_bounds__(256, 2) void k_attn_bwd(const AttnBwdArgs a) {
    const int lane = threadIdx.x & 63;
    const int tile = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    if (tile >= a.ntiles) return;
    const int KG = a.groups;
    const size_t nt_stride = (size_t)KG * 256;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 dy[NT * 4];
#pragma unroll
    for (int G = 0; G < NT * 4; ++G) {
        dy[G] = z4;
        if (G < KG) {
            dy[G] = ld4(a.gout_a + ((size_t)tile * KG + G) * 256 + lane * 4);
            if (a.gout_b) {
                const float4 gb = ld4(a.gout_b + ((size_t)tile * KG + G) * 256 + lane * 4);
                dy[G].x += gb.x; dy[G].y += gb.y; dy[G].z += gb.z; dy[G].w += gb.w;
            }
        }
    }
    f32x16 dv[NT], dx[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dv[nt][r] = 0.f; dx[nt][r] = 0.f; }
#pragma unroll
    for (int G = 0; G < NT * 4; ++G) {
        if (G < KG) {
            float4 w[NT];
            load_wfrag<NT>(w, a.WoT + (size_t)G * 256 + lane * 4, nt_stride);
            mfma_group<NT>(dv, w, dy[G].x, dy[G].y, dy[G].z, dy[G].w);
        }
    }
#pragma unroll
    for (int G = 0; G < NT * 4; ++G)
        if (G < KG)
            st4(a.dv + ((size_t)tile * KG + G) * 256 + lane * 4,
                make_float4(dv[G >> 2][4 * (G & 3)], dv[G >> 2][4 * (G & 3) + 1], dv[G >> 2][4 * (G & 3) + 2], dv[G >> 2][4 * (G & 3) + 3]));
#pragma unroll
    for (int G = 0; G < NT * 4; ++G) {
        if (G < KG) {
            float4 w[NT];
            load_wfrag<NT>(w, a.WvT + (size_t)G * 256 + lane * 4, nt_stride);
            mfma_group<NT>(dx, w, dv[G >> 2][4 * (G & 3)], dv[G >> 2][4 * (G & 3) + 1], dv[G >> 2][4 * (G & 3) + 2], dv[G >> 2][4 * (G & 3) + 3]);
        }
    }
    // dx = dy + Wv^T (Wo^T dy)
#pragma unroll
    for (int G = 0; G < NT * 4; ++G)
        if (G < KG)
            st4(a.gin + ((size_t)tile * KG + G) * 256 + lane * 4,
                make_float4(dx[G >> 2][4 * (G & 3)] + dy[G].x, dx[G >> 2][4 * (G & 3) + 1] + dy[G].y, dx[G >> 2][4 * (G & 3) + 2] + dy[G].z,
                            dx[G >> 2][4 * (G & 3) + 3] + dy[G].w));
}

}  // namespace dsg
