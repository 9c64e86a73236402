// Reverse-step update with the predicted solution clipped to label bounds (dsg_set_xstart_clip, steps.with_clip).
//
// Every step reads its row {s, ia, a, is} of the handle's clip table and the bounds lo / hi [D] (through a device block written per
// call, as the history rows are) and runs update_body (dsg_kernels.hpp) with CLIP on: for element i of feature f = i % D, with e the
// guided eps of the step (plane 0 on a one-pass step),
//     x0 = (y - s * e) * ia
//     xc = min(max(x0, lo[f]), hi[f])
//     e' = (xc == x0 || x0 is NaN) ? e : (y - a * xc) * is
// in float32; the update, the history term, rec_eps and the renorm then see e'.  The rule is written with the intrinsics of the body around
// it, which this toolchain compiles as plain operators: a product is contracted into the sum or difference that follows it (y - s * e
// is one v_fma_f32), so a moved element matches a separately rounded evaluation to float32 rounding, not to the bit.  An element
// whose prediction lies inside its bounds keeps e to the bit, so infinite bounds give the bits of the form without a clip.
// Six forms, one per form of the update without a clip: plain, SCHED, VAR, VAR + SCHED (the variants of a call share one clip), HIST and
// HIST + SCHED.  The streams of y are those of the form without a clip: the bounds are D floats.
#pragma once
#include "dsg_kernels.hpp"

namespace dsg {

__global__ __launch_bounds__(256) void k_update_clip(const UpdateArgs a, const ClipParams* __restrict__ clpp) {
    update_body<false, false, false, true>(a, nullptr, nullptr, nullptr, nullptr, clpp);
}
__global__ __launch_bounds__(256) void k_update_clip_sched(const UpdateArgs a, const float* const* __restrict__ gpp, const ClipParams* __restrict__ clpp) {
    update_body<false, true, false, true>(a, nullptr, gpp, nullptr, nullptr, clpp);
}
__global__ __launch_bounds__(256) void k_update_clip_var(const UpdateArgs a, const VarParams* __restrict__ vpp, const ClipParams* __restrict__ clpp) {
    update_body<true, false, false, true>(a, vpp, nullptr, nullptr, nullptr, clpp);
}
__global__ __launch_bounds__(256) void k_update_clip_var_sched(const UpdateArgs a, const VarParams* __restrict__ vpp, const float* const* __restrict__ gpp,
                                                               const ClipParams* __restrict__ clpp) {
    update_body<true, true, false, true>(a, vpp, gpp, nullptr, nullptr, clpp);
}
__global__ __launch_bounds__(256) void k_update_clip_hist(const UpdateArgs a, float* __restrict__ hist, const float* const* __restrict__ hpp,
                                                          const ClipParams* __restrict__ clpp) {
    update_body<false, false, true, true>(a, nullptr, nullptr, hist, hpp, clpp);
}
__global__ __launch_bounds__(256) void k_update_clip_hist_sched(const UpdateArgs a, const float* const* __restrict__ gpp, float* __restrict__ hist,
                                                                const float* const* __restrict__ hpp, const ClipParams* __restrict__ clpp) {
    update_body<false, true, true, true>(a, nullptr, gpp, hist, hpp, clpp);
}

}  // namespace dsg
