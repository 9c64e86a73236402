// Reverse-step update with a history term: two-step solver plans (dsg_set_step_history, steps.dpmpp_2m).
//
// A float32 tensor `hist`, one value per element of y, lives in the forward workspace beside `ywork`.  Every step reads its row
// {m, p, q} of the handle's history table (through a device word written per call, as the guidance weights are) and runs update_body
// (dsg_kernels.hpp) with HIST on:
//     out      = m != 0 ? v + m * hist_old : v           v: the update without a history, noise included
//     hist_new = p * y_old + q * eps                      stored iff p != 0 || q != 0; eps: the guided eps (plane 0 on a one-pass step)
//     y <- out
// in explicit round-to-nearest operations, no contraction.  Both branches are uniform per launch, so a first-order step of a history plan
// moves the bytes of k_update / k_update_sched.  The renorm and the trajectory record act on `out`, rec_eps records eps.
// Two forms: plain and SCHED (a guidance schedule is held).  Chunk variants have no history form: sample_impl refuses the pair.
#pragma once
#include "dsg_kernels.hpp"

namespace dsg {

__global__ __launch_bounds__(256) void k_update_hist(const UpdateArgs a, float* __restrict__ hist, const float* const* __restrict__ hpp) {
    update_body<false, false, true>(a, nullptr, nullptr, hist, hpp);
}
__global__ __launch_bounds__(256) void k_update_hist_sched(const UpdateArgs a, const float* const* __restrict__ gpp, float* __restrict__ hist,
                                                           const float* const* __restrict__ hpp) {
    update_body<false, true, true>(a, nullptr, gpp, hist, hpp);
}

}  // namespace dsg
