// Helpers shared by the forward and the backward of the loss (loss.hip, loss_grad.hip).
#pragma once
#include "common.h"

// mean_b (t_b^2 + sd^2) / (t_b sd)^2 in float64, by a block of 256 threads (sh holds 256 doubles)
__device__ __forceinline__ double mean_edm_scale(const float* __restrict__ t_hat, int B, double sd, double* sh) {
    double v = 0;
    for (int b = threadIdx.x; b < B; b += 256) { const double t = t_hat[b]; v += (t * t + sd * sd) / ((t * sd) * (t * sd)); }
    return block_sum_det<256>(v, sh) / B;
}
