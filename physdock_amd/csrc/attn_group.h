// Grouped attention launches (ABI 10, pd_attn_args.group_samples / bias_gstride / nk_group): several systems in one launch, one
// bias set and one real key count per run of group_samples consecutive batches.  Every attention kernel resolves its block's group
// ONCE, as scalars in 32-bit arithmetic, right after it knows its batch index, and from then on sees a plain single-group launch:
// the bias pointer moved to the group's fragment set (the 32-bit buffer offsets of the kernels stay relative to it) and nk = the
// group's key count, clamped to [1, launch nk] so that no group ever reads key rows past the launch's bound.
#pragma once
#include "physdock_hip.h"

__device__ __forceinline__ pd_attn_args pd_attn_group(pd_attn_args p, int b) {
    if (p.group_samples > 0 || p.nk_group) {
        const int g = p.group_samples > 0 ? b / p.group_samples : 0;
        if (p.bias) p.bias += (long long)g * p.bias_gstride;
        if (p.nk_group) {
            const int n = __builtin_amdgcn_readfirstlane(p.nk_group[g]);
            p.nk = n < 1 ? 1 : (n < p.nk ? n : p.nk);
        }
    }
    return p;
}
