// Binding modes of n poses: greedy leader clustering on a distance matrix, best pose first (tests/pose_clusters_ref.py is the written
// definition; the header gives the contract).  Three launches on one stream, no atomics, no allocation:
//
//   assign   ONE block of 1024 threads keeps labels[n] in LDS (32 KiB at n = 8192) and walks `order`, PC_BLOCK entries at a time from a
//            double-buffered LDS copy.  A step that finds its pose labelled or invalid is two dependent uniform LDS reads (the order
//            entry o[t], then lab[i]); every thread takes the same decisions, so there is no divergence and no barrier.  At a leader all threads sweep the leader's contiguous row D[i, :]
//            with coalesced loads (thread t owns the columns j = t mod 1024, in every sweep: lab[j] has ONE writer), label what joins,
//            write dist_to_leader and reduce size (integer) and radius (maximum) over the wave; the wave partials go to one of two LDS
//            rows by the parity of k, and after the leader's ONE barrier thread 0 folds them.  The leader's own label is stored after
//            that barrier - a thread still walking towards the leader must find it unlabelled - and the walk knows the last leader
//            from a register, so not even a repeated entry of `order` reads a label while it is written.  Only K rows of D are read.
//   sums     one thread per pose i: s_i = sum over the other members j of its cluster, ascending, of (double)D[j, i] - the column, so
//            that the 64 lanes of a wave read 256 contiguous bytes per j (D is symmetric by contract); labels[j] is uniform.
//   select   one wave per cluster walks the labels 64 at a time; a ballot names the members of a piece, lane order is pose order, and
//            every lane keeps the same running fp64 sums (s_i and the scores reach it through a shuffle from the owning lane) - the
//            stated order.  The medoid is the exact minimum of (s_i, i) by a key that orders doubles as integers.
#include "common.h"
#include "physdock_hip.h"

namespace {

constexpr int PC_BLOCK = 1024;
constexpr int PC_WAVES = PC_BLOCK / 64;
constexpr int PC_FREE = -1, PC_INVALID = -2;      // labels in LDS while the walk runs; both leave as -1


__global__ __launch_bounds__(PC_BLOCK) void pc_assign_kernel(const float* __restrict__ D, const int* __restrict__ order, float cutoff,
                                                            const unsigned char* __restrict__ valid, int* __restrict__ labels,
                                                            float* __restrict__ dist, int* __restrict__ leader, int* __restrict__ size,
                                                            float* __restrict__ radius, int* __restrict__ n_clusters, int n) {
    extern __shared__ int lab[];                   // [n]
    __shared__ int ord[2][PC_BLOCK];
    __shared__ int red_n[2][PC_WAVES];
    __shared__ float red_r[2][PC_WAVES];
    const int tid = threadIdx.x;
    const float nan = __uint_as_float(0x7fc00000u);
    for (int j = tid; j < n; j += PC_BLOCK) {
        lab[j] = (valid && !valid[j]) ? PC_INVALID : PC_FREE;
        dist[j] = nan;
    }
    int k = 0, last = -1;
    for (int base = 0, c = 0; base < n; base += PC_BLOCK, ++c) {
        int* const o = ord[c & 1];
        o[tid] = base + tid < n ? order[base + tid] : -1;
        __syncthreads();                           // also orders the initialisation of lab before the first walk
        const int m = min(PC_BLOCK, n - base);
        for (int t = 0; t < m; ++t) {
            const int i = o[t];
            if ((unsigned)i >= (unsigned)n || i == last || lab[i] != PC_FREE) continue;
            const float* __restrict__ row = D + (size_t)i * n;
            int cnt = 0;
            float rmax = -INFINITY;
            for (int j = tid; j < n; j += PC_BLOCK) {
                if (j != i && lab[j] != PC_FREE) continue;
                const float d = row[j];
                if (j == i || d <= cutoff) {       // fp32, inclusive, false for a NaN; the leader joins whatever its diagonal holds
                    if (j != i) lab[j] = k;
                    dist[j] = d;
                    ++cnt;
                    rmax = fmaxf(rmax, d);
                }
            }
            cnt = wave_sum(cnt);
            rmax = wave_max(rmax);
            if ((tid & 63) == 0) {
                red_n[k & 1][tid >> 6] = cnt;
                red_r[k & 1][tid >> 6] = rmax;
            }
            __syncthreads();
            if (tid == (i & (PC_BLOCK - 1))) lab[i] = k;
            if (tid == 0) {
                int tot = 0;
                float r = -INFINITY;
#pragma unroll
                for (int w = 0; w < PC_WAVES; ++w) {
                    tot += red_n[k & 1][w];
                    r = fmaxf(r, red_r[k & 1][w]);
                }
                leader[k] = i;
                size[k] = tot;
                radius[k] = r;
            }
            last = i;
            ++k;
        }
    }
    __syncthreads();                               // the last leader's own label
    for (int j = tid; j < n; j += PC_BLOCK) {
        labels[j] = max(lab[j], -1);
        if (j >= k) {
            leader[j] = -1;
            size[j] = 0;
            radius[j] = nan;
        }
    }
    if (tid == 0) n_clusters[0] = k;
}

__global__ __launch_bounds__(64) void pc_sums_kernel(const float* __restrict__ D, const int* __restrict__ labels, double* __restrict__ s, int n) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const int mine = labels[i];
    double acc = 0.0;
    if (mine >= 0) {
#pragma unroll 8
        for (int j = 0; j < n; ++j) {
            const float d = D[(size_t)j * n + i];
            if (labels[j] == mine && j != i) acc += (double)d;
        }
    }
    s[i] = acc;
}

// doubles ordered as unsigned integers: negative values have all bits flipped, the others the sign bit set; a NaN counts as +inf
__device__ __forceinline__ pd_u64 pc_order_key(double v) {
    if (v != v) v = INFINITY;
    const pd_u64 b = (pd_u64)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__global__ __launch_bounds__(64) void pc_select_kernel(const int* __restrict__ labels, const double* __restrict__ s,
                                                      const float* __restrict__ score, const int* __restrict__ size,
                                                      const int* __restrict__ n_clusters, int* __restrict__ medoid,
                                                      float* __restrict__ spread, float* __restrict__ mean_score, int n) {
    const int k = blockIdx.x, lane = threadIdx.x;
    const float nan = __uint_as_float(0x7fc00000u);
    if (k >= n_clusters[0]) {
        if (lane == 0) {
            medoid[k] = -1;
            spread[k] = nan;
            mean_score[k] = nan;
        }
        return;
    }
    pd_u64 best_key = ~0ull;
    int best_i = 0x7fffffff;
    double total = 0.0, sc = 0.0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const bool member = i < n && labels[i] == k;
        unsigned long long m = __ballot(member);
        if (m == 0) continue;
        const double si = member ? s[i] : 0.0;
        const double ci = (member && score) ? (double)score[i] : 0.0;
        if (member) {
            const pd_u64 key = pc_order_key(si);
            if (key < best_key) {                  // a lane meets its poses in ascending order: the first of equal keys stays
                best_key = key;
                best_i = i;
            }
        }
        while (m) {
            const int b = __builtin_ctzll(m);
            m &= m - 1;
            total += __shfl(si, b);
            sc += __shfl(ci, b);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const pd_u64 ok = ((pd_u64)__shfl_xor((unsigned)(best_key >> 32), o) << 32) | __shfl_xor((unsigned)best_key, o);
        const int oi = __shfl_xor(best_i, o);
        if (ok < best_key || (ok == best_key && oi < best_i)) {
            best_key = ok;
            best_i = oi;
        }
    }
    if (lane == 0) {
        const int sz = size[k];
        medoid[k] = best_i;
        spread[k] = sz > 1 ? (float)(total / (double)(sz * (sz - 1))) : 0.f;
        mean_score[k] = score ? (float)(sc / (double)sz) : nan;
    }
}

}  // namespace

PD_EXPORT int pd_pose_clusters_workspace_numel(int n) {
    if (n < 1) return PD_ERR_ARG;
    if (n > PD_POSE_CLUSTERS_MAX_POSES) return PD_ERR_UNSUPPORTED;
    return n;
}

PD_EXPORT int pd_pose_clusters(const float* D, const int* order, float cutoff, const unsigned char* valid, const float* score, double* ws,
                               long long ws_numel, int* labels, float* dist_to_leader, int* leader, int* size, float* radius, int* medoid,
                               float* spread, float* mean_score, int* n_clusters, int n, void* stream) {
    if (n < 1) return PD_ERR_ARG;
    if (!D || !order || !ws || !labels || !dist_to_leader || !leader || !size || !radius || !medoid || !spread || !mean_score || !n_clusters)
        return PD_ERR_ARG;
    if ((((uintptr_t)D | (uintptr_t)order | (uintptr_t)score | (uintptr_t)labels | (uintptr_t)dist_to_leader | (uintptr_t)leader |
          (uintptr_t)size | (uintptr_t)radius | (uintptr_t)medoid | (uintptr_t)spread | (uintptr_t)mean_score | (uintptr_t)n_clusters) & 3) != 0 ||
        ((uintptr_t)ws & 7) != 0)
        return PD_ERR_ARG;
    if (!(cutoff >= 0.f) || !(cutoff <= 3.4028234e38f)) return PD_ERR_ARG;                      // negative, NaN or infinite
    if (n > PD_POSE_CLUSTERS_MAX_POSES) return PD_ERR_UNSUPPORTED;
    if (ws_numel < (long long)n) return PD_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pc_assign_kernel, dim3(1), dim3(PC_BLOCK), (size_t)n * sizeof(int), st, D, order, cutoff, valid, labels,
                       dist_to_leader, leader, size, radius, n_clusters, n);
    hipLaunchKernelGGL(pc_sums_kernel, dim3((n + 63) / 64), dim3(64), 0, st, D, (const int*)labels, ws, n);
    hipLaunchKernelGGL(pc_select_kernel, dim3(n), dim3(64), 0, st, (const int*)labels, (const double*)ws, score, (const int*)size,
                       (const int*)n_clusters, medoid, spread, mean_score, n);
    return pd_check_launch();
}
