// The inference-time confidence metrics (PhysDock/data/tools/get_metrics.py): per-atom pLDDT and its mean, the expected aligned
// error, pTM / ipTM with the row they were taken from, the chain-pair clash flag and ranking_confidence, for P stacked logit sets
// and B poses at once.  fp32 throughout (the 64-entry TM table is formed once per call in float64 and rounded).  The logits are
// read exactly once: a pair's bins sit in the 16 lanes of one DPP row, four bins per lane from one 16-byte load, so a wave takes
// four pairs per load instruction and all in-row reductions are VALU-only (quad_perm x2, row_half_mirror, row_mirror).
// Every floating-point reduction is ordered: a row's pairs are summed 16 at a time in a fixed tree, whichever block and wave
// takes them, the partial sums are combined in ascending j by a second kernel, and there is no floating-point atomic.  Clash
// counts are integers (vector atomics; integer addition is order-independent).  No launcher allocates, reads back or synchronises.
#include "common.h"
#include "physdock_hip.h"

namespace {

constexpr int WS_HEAD = 64;      // floats of the PAE workspace in front of the partial sums [P][T][ceil(T / 16)][2]: the TM table
constexpr int PPI = 64;          // pairs per block iteration: 4 waves x 4 loads x 4 lane rows
constexpr int MAX_CHAIN = 64;
constexpr int CA = 256;          // atoms per block of the clash kernel (one lane per atom)

__device__ __forceinline__ float row16_sum(float v) {      // sum over the 16 lanes of a DPP row, the same bits in every lane
    v += pd_dpp<0xB1>(v);
    v += pd_dpp<0x4E>(v);
    v += pd_dpp<0x141>(v);
    v += pd_dpp<0x140>(v);
    return v;
}
__device__ __forceinline__ float row16_max(float v) {
    v = fmaxf(v, pd_dpp<0xB1>(v));
    v = fmaxf(v, pd_dpp<0x4E>(v));
    v = fmaxf(v, pd_dpp<0x141>(v));
    v = fmaxf(v, pd_dpp<0x140>(v));
    return v;
}

// bins 4 sub .. 4 sub + 3 of one row of logits; bins >= nb are -inf (weight 0), a row outside the range is all zeros (finite, unused)
template <bool VEC>
__device__ __forceinline__ void load_bins(const float* __restrict__ row, int sub, int nb, bool valid, float v[4]) {
    if (VEC) {
        f32x4 q = {0.f, 0.f, 0.f, 0.f};
        const bool on = 4 * sub < nb;                                       // nb % 4 == 0 here
        if (valid && on) q = *reinterpret_cast<const f32x4*>(row + 4 * sub);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (on || !valid) ? q[e] : -INFINITY;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int k = 4 * sub + e;
            v[e] = !valid ? 0.f : (k < nb ? row[k] : -INFINITY);
        }
    }
}

// softmax of one row held by a DPP row of lanes, and two expectations from it: sum_k p_k c_k, sum_k p_k t_k
__device__ __forceinline__ void expect2(const float v[4], const float c[4], const float t[4], float& ec, float& et) {
    const float mx = row16_max(fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
    float s = 0.f, sc = 0.f, st = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float ez = expf(v[e] - mx);
        s += ez;
        sc += ez * c[e];
        st += ez * t[e];
    }
    const float inv = 1.0f / row16_sum(s);
    ec = row16_sum(sc) * inv;
    et = row16_sum(st) * inv;
}

// ------------------------------------------------------------------ pLDDT (compute_plddt)
// rows = P * A atoms, 16 rows per wave iteration; atom_plddts = 100 sum_k softmax(l)_k (k + 0.5) / nb
template <bool VEC>
__global__ __launch_bounds__(256) void plddt_kernel(const float* __restrict__ logits, float* __restrict__ out, long long R, int nb) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane >> 4, sub = lane & 15;
    float c[4], z[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) c[e] = 4 * sub + e < nb ? ((float)(4 * sub + e) + 0.5f) / (float)nb : 0.f;
    const long long r0 = ((long long)blockIdx.x * 4 + wv) * 16;
    float res[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const long long r = r0 + 4 * u + g;
        float v[4], et;
        load_bins<VEC>(logits + r * nb, sub, nb, r < R, v);
        expect2(v, c, z, res[u], et);
    }
    const float mine = sub == 0 ? res[0] : sub == 1 ? res[1] : sub == 2 ? res[2] : res[3];
    const long long r = r0 + 4 * sub + g;
    if (sub < 4 && r < R) out[r] = mine * 100.f;
}

// mean_plddt[p]: the plain mean over all A atoms, summed in float64 in a fixed order
__global__ __launch_bounds__(256) void plddt_mean_kernel(const float* __restrict__ atom, float* __restrict__ mean, int A) {
    __shared__ double sh[256];
    const float* a = atom + (long long)blockIdx.x * A;
    double s = 0;
    for (int e = threadIdx.x; e < A; e += 256) s += a[e];
    s = block_sum_det<256>(s, sh);
    if (threadIdx.x == 0) mean[blockIdx.x] = (float)(s / A);
}

// ------------------------------------------------------------------ PAE, pTM, ipTM (compute_predicted_aligned_error, predicted_tm_score)
// tm[k] = 1 / (1 + centre_k^2 / d0^2), d0 = 1.24 (max(int(sum w), 19) - 15)^(1/3) - 1.8: 64 values, once per call, in float64
__global__ __launch_bounds__(256) void tm_table_kernel(const float* __restrict__ w, const float* __restrict__ centres, float* __restrict__ tab,
                                                      int T, int nb) {
    __shared__ double sh[256];
    double s = 0;
    for (int t = threadIdx.x; t < T; t += 256) s += w[t];
    s = block_sum_det<256>(s, sh);
    const int n = s >= 2147483647.0 ? 2147483647 : (int)s;                    // int(): truncation
    const double d0 = 1.24 * cbrt((double)(max(n, 19) - 15)) - 1.8;
    if ((int)threadIdx.x < WS_HEAD) {
        const double c = (int)threadIdx.x < nb ? (double)centres[threadIdx.x] : 0.0;
        tab[threadIdx.x] = (int)threadIdx.x < nb ? (float)(1.0 / (1.0 + (c * c) / (d0 * d0))) : 0.f;
    }
}

// block = (row i, j-split s, logit set p): the pairs (i, j), j in [s chunk, (s + 1) chunk), 64 per iteration.  Wave wv takes 16
// consecutive pairs of every 64, its load u the four pairs 4 u .. 4 u + 3, one per lane row g.  Per pair one softmax gives
// pae = sum_k p_k centre_k (written) and tm = sum_k p_k tm_k.  The 16 terms tm w_j of a wave iteration (once for all pairs, once
// for asym_j != asym_i) are added in a fixed tree and written as part[p][i][j / 16]: the partial sums do not depend on how the
// j range was split over blocks, so any P gives the same bits.
__device__ __forceinline__ float rows4_sum(float v) {                        // (row 0 + row 1) + (row 2 + row 3), wave-uniform
    const float a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float b = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float c = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return (a + b) + (c + d);
}

template <bool VEC>
__global__ __launch_bounds__(256) void pae_tm_kernel(const float* __restrict__ logits, const float* __restrict__ centres,
                                                    const float* __restrict__ tab, const float* __restrict__ w,
                                                    const int* __restrict__ asym, float* __restrict__ part, float* __restrict__ pae,
                                                    int T, int nb, int nsplit, int chunk) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane >> 4, sub = lane & 15;
    const int i = blockIdx.x / nsplit, s = blockIdx.x % nsplit, p = blockIdx.y;
    const int j0 = s * chunk, j1 = min(T, j0 + chunk), units = (T + 15) / 16;
    float c[4], t[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int k = 4 * sub + e;
        c[e] = k < nb ? centres[k] : 0.f;
        t[e] = k < nb ? tab[k] : 0.f;
    }
    const int ai = asym ? asym[i] : 0;
    const long long rowi = (long long)p * T + i;
    const float* base = logits + rowi * T * nb;
    for (int jb = j0 + wv * 16; jb < j1; jb += PPI) {                         // wave-uniform; j0 and chunk are multiples of 64
        float v[4][4], res[4], term[4], termi[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = jb + 4 * u + g;
            load_bins<VEC>(base + (long long)j * nb, sub, nb, j < j1, v[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = jb + 4 * u + g;
            const bool in = j < j1;
            float tm;
            expect2(v[u], c, t, res[u], tm);
            const float wj = in ? w[j] : 0.f;
            const bool other = in && asym && asym[j] != ai;
            term[u] = in ? tm * wj : 0.f;
            termi[u] = other ? term[u] : 0.f;
        }
        const float mine = sub == 0 ? res[0] : sub == 1 ? res[1] : sub == 2 ? res[2] : res[3];
        const int j = jb + 4 * sub + g;
        if (pae && sub < 4 && j < j1) pae[rowi * T + j] = mine;
        const float all = rows4_sum((term[0] + term[1]) + (term[2] + term[3]));
        const float inter = rows4_sum((termi[0] + termi[1]) + (termi[2] + termi[3]));
        if (lane == 0) {
            float* o = part + (rowi * units + (jb >> 4)) * 2;
            o[0] = all;
            o[1] = inter;
        }
    }
}

// block = logit set p, one lane per row i: the partials of the row in ascending j, the weight sums over j in ascending j,
//   per_alignment_i = w_i sum_j tm_ij m_ij w_j / (1e-8 + w_i sum_j m_ij w_j)      for m = 1 (pTM) and m = asym_i != asym_j (ipTM)
// and the value at the FIRST maximal row of per_alignment_i w_i (numpy argmax).
__global__ __launch_bounds__(256) void tm_final_kernel(const float* __restrict__ part, const float* __restrict__ w,
                                                      const int* __restrict__ asym, float* __restrict__ ptm, float* __restrict__ iptm,
                                                      int* __restrict__ rows, float* __restrict__ per_alignment, int T) {
    __shared__ float bv[2][256], bp[2][256];
    __shared__ int bi[2][256];
    const int p = blockIdx.x;
    float best[2] = {-INFINITY, -INFINITY}, bestpa[2] = {0.f, 0.f};
    int besti[2] = {0x7fffffff, 0x7fffffff};
    for (int i = threadIdx.x; i < T; i += 256) {
        const int units = (T + 15) / 16;
        const float* pr = part + ((long long)p * T + i) * units * 2;
        float num[2] = {0.f, 0.f}, den[2] = {0.f, 0.f};
        for (int s = 0; s < units; ++s) { num[0] += pr[2 * s]; num[1] += pr[2 * s + 1]; }
        const int ai = asym ? asym[i] : 0;
        for (int j = 0; j < T; ++j) {
            const float wj = w[j];
            den[0] += wj;
            den[1] += (asym && asym[j] != ai) ? wj : 0.f;
        }
        const float wi = w[i];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const float pa = (wi * num[q]) / (1e-8f + wi * den[q]);
            if (per_alignment) per_alignment[((long long)p * 2 + q) * T + i] = pa;
            const float val = pa * wi;
            if (val > best[q]) { best[q] = val; besti[q] = i; bestpa[q] = pa; }      // strict: the first of equal values stays
        }
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) { bv[q][threadIdx.x] = best[q]; bi[q][threadIdx.x] = besti[q]; bp[q][threadIdx.x] = bestpa[q]; }
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const float ov = bv[q][threadIdx.x + s];
                const int oi = bi[q][threadIdx.x + s];
                if (ov > bv[q][threadIdx.x] || (ov == bv[q][threadIdx.x] && oi < bi[q][threadIdx.x])) {
                    bv[q][threadIdx.x] = ov; bi[q][threadIdx.x] = oi; bp[q][threadIdx.x] = bp[q][threadIdx.x + s];
                }
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        ptm[p] = bp[0][0];
        iptm[p] = bp[1][0];
        rows[2 * p] = bi[0][0] == 0x7fffffff ? 0 : bi[0][0];                  // every value NaN: row 0
        rows[2 * p + 1] = bi[1][0] == 0x7fffffff ? 0 : bi[1][0];
    }
}

// number of j-splits of a row and their length (a multiple of 64 pairs): about 2048 blocks where P T alone gives fewer
inline int tm_split(int P, int T, int* chunk) {
    const long long rows = (long long)P * T;
    long long want = rows >= 2048 ? 1 : (2048 + rows - 1) / rows;
    const int most = (T + PPI - 1) / PPI;
    if (want > most) want = most;
    const int per = (int)((T + want - 1) / want);
    const int ch = (per + PPI - 1) / PPI * PPI;
    *chunk = ch;
    return (T + ch - 1) / ch;
}

// ------------------------------------------------------------------ clash (get_has_clash) and ranking_confidence
__global__ __launch_bounds__(256) void zero_int_kernel(int* __restrict__ v, long long n) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e < n) v[e] = 0;
}

// block = (tile of CA atoms, pose b), one lane per atom i; all atoms j staged CA at a time.  Eligible: a_mask == 1 and polymer.
// cnt[b][ci][cj] += 1 for every ORDERED eligible pair (i, j) with |x_i - x_j| < 1.1 (i == j included: the reference's
// self-pairs count the zero self-distances), so cnt[b][a][c] is the reference's n_clash of the chain pair (a, c).
__global__ __launch_bounds__(CA) void clash_count_kernel(const float* __restrict__ x, const float* __restrict__ a_mask,
                                                        const int* __restrict__ chain, const float* __restrict__ polymer,
                                                        int* __restrict__ cnt, int A, int nc) {
    __shared__ float sx[CA], sy[CA], sz[CA];
    __shared__ int sc[CA];
    const int i = blockIdx.x * CA + threadIdx.x;
    const float* X = x + (long long)blockIdx.y * A * 3;
    int* C = cnt + (long long)blockIdx.y * nc * nc;
    int ci = -1;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (i < A) {
        px = X[3 * i]; py = X[3 * i + 1]; pz = X[3 * i + 2];
        const int c = chain[i];
        if (a_mask[i] == 1.f && polymer[i] != 0.f && c >= 0 && c < nc) ci = c;
    }
    for (int t0 = 0; t0 < A; t0 += CA) {
        const int n = min(CA, A - t0);
        __syncthreads();
        if ((int)threadIdx.x < n) {
            const int j = t0 + threadIdx.x;
            sx[threadIdx.x] = X[3 * j]; sy[threadIdx.x] = X[3 * j + 1]; sz[threadIdx.x] = X[3 * j + 2];
            const int c = chain[j];
            sc[threadIdx.x] = (a_mask[j] == 1.f && polymer[j] != 0.f && c >= 0 && c < nc) ? c : -1;
        }
        __syncthreads();
        if (ci < 0) continue;
        for (int e = 0; e < n; ++e) {
            const int cj = sc[e];
            const float dx = px - sx[e], dy = py - sy[e], dz = pz - sz[e];
            const float d = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
            if (cj >= 0 && d < 1.1f) atomicAdd(&C[ci * nc + cj], 1);
        }
    }
}

// block = pose b.  N_c = eligible atoms of chain c; the reference loops a over uniq[:-1] and c over uniq[1:], uniq = the chains
// WITH eligible atoms in ascending order, which for three or more chains pairs a middle chain with itself (n_clash >= N: always a
// clash); skip_self restricts the loop to a < c.  Clash: n > 100 or n / min(N_a, N_c) > 0.5.  The second test is done as
// 2 n > min in integers: it is only reached with n <= 100, where the fp32 quotient n / m of the reference compares with 0.5 as the
// exact one does for every m <= 2^24 (2 n > m means n / m - 1/2 >= 1 / (2 m) >= 2^-25, half the spacing of fp32 above 0.5, so the
// rounded quotient stays above 0.5; 2 n <= m rounds to at most 0.5).  Fewer than two such chains: no clash.
// ranking[b] = 0.8 iptm + 0.2 ptm - has_clash, (i)ptm read at b * tm_stride (0: one shared value).
__global__ __launch_bounds__(256) void clash_final_kernel(const int* __restrict__ cnt, const float* __restrict__ a_mask,
                                                        const int* __restrict__ chain, const float* __restrict__ polymer,
                                                        const float* __restrict__ ptm, const float* __restrict__ iptm, int tm_stride,
                                                        long long* __restrict__ has_clash, float* __restrict__ ranking, int A, int nc,
                                                        int skip_self) {
    __shared__ int N[MAX_CHAIN];
    __shared__ int first, last, hit;
    const int b = blockIdx.x;
    if ((int)threadIdx.x < MAX_CHAIN) N[threadIdx.x] = 0;
    if (threadIdx.x == 0) { first = 0x7fffffff; last = -1; hit = 0; }
    __syncthreads();
    for (int a = threadIdx.x; a < A; a += 256) {
        const int c = chain[a];
        if (a_mask[a] == 1.f && polymer[a] != 0.f && c >= 0 && c < nc) atomicAdd(&N[c], 1);
    }
    __syncthreads();
    if ((int)threadIdx.x < nc && N[threadIdx.x] > 0) { atomicMin(&first, (int)threadIdx.x); atomicMax(&last, (int)threadIdx.x); }
    __syncthreads();
    const int* C = cnt + (long long)b * nc * nc;
    for (int e = threadIdx.x; e < nc * nc; e += 256) {
        const int a = e / nc, c = e % nc;
        if (N[a] == 0 || N[c] == 0) continue;
        if (skip_self ? a >= c : (a == last || c == first)) continue;
        const int n = C[e], m = min(N[a], N[c]);
        if (n > 100 || 2 * n > m) atomicOr(&hit, 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        has_clash[b] = hit;
        if (ranking) ranking[b] = (0.8f * iptm[(long long)b * tm_stride] + 0.2f * ptm[(long long)b * tm_stride]) - (float)hit;
    }
}

}  // namespace

PD_EXPORT int pd_metrics_workspace_numel(int P, int T) {
    if (P < 1 || T < 1) return PD_ERR_ARG;
    const long long n = WS_HEAD + (long long)P * T * ((T + 15) / 16) * 2;
    return n > 0x7fffffffLL ? PD_ERR_UNSUPPORTED : (int)n;
}

PD_EXPORT int pd_metrics_plddt(const float* p_plddt, float* atom_plddts, float* mean_plddt, int P, int A, int no_bins, void* stream) {
    if (!p_plddt || !atom_plddts || !mean_plddt || P < 1 || A < 1 || no_bins < 1) return PD_ERR_ARG;
    if (no_bins > 64) return PD_ERR_UNSUPPORTED;                            // 16 lanes x 4 bins per row
    const long long R = (long long)P * A, nblk = (R + 63) / 64;
    if (nblk > 0x7fffffffLL) return PD_ERR_UNSUPPORTED;
    const bool vec = no_bins % 4 == 0 && ((uintptr_t)p_plddt & 15) == 0;
    if (vec) hipLaunchKernelGGL(plddt_kernel<true>, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, p_plddt, atom_plddts, R, no_bins);
    else hipLaunchKernelGGL(plddt_kernel<false>, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, p_plddt, atom_plddts, R, no_bins);
    hipLaunchKernelGGL(plddt_mean_kernel, dim3(P), dim3(256), 0, (hipStream_t)stream, atom_plddts, mean_plddt, A);
    return pd_check_launch();
}

PD_EXPORT int pd_metrics_pae_tm(const float* p_pae, const float* centres, const float* weights, const int* asym_id, float* ws, float* pae,
                                float* ptm, float* iptm, int* rows, float* per_alignment, int P, int T, int no_bins, void* stream) {
    if (!p_pae || !centres || !weights || !ws || !ptm || !iptm || !rows || P < 1 || T < 1 || no_bins < 1) return PD_ERR_ARG;
    if (no_bins > 64 || P > 65535) return PD_ERR_UNSUPPORTED;
    int chunk;
    const int nsplit = tm_split(P, T, &chunk);
    if ((long long)T * nsplit > 0x7fffffffLL || WS_HEAD + (long long)P * T * ((T + 15) / 16) * 2 > 0x7fffffffLL) return PD_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    float* part = ws + WS_HEAD;
    hipLaunchKernelGGL(tm_table_kernel, dim3(1), dim3(256), 0, st, weights, centres, ws, T, no_bins);
    const bool vec = no_bins % 4 == 0 && ((uintptr_t)p_pae & 15) == 0;
    const dim3 grid((unsigned)(T * nsplit), (unsigned)P);
    if (vec) hipLaunchKernelGGL(pae_tm_kernel<true>, grid, dim3(256), 0, st, p_pae, centres, ws, weights, asym_id, part, pae, T, no_bins, nsplit, chunk);
    else hipLaunchKernelGGL(pae_tm_kernel<false>, grid, dim3(256), 0, st, p_pae, centres, ws, weights, asym_id, part, pae, T, no_bins, nsplit, chunk);
    hipLaunchKernelGGL(tm_final_kernel, dim3(P), dim3(256), 0, st, part, weights, asym_id, ptm, iptm, rows, per_alignment, T);
    return pd_check_launch();
}

PD_EXPORT int pd_metrics_clash(const float* x_pred, const float* a_mask, const int* chain, const float* polymer, int* counts,
                               const float* ptm, const float* iptm, int tm_stride, long long* has_clash, float* ranking, int B, int A,
                               int n_chain, int skip_self_pairs, void* stream) {
    if (!x_pred || !a_mask || !chain || !polymer || !counts || !has_clash || B < 1 || A < 1 || n_chain < 1 ||
        (ranking && (!ptm || !iptm)) || tm_stride < 0 || tm_stride > 1)
        return PD_ERR_ARG;
    if (n_chain > MAX_CHAIN || B > 65535 || A > 46340) return PD_ERR_UNSUPPORTED;   // counts up to A^2 stay below 2^31
    hipStream_t st = (hipStream_t)stream;
    const long long n = (long long)B * n_chain * n_chain;
    hipLaunchKernelGGL(zero_int_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, counts, n);
    hipLaunchKernelGGL(clash_count_kernel, dim3((A + CA - 1) / CA, B), dim3(CA), 0, st, x_pred, a_mask, chain, polymer, counts, A, n_chain);
    hipLaunchKernelGGL(clash_final_kernel, dim3(B), dim3(256), 0, st, counts, a_mask, chain, polymer, ptm, iptm, tm_stride, has_clash,
                       ranking, A, n_chain, skip_self_pairs);
    return pd_check_launch();
}
