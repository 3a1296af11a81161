// How well does a pose agree with what the trunk itself predicted about distances?  The released model carries a trained distance head
// (linear_distogram: no_bins logits per token pair over the pseudo-beta distance); these kernels score P poses of one system against
// those logits on the interface (ligand token x receptor token) and inside the ligand, without a ground truth, confidence weights or a
// borrowed force field.  (physdock_amd/distogram.py builds the tables once per system; tests/distogram_score_ref.py is the written
// definition.)  Caveat: agreement with the trunk is self-consistency, not accuracy; the contact cutoff, the cap on the expected distance
// and the choice of classes are this package's own defaults and have NOT BEEN VALIDATED on real complexes.
//
// One system: logits l [T][T][K] fp32, token_class [T] (0 inactive, 1 receptor, 2 ligand), pb_atom [T] (the pseudo-beta atom of an
// active token), rows [n_rows] = the n_ligand_rows ligand tokens in ascending order and then, with the receptor class, the receptor
// tokens in ascending order.  Edges e_k, k < K - 1, and centres c_b, b < K, come from the host in float64 (bounds_sq[k] = e_k e_k).
//   tables    lse = m + log(sum_b exp(l_b - m)), m = max_b l_b, ascending b in float64; u_b = lse - l_b;
//             expected = sum_b exp(-u_b) c_b, p_contact = sum_{b <= contact_bin} exp(-u_b), each rounded once to fp32
//   pair      d2 = (dx dx + dy dy) + dz dz in float64 from the fp32 coordinates, no fused multiply-add; bin = #{k : d2 > e_k e_k};
//             nll = lse - l[bin]; d = sqrt(d2)
//   classes   interface (i ligand, j receptor, read at l[i][j]), ligand (i < j both ligand), receptor (i < j both receptor)
//   potential V(d) = the linear interpolation of u_b over the centres, constant below c_0 and from c_{K-1} on; at a centre the slope
//             is the right-hand segment's; a pair at d = 0 has no gradient
//
// dg_tables_kernel          256 pairs per block, their logits staged through LDS with an odd row stride (a lane then reads its own row
//                           without a bank conflict), one lane per pair
// dg_score_kernel           one block of four waves per (tile of four rows, pose), the pose's pseudo-beta coordinates in LDS; a wave
//                           owns a row, its lanes walk the columns; per row eight float64 partials (counts are exact in float64)
// dg_reduce_kernel          one block per pose: ok, the row partials summed by block_sum_det, the per-token means (a receptor token's
//                           column is gathered again from the bins, ligand rows ascending)
// dg_potential_rows_kernel  one block per (ligand token, pose) over all partners
// dg_potential_mean_kernel  one block per pose
// Every sum is float64 in a fixed order (a fixed butterfly over the lanes of a wave, a fixed halving tree over the threads of a block),
// there are no atomics, and a pose reads nothing of another pose: a pose's results are bit-identical whatever the batch.  float64
// throughout: the workload is P x rows x T pairs, small next to the sampler; float64 VALU is far from being the limit here.
#include "common.h"
#include "physdock_hip.h"

namespace {

constexpr int DG_MAX_BINS = PD_DISTOGRAM_MAX_BINS, DG_MAX_T = PD_DISTOGRAM_MAX_TOKENS, DG_MAX_P = 65535;
constexpr int DG_PART = PD_DISTOGRAM_ROW_PARTIALS, DG_POT_PART = PD_DISTOGRAM_POTENTIAL_PARTIALS;
static_assert(DG_MAX_BINS == 64 && DG_MAX_T == 4096 && DG_PART == 8 && DG_POT_PART == 5, "the numbers the header documents");

struct DgEdges { double e2[DG_MAX_BINS - 1]; };      // kernel arguments: read with a uniform index, they stay in scalar registers
struct DgCentres { double c[DG_MAX_BINS]; };

__global__ __launch_bounds__(256) void dg_tables_kernel(const float* __restrict__ logits, DgCentres cen, int cstar,
                                                       double* __restrict__ lse, float* __restrict__ expected,
                                                       float* __restrict__ p_contact, long long npairs, int K) {
#pragma clang fp contract(off)
    extern __shared__ float sl[];
    const int ld = K | 1;
    const long long p0 = (long long)blockIdx.x * 256;
    const int np = (int)min((long long)256, npairs - p0);
    for (int e = threadIdx.x; e < np * K; e += 256) sl[(e / K) * ld + e % K] = logits[p0 * K + e];
    __syncthreads();
    if ((int)threadIdx.x >= np) return;
    const float* l = sl + threadIdx.x * ld;
    double m = (double)l[0];
    for (int k = 1; k < K; ++k) m = fmax(m, (double)l[k]);
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += exp((double)l[k] - m);
    const double z = m + log(s);
    double ex = 0.0, pc = 0.0;
    for (int k = 0; k < K; ++k) {
        const double pr = exp(-(z - (double)l[k]));
        ex += pr * cen.c[k];
        if (k <= cstar) pc += pr;
    }
    lse[p0 + threadIdx.x] = z;
    expected[p0 + threadIdx.x] = (float)ex;
    p_contact[p0 + threadIdx.x] = (float)pc;
}

// the pose's pseudo-beta coordinates, one triple per token (zeros for an inactive token), into LDS
__device__ __forceinline__ void dg_stage_pose(float* sx, const float* __restrict__ xp, const int* __restrict__ pb,
                                              const unsigned char* __restrict__ cls, int T) {
    for (int t = threadIdx.x; t < T; t += blockDim.x) {
        const bool on = cls[t] != 0;
        const long long a = on ? pb[t] : 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) sx[3 * t + c] = on ? xp[3 * a + c] : 0.f;
    }
    __syncthreads();
}

// does the pose hold a non-finite coordinate at an active pseudo-beta atom?  (every thread of the block gets the answer)
__device__ __forceinline__ bool dg_pose_bad(const float* __restrict__ xp, const int* __restrict__ pb,
                                            const unsigned char* __restrict__ cls, int T) {
    int bad = 0;
    for (int t = threadIdx.x; t < T; t += blockDim.x) {
        if (!cls[t]) continue;
        const long long a = pb[t];
        bad |= !(isfinite(xp[3 * a]) && isfinite(xp[3 * a + 1]) && isfinite(xp[3 * a + 2]));
    }
    return __syncthreads_or(bad) != 0;
}

__global__ __launch_bounds__(256) void dg_score_kernel(const float* __restrict__ x, const int* __restrict__ pb,
                                                      const unsigned char* __restrict__ cls, const int* __restrict__ rows,
                                                      const float* __restrict__ logits, const double* __restrict__ lse,
                                                      const float* __restrict__ expected, const float* __restrict__ p_contact,
                                                      DgEdges ed, int cstar, float max_expected, unsigned char* __restrict__ bins,
                                                      double* __restrict__ part, int A, int T, int K, int nL, int NR) {
#pragma clang fp contract(off)
    extern __shared__ float sx[];
    const int p = blockIdx.y;
    dg_stage_pose(sx, x + (long long)p * A * 3, pb, cls, T);
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= NR) return;                                   // (behind the block's only barrier)
    const int i = rows[r];
    const bool ligrow = r < nL;
    const double xi = (double)sx[3 * i], yi = (double)sx[3 * i + 1], zi = (double)sx[3 * i + 2];
    double s_main = 0.0, s_lig = 0.0, s_ee = 0.0, s_pc = 0.0;
    int n_ee = 0, n_pred = 0, n_hit = 0, n_con = 0;
    for (int j = lane; j < T; j += 64) {
        const int cj = cls[j];
        int bin = 255;
        double d2 = 0.0;
        if (cj) {
            const double dx = xi - (double)sx[3 * j], dy = yi - (double)sx[3 * j + 1], dz = zi - (double)sx[3 * j + 2];
            d2 = (dx * dx + dy * dy) + dz * dz;
            bin = 0;
            for (int k = 0; k < K - 1; ++k) bin += d2 > ed.e2[k];
        }
        if (ligrow) bins[((long long)p * nL + r) * T + j] = (unsigned char)bin;
        if (!cj) continue;
        const long long ij = (long long)i * T + j;
        if (ligrow && cj == 1) {
            s_main += lse[ij] - (double)logits[ij * K + bin];
            const double ex = (double)expected[ij];
            if (ex <= (double)max_expected) { s_ee += fabs(sqrt(d2) - ex); ++n_ee; }
            const float pc = p_contact[ij];
            const bool near = bin <= cstar;
            if (pc >= 0.5f) { ++n_pred; n_hit += near; }
            if (near) { ++n_con; s_pc += (double)pc; }
        } else if (ligrow && j > i) {
            s_lig += lse[ij] - (double)logits[ij * K + bin];
        } else if (!ligrow && cj == 1 && j > i) {
            s_main += lse[ij] - (double)logits[ij * K + bin];
        }
    }
    s_main = wave_sum(s_main); s_lig = wave_sum(s_lig); s_ee = wave_sum(s_ee); s_pc = wave_sum(s_pc);
    n_ee = wave_sum(n_ee); n_pred = wave_sum(n_pred); n_hit = wave_sum(n_hit); n_con = wave_sum(n_con);
    if (lane == 0) {
        double* o = part + ((long long)p * NR + r) * DG_PART;
        o[0] = s_main; o[1] = s_lig; o[2] = s_ee; o[3] = s_pc;
        o[4] = (double)n_ee; o[5] = (double)n_pred; o[6] = (double)n_hit; o[7] = (double)n_con;
    }
}

__device__ __forceinline__ float dg_mean(double s, double n) { return n > 0.0 ? (float)(s / n) : __builtin_nanf(""); }

__global__ __launch_bounds__(256) void dg_reduce_kernel(const float* __restrict__ x, const int* __restrict__ pb,
                                                       const unsigned char* __restrict__ cls, const int* __restrict__ rows,
                                                       const int* __restrict__ row_of, const float* __restrict__ logits,
                                                       const double* __restrict__ lse, unsigned char* __restrict__ bins,
                                                       const double* __restrict__ part, float* __restrict__ values,
                                                       float* __restrict__ token_nll, int* __restrict__ n_contacts,
                                                       unsigned char* __restrict__ ok, int P, int A, int T, int K, int nL, int nR, int NR) {
    __shared__ double sh[256];
    const int p = blockIdx.x;
    const bool bad = dg_pose_bad(x + (long long)p * A * 3, pb, cls, T);
    double v[DG_PART] = {0, 0, 0, 0, 0, 0, 0, 0}, s_rec = 0.0;
    for (int r = threadIdx.x; r < NR; r += 256) {
        const double* o = part + ((long long)p * NR + r) * DG_PART;
        if (r < nL) {
#pragma unroll
            for (int q = 0; q < DG_PART; ++q) v[q] += o[q];
        } else {
            s_rec += o[0];
        }
    }
#pragma unroll
    for (int q = 0; q < DG_PART; ++q) v[q] = block_sum_det<256>(v[q], sh);
    s_rec = block_sum_det<256>(s_rec, sh);
    const float nan = __builtin_nanf("");
    if (threadIdx.x == 0) {
        const double n_int = (double)nL * nR, n_lig = (double)nL * (nL - 1) / 2, n_rec = NR > nL ? (double)nR * (nR - 1) / 2 : 0.0;
        float o[PD_DISTOGRAM_VALUES];
        o[0] = dg_mean(v[0], n_int);
        o[1] = dg_mean(v[1], n_lig);
        o[2] = dg_mean(s_rec, n_rec);
        o[3] = dg_mean((v[0] + v[1]) + s_rec, n_int + n_lig + n_rec);
        o[4] = dg_mean(v[2], v[4]);
        o[5] = dg_mean(v[6], v[5]);
        o[6] = dg_mean(v[3], v[7]);
#pragma unroll
        for (int q = 0; q < PD_DISTOGRAM_VALUES; ++q) values[(long long)q * P + p] = bad ? nan : o[q];
        n_contacts[p] = bad ? 0 : (int)v[7];
        ok[p] = bad ? 0 : 1;
    }
    for (int t = threadIdx.x; t < T; t += 256) {
        float out = nan;
        if (!bad && cls[t] == 2) {
            out = dg_mean(part[((long long)p * NR + row_of[t]) * DG_PART], (double)nR);
        } else if (!bad && cls[t] == 1 && nL > 0) {
            double s = 0.0;
            for (int r = 0; r < nL; ++r) {
                const long long ij = (long long)rows[r] * T + t;
                s += lse[ij] - (double)logits[ij * K + bins[((long long)p * nL + r) * T + t]];
            }
            out = (float)(s / (double)nL);
        }
        token_nll[(long long)p * T + t] = out;
    }
    if (bad)
        for (long long e = threadIdx.x; e < (long long)nL * T; e += 256) bins[(long long)p * nL * T + e] = 0;
}

__global__ __launch_bounds__(256) void dg_potential_rows_kernel(const float* __restrict__ x, const int* __restrict__ pb,
                                                               const unsigned char* __restrict__ cls, const int* __restrict__ rows,
                                                               const float* __restrict__ logits, const double* __restrict__ lse,
                                                               DgCentres cen, double* __restrict__ part, int A, int T, int K, int nL) {
#pragma clang fp contract(off)
    extern __shared__ float sx[];
    __shared__ double cs[DG_MAX_BINS], sh[256];
    const int p = blockIdx.y, r = blockIdx.x, i = rows[r];
    if ((int)threadIdx.x < K) cs[threadIdx.x] = cen.c[threadIdx.x];
    dg_stage_pose(sx, x + (long long)p * A * 3, pb, cls, T);
    const double xi = (double)sx[3 * i], yi = (double)sx[3 * i + 1], zi = (double)sx[3 * i + 2];
    double sv = 0.0, gx = 0.0, gy = 0.0, gz = 0.0, ga = 0.0;
    for (int j = threadIdx.x; j < T; j += 256) {
        const int cj = cls[j];
        if (!cj || j == i) continue;
        const double dx = xi - (double)sx[3 * j], dy = yi - (double)sx[3 * j + 1], dz = zi - (double)sx[3 * j + 2];
        const double d = sqrt((dx * dx + dy * dy) + dz * dz);
        const bool counted = cj == 1 || j > i;                       // an interface pair, or the ligand pair's own row
        const long long ij = counted ? (long long)i * T + j : (long long)j * T + i;
        const float* l = logits + ij * K;
        int n = 0;
        for (int k = 0; k < K; ++k) n += cs[k] <= d;
        double val, slope = 0.0;
        if (n == 0) {
            val = lse[ij] - (double)l[0];
        } else if (n == K) {
            val = lse[ij] - (double)l[K - 1];
        } else {
            const int b = n - 1;
            const double du = (double)l[b] - (double)l[b + 1], w = cs[b + 1] - cs[b];
            val = (lse[ij] - (double)l[b]) + du * ((d - cs[b]) / w);
            slope = du / w;
        }
        if (counted) sv += val;
        if (d > 0.0) {
            const double q = slope / d, tx = q * dx, ty = q * dy, tz = q * dz;
            gx += tx; gy += ty; gz += tz;
            ga += (fabs(tx) + fabs(ty)) + fabs(tz);
        }
    }
    sv = block_sum_det<256>(sv, sh);
    gx = block_sum_det<256>(gx, sh); gy = block_sum_det<256>(gy, sh); gz = block_sum_det<256>(gz, sh);
    ga = block_sum_det<256>(ga, sh);
    if (threadIdx.x == 0) {
        double* o = part + ((long long)p * nL + r) * DG_POT_PART;
        o[0] = sv; o[1] = gx; o[2] = gy; o[3] = gz; o[4] = ga;
    }
}

__global__ __launch_bounds__(256) void dg_potential_mean_kernel(const float* __restrict__ x, const int* __restrict__ pb,
                                                               const unsigned char* __restrict__ cls, const double* __restrict__ part,
                                                               float* __restrict__ potential, float* __restrict__ forces,
                                                               float* __restrict__ abs_force, int A, int T, int nL, int nR) {
    __shared__ double sh[256];
    const int p = blockIdx.x;
    const bool bad = dg_pose_bad(x + (long long)p * A * 3, pb, cls, T);
    const double n = (double)nL * nR + (double)nL * (nL - 1) / 2;
    const bool none = bad || !(n > 0.0);
    const float nan = __builtin_nanf("");
    double s = 0.0;
    for (int r = threadIdx.x; r < nL; r += 256) s += part[((long long)p * nL + r) * DG_POT_PART];
    s = block_sum_det<256>(s, sh);
    if (threadIdx.x == 0) potential[p] = none ? nan : (float)(s / n);
    if (!forces) return;
    for (int r = threadIdx.x; r < nL; r += 256) {
        const double* o = part + ((long long)p * nL + r) * DG_POT_PART;
#pragma unroll
        for (int c = 0; c < 3; ++c) forces[((long long)p * nL + r) * 3 + c] = none ? nan : (float)(-(o[1 + c] / n));
        abs_force[(long long)p * nL + r] = none ? nan : (float)(o[4] / n);
    }
}

// the limits every entry point shares: PD_OK, or the code to return
int dg_check_sizes(int T, int K) {
    if (T < 1 || K < 2) return PD_ERR_ARG;
    if (T > DG_MAX_T || K > DG_MAX_BINS) return PD_ERR_UNSUPPORTED;
    return PD_OK;
}
int dg_check_poses(int P, int A) {
    if (P < 1 || A < 1) return PD_ERR_ARG;
    return P > DG_MAX_P ? PD_ERR_UNSUPPORTED : PD_OK;
}
bool dg_finite(const double* v, int n) {
    for (int k = 0; k < n; ++k)
        if (!(v[k] - v[k] == 0.0)) return false;
    return true;
}

}  // namespace

PD_EXPORT int pd_distogram_tables(const float* logits, const double* centres, int contact_bin, double* lse, float* expected,
                                  float* p_contact, int T, int no_bins, void* stream) {
    if (!logits || !centres || !lse || !expected || !p_contact || pd_misaligned(logits, 4) || pd_misaligned(lse, 8) ||
        pd_misaligned(expected, 4) || pd_misaligned(p_contact, 4))
        return PD_ERR_ARG;
    if (const int rc = dg_check_sizes(T, no_bins)) return rc;
    if (contact_bin < -1 || contact_bin > no_bins - 2 || !dg_finite(centres, no_bins)) return PD_ERR_ARG;
    DgCentres cen = {};
    for (int k = 0; k < no_bins; ++k) cen.c[k] = centres[k];
    const size_t lds = (size_t)256 * (no_bins | 1) * sizeof(float);
    if (lds > 65536) {                                     // no_bins = 64: 66560 bytes, over the default limit of a block
        static const bool raised = hipFuncSetAttribute(reinterpret_cast<const void*>(dg_tables_kernel),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, 256 * (DG_MAX_BINS | 1) * 4) == hipSuccess;
        if (!raised) return PD_ERR_LAUNCH;
    }
    const long long npairs = (long long)T * T;
    hipLaunchKernelGGL(dg_tables_kernel, dim3((unsigned)((npairs + 255) / 256)), dim3(256), lds, (hipStream_t)stream, logits, cen,
                       contact_bin, lse, expected, p_contact, npairs, no_bins);
    return pd_check_launch();
}

PD_EXPORT int pd_distogram_score(const float* x, const int* pb_atom, const unsigned char* token_class, const int* rows,
                                 const float* logits, const double* lse, const float* expected, const float* p_contact,
                                 const double* bounds_sq, int contact_bin, float max_expected, unsigned char* bins, double* ws,
                                 long long ws_numel, int P, int A, int T, int no_bins, int n_ligand_rows, int n_rows, void* stream) {
    if (!x || !pb_atom || !token_class || !logits || !lse || !expected || !p_contact || !bounds_sq) return PD_ERR_ARG;
    if (pd_misaligned(x, 4) || pd_misaligned(pb_atom, 4) || pd_misaligned(rows, 4) || pd_misaligned(logits, 4) || pd_misaligned(lse, 8) ||
        pd_misaligned(expected, 4) || pd_misaligned(p_contact, 4) || pd_misaligned(ws, 8))
        return PD_ERR_ARG;
    if (const int rc = dg_check_sizes(T, no_bins)) return rc;
    if (const int rc = dg_check_poses(P, A)) return rc;
    if (n_ligand_rows < 0 || n_rows < n_ligand_rows || n_rows > T || contact_bin < -1 || contact_bin > no_bins - 2 ||
        !(max_expected == max_expected) || !dg_finite(bounds_sq, no_bins - 1))
        return PD_ERR_ARG;
    if (n_rows == 0) return PD_OK;                         // no ligand token and no receptor class: nothing to sum
    if (!rows || !ws || (n_ligand_rows > 0 && !bins) || ws_numel < (long long)P * n_rows * DG_PART) return PD_ERR_ARG;
    DgEdges ed = {};
    for (int k = 0; k < no_bins - 1; ++k) ed.e2[k] = bounds_sq[k];
    hipLaunchKernelGGL(dg_score_kernel, dim3((unsigned)((n_rows + 3) / 4), (unsigned)P), dim3(256), (size_t)T * 3 * sizeof(float),
                       (hipStream_t)stream, x, pb_atom, token_class, rows, logits, lse, expected, p_contact, ed, contact_bin,
                       max_expected, bins, ws, A, T, no_bins, n_ligand_rows, n_rows);
    return pd_check_launch();
}

PD_EXPORT int pd_distogram_reduce(const float* x, const int* pb_atom, const unsigned char* token_class, const int* rows,
                                  const int* row_of, const float* logits, const double* lse, unsigned char* bins, const double* ws,
                                  long long ws_numel, float* values, float* token_nll, int* n_contacts, unsigned char* ok, int P, int A,
                                  int T, int no_bins, int n_ligand_rows, int n_receptor_tokens, int n_rows, void* stream) {
    if (!x || !pb_atom || !token_class || !row_of || !logits || !lse || !values || !token_nll || !n_contacts || !ok) return PD_ERR_ARG;
    if (pd_misaligned(x, 4) || pd_misaligned(pb_atom, 4) || pd_misaligned(rows, 4) || pd_misaligned(row_of, 4) || pd_misaligned(logits, 4) ||
        pd_misaligned(lse, 8) || pd_misaligned(ws, 8) || pd_misaligned(values, 4) || pd_misaligned(token_nll, 4) || pd_misaligned(n_contacts, 4))
        return PD_ERR_ARG;
    if (const int rc = dg_check_sizes(T, no_bins)) return rc;
    if (const int rc = dg_check_poses(P, A)) return rc;
    if (n_ligand_rows < 0 || n_receptor_tokens < 0 || n_ligand_rows + n_receptor_tokens > T ||
        (n_rows != n_ligand_rows && n_rows != n_ligand_rows + n_receptor_tokens))
        return PD_ERR_ARG;
    if (n_rows > 0 && (!rows || !ws || (n_ligand_rows > 0 && !bins) || ws_numel < (long long)P * n_rows * DG_PART)) return PD_ERR_ARG;
    hipLaunchKernelGGL(dg_reduce_kernel, dim3((unsigned)P), dim3(256), 0, (hipStream_t)stream, x, pb_atom, token_class, rows, row_of,
                       logits, lse, bins, ws, values, token_nll, n_contacts, ok, P, A, T, no_bins, n_ligand_rows, n_receptor_tokens,
                       n_rows);
    return pd_check_launch();
}

PD_EXPORT int pd_distogram_potential(const float* x, const int* pb_atom, const unsigned char* token_class, const int* rows,
                                     const float* logits, const double* lse, const double* centres, double* ws, long long ws_numel,
                                     float* potential, float* forces, float* abs_force, int P, int A, int T, int no_bins,
                                     int n_ligand_rows, int n_receptor_tokens, void* stream) {
    if (!x || !pb_atom || !token_class || !logits || !lse || !centres || !potential || (forces == nullptr) != (abs_force == nullptr))
        return PD_ERR_ARG;
    if (pd_misaligned(x, 4) || pd_misaligned(pb_atom, 4) || pd_misaligned(rows, 4) || pd_misaligned(logits, 4) || pd_misaligned(lse, 8) ||
        pd_misaligned(ws, 8) || pd_misaligned(potential, 4) || pd_misaligned(forces, 4) || pd_misaligned(abs_force, 4))
        return PD_ERR_ARG;
    if (const int rc = dg_check_sizes(T, no_bins)) return rc;
    if (const int rc = dg_check_poses(P, A)) return rc;
    if (n_ligand_rows < 0 || n_receptor_tokens < 0 || n_ligand_rows + n_receptor_tokens > T || !dg_finite(centres, no_bins))
        return PD_ERR_ARG;
    if (n_ligand_rows > 0) {
        if (!rows || !ws || ws_numel < (long long)P * n_ligand_rows * DG_POT_PART) return PD_ERR_ARG;
        DgCentres cen = {};
        for (int k = 0; k < no_bins; ++k) cen.c[k] = centres[k];
        hipLaunchKernelGGL(dg_potential_rows_kernel, dim3((unsigned)n_ligand_rows, (unsigned)P), dim3(256), (size_t)T * 3 * sizeof(float),
                           (hipStream_t)stream, x, pb_atom, token_class, rows, logits, lse, cen, ws, A, T, no_bins, n_ligand_rows);
    }
    hipLaunchKernelGGL(dg_potential_mean_kernel, dim3((unsigned)P), dim3(256), 0, (hipStream_t)stream, x, pb_atom, token_class, ws,
                       potential, forces, abs_force, A, T, n_ligand_rows, n_receptor_tokens);
    return pd_check_launch();
}
