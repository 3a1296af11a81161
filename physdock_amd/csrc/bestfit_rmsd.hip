// Best-fit (superposed) symmetry-corrected ligand RMSD: the ligand-only RMSD minimised over rigid superpositions and over a table
// of graph automorphisms of the ligand (physdock_amd/symmetry.py) - what RDKit calls GetBestRMS.  pd_pairwise_rmsd and pd_sym_rmsd
// compare ligands in a fixed frame (how far is the ligand from where it should be); this one asks whether the CONFORMATION is right.
// tests/bestfit_rmsd_ref.py is the written definition.
//
//   a, b [L,3]: the two ligands, each centred on its unweighted centroid in float64; G = sum of squared norms
//   msd(a, b, m) = min over proper rotations R of (1/L) sum_k |R a[k] - b[perm[m][k]]|^2
//                = (G_a + G_b - 2 lambda_max(N(a, b o perm_m))) / L                              (Horn 1987)
//   D = (float) sqrt(max(0, min_m msd)), the smallest m wins a tie; quat = the unit eigenvector (w, x, y, z) of lambda_max of the
//   winning m, first non-zero component positive: R(quat) a ~ b o perm_m.  Proper rotations only: a mirror image does not match.
//
// Two launches.  bestfit_prepare_kernel, one block per structure: the centred float64 ligand coordinates, G and a finite flag go
// to the workspace, so that none of them depends on the tile that later reads them.  bestfit_rmsd_kernel, one block of 256 threads
// per (row i, tile of TJ columns): the row's and the tile's centred coordinates sit in LDS as float64 (24 B per atom per structure,
// structures (3 L | 1) doubles apart: an odd stride, so that lanes that read the same atom of different columns hit different
// banks); the 256 threads are TJ groups of G = 256 / TJ lanes, group t owns column j0 + t and its lanes stride over the table rows
// m.  One thread owns one (i, j, m): the nine covariance sums over k ascending with explicit fma, Horn's 4x4 matrix, lambda_max
// by cyclic Jacobi in float64 (fixed sweep order, stops when the off-diagonal part is exactly zero).  NOT the Newton iteration on
// the characteristic polynomial (QCP): it loses digits exactly where two conformers coincide, the case pruning depends on.  The
// minimum over m is exact - the key (bits of the non-negative msd, m) is ordered as the pair is - and is a shuffle reduction over
// the G lanes (one LDS step over the four waves when G = 256).  No atomics.  The eigenvector is computed for the winning m only,
// and only when quat is asked for.  TJ is 64, 16, 4 or 1: the largest with G >= M (so that M = 1 .. 4 run 64 columns per block)
// whose tile fits 64 KiB of LDS.  A value depends on its own two structures and the table only, never on na, nb, TJ or the launch.
#include "common.h"
#include "geom3.h"
#include "physdock_hip.h"

namespace {

constexpr int BF_MAX_L = 1024;          // ligand atoms, as pd_sym_rmsd: two structures of 24 B per atom stay below 64 KiB
constexpr int BF_MAX_M = 65535;         // table rows: an unsigned short entry addresses an atom
constexpr int BF_MAX_N = 65535;         // rows / columns: blockIdx.y
constexpr int BF_LDS_BYTES = 65536 - 256;

typedef pd_u64 u64;

__host__ __device__ inline int bf_lds_stride(int L) { return (3 * L) | 1; }
__host__ __device__ inline long long bf_ws_stride(int L) { return 3LL * L + 2; }       // centred [L][3] | G | finite flag

inline int bf_tile(int L, int M) {
    int tj = M <= 4 ? 64 : (M <= 16 ? 16 : (M <= 64 ? 4 : 1));
    while (tj > 1 && (long long)(tj + 1) * bf_lds_stride(L) * 8 > BF_LDS_BYTES) tj /= 4;
    return tj;
}

// the nine covariance sums of row a against column b seen through table row m, k ascending
__device__ __forceinline__ void bf_covariance(const double* a, const double* b, const unsigned short* __restrict__ perms_t, int L,
                                              int M, int m, double (&S)[9]) {
#pragma unroll
    for (int e = 0; e < 9; ++e) S[e] = 0.0;
    const unsigned short* pm = perms_t ? perms_t + m : nullptr;
#pragma unroll 2
    for (int k = 0; k < L; ++k) {
        const int p = pm ? (int)pm[(long long)k * M] : k;
        const double ax = a[3 * k], ay = a[3 * k + 1], az = a[3 * k + 2];
        const double bx = b[3 * p], by = b[3 * p + 1], bz = b[3 * p + 2];
        S[0] = fma(ax, bx, S[0]); S[1] = fma(ax, by, S[1]); S[2] = fma(ax, bz, S[2]);
        S[3] = fma(ay, bx, S[3]); S[4] = fma(ay, by, S[4]); S[5] = fma(ay, bz, S[5]);
        S[6] = fma(az, bx, S[6]); S[7] = fma(az, by, S[7]); S[8] = fma(az, bz, S[8]);
    }
}

// per structure: centred float64 coordinates, G and the finite flag.  Sums: every thread adds its atoms k = tid, tid + 256, .. in
// order, then a fixed tree over the 256 partial sums - a function of the structure alone.  An index outside the structure is never
// followed: it marks the structure as not finite (the host layer refuses such an index before any call).
__global__ __launch_bounds__(256) void bestfit_prepare_kernel(const float* __restrict__ xa, const int* __restrict__ idx_a, int na, int Aa,
                                                             const float* __restrict__ xb, const int* __restrict__ idx_b, int Ab, int L,
                                                             double* __restrict__ ws) {
    __shared__ double red[3][256];
    const int s = blockIdx.x, tid = threadIdx.x;
    const bool col = s >= na;
    const int A = col ? Ab : Aa;
    const float* src = col ? xb + (long long)(s - na) * Ab * 3 : xa + (long long)s * Aa * 3;
    const int* idx = col ? idx_b : idx_a;
    double* out = ws + (long long)s * bf_ws_stride(L);
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int bad = 0;
    for (int k = tid; k < L; k += 256) {
        const int a = idx ? idx[k] : k;
        if ((unsigned)a >= (unsigned)A) { bad = 1; continue; }
        const float x = src[3 * a], y = src[3 * a + 1], z = src[3 * a + 2];
        if (!(isfinite(x) && isfinite(y) && isfinite(z))) bad = 1;
        sx += (double)x; sy += (double)y; sz += (double)z;
    }
    bad = __syncthreads_or(bad);
    red[0][tid] = sx; red[1][tid] = sy; red[2][tid] = sz;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; red[2][tid] += red[2][tid + o]; }
        __syncthreads();
    }
    const double cx = red[0][0] / (double)L, cy = red[1][0] / (double)L, cz = red[2][0] / (double)L;
    __syncthreads();
    double g = 0.0;
    for (int k = tid; k < L; k += 256) {
        const int a = idx ? idx[k] : k;
        double dx = 0.0, dy = 0.0, dz = 0.0;
        if ((unsigned)a < (unsigned)A) { dx = (double)src[3 * a] - cx; dy = (double)src[3 * a + 1] - cy; dz = (double)src[3 * a + 2] - cz; }
        out[3 * k] = dx; out[3 * k + 1] = dy; out[3 * k + 2] = dz;
        g = fma(dx, dx, g); g = fma(dy, dy, g); g = fma(dz, dz, g);
    }
    red[0][tid] = g;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[0][tid] += red[0][tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        out[3 * L] = red[0][0];
        out[3 * L + 1] = bad ? 0.0 : 1.0;
    }
}

__global__ __launch_bounds__(256) void bestfit_rmsd_kernel(const double* __restrict__ ws, const unsigned short* __restrict__ perms_t,
                                                          float* __restrict__ D, int* __restrict__ best_perm, double* __restrict__ quat,
                                                          int na, int nb, int L, int M, int TJ, int symmetric) {
    extern __shared__ double sm[];          // [TJ + 1][3 L | 1]: row i, then the columns of the tile
    __shared__ u64 red_v[4];
    __shared__ unsigned red_m[4];
    const int i = blockIdx.y, j0 = blockIdx.x * TJ, tid = threadIdx.x;
    if (symmetric && j0 + TJ - 1 < i) return;          // a tile left of the diagonal: mirrored from the upper triangle
    const int stride = bf_lds_stride(L), n3 = 3 * L;
    const long long wstride = bf_ws_stride(L);
    const double* row = ws + (long long)i * wstride;
    const double* cols = ws + (long long)(symmetric ? 0 : na) * wstride;
    for (int e = tid; e < n3; e += 256) sm[e] = row[e];
    for (int t = 0; t < TJ; ++t) {
        const int j = j0 + t;
        if (j >= nb || (symmetric && j <= i)) continue;
        const double* c = cols + (long long)j * wstride;
        double* dst = sm + (t + 1) * stride;
        for (int e = tid; e < n3; e += 256) dst[e] = c[e];
    }
    __syncthreads();
    const int G = 256 / TJ, t = tid / G, g = tid % G, j = j0 + t;
    const bool live = j < nb && !(symmetric && j <= i);
    const double* b = sm + (t + 1) * stride;
    double Gsum = 0.0;
    bool finite = false;
    if (live) {
        const double* c = cols + (long long)j * wstride;
        Gsum = row[n3] + c[n3];
        finite = row[n3 + 1] != 0.0 && c[n3 + 1] != 0.0;
    }
    pd_dkey best = {~0ull, 0xffffffffu};
    if (finite) {
        for (int m = g; m < M; m += G) {
            double S[9];
            bf_covariance(sm, b, perms_t, L, M, m, S);
            const double lam = horn_lambda_max<false>(S, nullptr);
            double msd = (Gsum - 2.0 * lam) / (double)L;
            if (!(msd > 0.0)) msd = 0.0;
            pd_dkey k = {(u64)__double_as_longlong(msd), (unsigned)m};
            best = pd_dkey_min(best, k);
        }
    }
    for (int o = (G < 64 ? G : 64) >> 1; o > 0; o >>= 1) best = pd_dkey_min(best, pd_dkey_xor(best, o));
    if (G == 256) {
        if ((tid & 63) == 0) { red_v[tid >> 6] = best.v; red_m[tid >> 6] = best.m; }
        __syncthreads();
        best.v = red_v[0]; best.m = red_m[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) { pd_dkey k = {red_v[w], red_m[w]}; best = pd_dkey_min(best, k); }
    }
    if (g != 0 || j >= nb) return;
    if (symmetric && j <= i) {
        if (j == i) D[(long long)i * nb + i] = 0.f;
        return;
    }
    const long long o = (long long)i * nb + j;
    if (!finite) {
        const float nanf_ = __int_as_float(0x7fc00000);
        D[o] = nanf_;
        if (symmetric) D[(long long)j * nb + i] = nanf_;
        if (best_perm) best_perm[o] = -1;
        if (quat) {
            const double nand = __longlong_as_double(0x7ff8000000000000ll);
            quat[4 * o] = nand; quat[4 * o + 1] = nand; quat[4 * o + 2] = nand; quat[4 * o + 3] = nand;
        }
        return;
    }
    const float r = (float)sqrt(__longlong_as_double((long long)best.v));
    D[o] = r;
    if (symmetric) D[(long long)j * nb + i] = r;
    if (best_perm) best_perm[o] = (int)best.m;
    if (quat) {
        double S[9], q[4];
        bf_covariance(sm, b, perms_t, L, M, (int)best.m, S);
        horn_lambda_max<true>(S, q);
        quat[4 * o] = q[0]; quat[4 * o + 1] = q[1]; quat[4 * o + 2] = q[2]; quat[4 * o + 3] = q[3];
    }
}

}  // namespace

PD_EXPORT int pd_bestfit_rmsd_workspace_numel(int na, int nb, int L) {
    if (na < 1 || nb < 1 || L < 1) return PD_ERR_ARG;
    if (L > BF_MAX_L || na > BF_MAX_N || nb > BF_MAX_N) return PD_ERR_UNSUPPORTED;
    return (int)(((long long)na + nb) * bf_ws_stride(L));           // at most 131070 * 3074 < 2^31
}

PD_EXPORT int pd_bestfit_rmsd(const float* xa, const int* idx_a, const float* xb, const int* idx_b, const unsigned short* perms_t,
                              double* ws, long long ws_numel, float* D, int* best_perm, double* quat, int na, int nb, int Aa, int Ab,
                              int L, int M, int symmetric, void* stream) {
    if (!xa || !ws || !D || na < 1 || nb < 1 || Aa < 1 || L < 1 || M < 1 || (!perms_t && M != 1)) return PD_ERR_ARG;
    if (symmetric) {
        if ((xb && xb != xa) || nb != na || best_perm || quat) return PD_ERR_ARG;
    } else if (!xb || Ab < 1 || (!idx_b && Ab < L)) {
        return PD_ERR_ARG;
    }
    if (!idx_a && Aa < L) return PD_ERR_ARG;
    if (pd_misaligned(xa, 4) || pd_misaligned(xb, 4) || pd_misaligned(idx_a, 4) || pd_misaligned(idx_b, 4) || pd_misaligned(perms_t, 2) ||
        pd_misaligned(ws, 8) || pd_misaligned(D, 4) || pd_misaligned(best_perm, 4) || pd_misaligned(quat, 8))
        return PD_ERR_ARG;
    if (L > BF_MAX_L || M > BF_MAX_M || na > BF_MAX_N || nb > BF_MAX_N) return PD_ERR_UNSUPPORTED;
    if (ws_numel < ((long long)na + nb) * bf_ws_stride(L)) return PD_ERR_ARG;
    const int ns = symmetric ? na : na + nb;
    hipLaunchKernelGGL(bestfit_prepare_kernel, dim3(ns), dim3(256), 0, (hipStream_t)stream, xa, idx_a, na, Aa, xb, idx_b, Ab, L, ws);
    const int tj = bf_tile(L, M);
    hipLaunchKernelGGL(bestfit_rmsd_kernel, dim3((nb + tj - 1) / tj, na), dim3(256), (size_t)(tj + 1) * bf_lds_stride(L) * sizeof(double),
                       (hipStream_t)stream, (const double*)ws, perms_t, D, best_perm, quat, na, nb, L, M, tj, symmetric ? 1 : 0);
    return pd_check_launch();
}
