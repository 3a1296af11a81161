// Symmetry-corrected ligand RMSD for pose ranking: the pairwise RMSD matrix of pd_pairwise_rmsd (sampler.hip) with the minimum
// over a table of graph automorphisms of the ligand (physdock_amd/symmetry.py), and the same against a reference structure.
//
//   D[i,j] = D[j,i] = sqrt( min_m (1/L) sum_a |x_i[idx[a]] - x_j[idx[perms[m][a]]]|^2 )      (i < j; D[i,i] = 0)
//
// One block per (pose i, tile of TJ poses j; column j == n is the reference).  The ligand coordinates of pose i and of the
// tile are gathered into LDS once (16 bytes per atom, so that a permuted atom is ONE ds_read_b128); threads own permutations
// and stride over m, and every table entry a thread loads serves all TJ poses of the tile.  The table is atom-major
// (perms_t[a][m]), so the 64 lanes of a wave read 128 contiguous bytes per atom.  Each permutation's sum is taken by one
// thread over a in ascending order with explicit fmaf, and the minimum over m is exact (the key (bits of the sum, m) is
// ordered as the pair is, because the sums are non-negative), so results do not depend on the launch shape and the smallest
// m wins a tie.  No atomics, no scratch buffer: the block minimum is a wave reduction and one LDS step over the four waves.
#include "common.h"
#include "physdock_hip.h"

namespace {

constexpr int SYM_MAX_L = 1024;        // ligand atoms: (TJ + 1) * 16 * L bytes of LDS stay below 64 KiB (TJ = 4 up to 768 atoms, else 2)
constexpr int SYM_MAX_M = 65535;       // table rows: an unsigned short entry addresses an atom, the key's low word holds m
constexpr int SYM_TJ_WIDE_MAX_L = 768;

typedef pd_u64 u64;

template <int TJ>
__global__ __launch_bounds__(256) void sym_rmsd_kernel(const float* __restrict__ x, const int* __restrict__ idx,
                                                      const float* __restrict__ ref, const unsigned short* __restrict__ perms_t,
                                                      float* __restrict__ D, float* __restrict__ rmsd_ref,
                                                      int* __restrict__ best_perm_ref, int n, int A, int L, int M) {
    extern __shared__ f32x4 sm[];          // [TJ + 1][L]: pose i, then the poses of the tile
    __shared__ u64 red[4][TJ];
    const int i = blockIdx.y, j0 = blockIdx.x * TJ;
    if (j0 + TJ - 1 < i) return;           // a tile left of the diagonal: its values are mirrored from the upper triangle
    const int tid = threadIdx.x;
    const float* src[TJ + 1];
    src[0] = x + (long long)i * A * 3;
#pragma unroll
    for (int t = 0; t < TJ; ++t) {
        const int j = j0 + t;
        src[t + 1] = (j > i && j < n) ? x + (long long)j * A * 3 : ((j == n && ref) ? ref : nullptr);
    }
    for (int a = tid; a < L; a += 256) {
        const int k = idx ? idx[a] : a;
#pragma unroll
        for (int t = 0; t <= TJ; ++t) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (src[t]) { v[0] = src[t][3 * k]; v[1] = src[t][3 * k + 1]; v[2] = src[t][3 * k + 2]; }
            sm[t * L + a] = v;
        }
    }
    __syncthreads();
    u64 best[TJ];
#pragma unroll
    for (int t = 0; t < TJ; ++t) best[t] = ~0ull;
    for (int m = tid; m < M; m += 256) {
        float acc[TJ];
#pragma unroll
        for (int t = 0; t < TJ; ++t) acc[t] = 0.f;
        const unsigned short* pm = perms_t + m;
#pragma unroll 4
        for (int a = 0; a < L; ++a) {
            const int p = pm[(long long)a * M];
            const f32x4 xi = sm[a];
#pragma unroll
            for (int t = 0; t < TJ; ++t) {
                const f32x4 xj = sm[(t + 1) * L + p];
                const float dx = xi[0] - xj[0], dy = xi[1] - xj[1], dz = xi[2] - xj[2];
                acc[t] = acc[t] + fmaf(dz, dz, fmaf(dy, dy, dx * dx));
            }
        }
#pragma unroll
        for (int t = 0; t < TJ; ++t) best[t] = pd_key_min(best[t], ((u64)__float_as_uint(acc[t]) << 32) | (unsigned)m);
    }
#pragma unroll
    for (int t = 0; t < TJ; ++t) {
        const u64 k = pd_wave_key_min(best[t]);
        if ((tid & 63) == 0) red[tid >> 6][t] = k;
    }
    __syncthreads();
    if (tid < TJ) {
        const int j = j0 + tid;
        const u64 k = pd_key_min(pd_key_min(red[0][tid], red[1][tid]), pd_key_min(red[2][tid], red[3][tid]));
        const float r = sqrtf(__uint_as_float((unsigned)(k >> 32)) / (float)L);
        if (j == i) {
            D[(long long)i * n + i] = 0.f;
        } else if (j > i && j < n) {
            D[(long long)i * n + j] = r;
            D[(long long)j * n + i] = r;
        } else if (j == n && ref) {
            rmsd_ref[i] = r;
            if (best_perm_ref) best_perm_ref[i] = (int)(unsigned)(k & 0xffffffffull);
        }
    }
}

}  // namespace

PD_EXPORT int pd_sym_rmsd(const float* x, const int* idx, const float* ref, const unsigned short* perms_t, float* D,
                          float* rmsd_ref, int* best_perm_ref, int n, int A, int L, int M, void* stream) {
    if (!x || !perms_t || !D || n <= 0 || A <= 0 || L <= 0 || M <= 0 || (ref && !rmsd_ref)) return PD_ERR_ARG;
    if (L > SYM_MAX_L || M > SYM_MAX_M || n > 65535) return PD_ERR_UNSUPPORTED;
    if (L <= SYM_TJ_WIDE_MAX_L)
        hipLaunchKernelGGL(sym_rmsd_kernel<4>, dim3((n + 1 + 3) / 4, n), dim3(256), (size_t)5 * L * sizeof(f32x4), (hipStream_t)stream,
                           x, idx, ref, perms_t, D, rmsd_ref, best_perm_ref, n, A, L, M);
    else
        hipLaunchKernelGGL(sym_rmsd_kernel<2>, dim3((n + 1 + 1) / 2, n), dim3(256), (size_t)3 * L * sizeof(f32x4), (hipStream_t)stream,
                           x, idx, ref, perms_t, D, rmsd_ref, best_perm_ref, n, A, L, M);
    return pd_check_launch();
}
