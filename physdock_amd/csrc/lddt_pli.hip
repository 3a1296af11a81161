// lDDT-PLI of P poses of one ligand in its receptor against one ground truth, maximised over a table of graph automorphisms of
// the ligand (physdock_amd/lddt_pli.py builds the tables once per system).  With N(i) the receptor atoms within the inclusion
// radius of ligand atom i in the ground truth and d_gt(i,j) their distances there (fp32, from the host):
//
//   c_t(i,k) = #{ j in N(i) : | |x[lig[k]] - x[j]| - d_gt(i,j) | < thr[t] }        (t = 0 .. 3; k a candidate image of i)
//   C_t(m)   = sum_i c_t(i, perms[m][i]),   m* = the smallest m that maximises sum_t C_t(m)
//   lddt_pli = sum_t C_t(m*) / (4 sum_i |N(i)|)                                     (0 without contacts)
//
// Two kernels, no atomics, no scratch memory.  lddt_pli_counts_kernel: one block per (ligand atom i, pose).  A thread keeps
// CPT contacts of i in registers (pose coordinates of the receptor atom and d_gt: nothing is shared between threads, so the tile
// needs no LDS), the block walks the candidates of i - the distinct images perms[:, i], a handful for a real ligand - and every
// candidate costs one distance and four compares per contact.  The four counts of a thread travel packed in one dword through
// the wave reduction (8 bits each: at most 64 * CPT per wave) and are unpacked before the step over the four waves.  An atom
// with more than LDDT_TILE contacts takes several passes; thread t < 4 owns counts[p][c][t] and adds to what it stored itself.
// lddt_pli_select_kernel: one block per pose.  The totals sum_t c_t of all candidates sit in LDS (read from the counts in global
// memory beyond LDDT_LDS_CAND candidates); threads own permutations and stride over m, reading the slot table atom-major
// (slot_t[i][m]: 64 lanes read 128 contiguous bytes per atom, as sym_rmsd.hip reads its table).  The key (~total, m) is
// minimised exactly, so the smallest m wins a tie; all sums are integers, so no result depends on the launch shape.
#include "common.h"
#include "physdock_hip.h"

namespace {

constexpr int LDDT_MAX_L = 1024;       // ligand atoms (the symmetry table's limits)
constexpr int LDDT_MAX_M = 65535;      // table rows: an unsigned short slot, the key's low word holds m
constexpr int LDDT_CPT = 2;            // contacts a thread of the counts kernel keeps in registers
constexpr int LDDT_TILE = 256 * LDDT_CPT;
constexpr int LDDT_LDS_CAND = 4096;    // candidates whose totals the select kernel keeps in LDS (16 KiB)
static_assert(LDDT_TILE == PD_LDDT_PLI_TILE && LDDT_LDS_CAND == PD_LDDT_PLI_LDS_CAND, "the constants the header documents");
static_assert(64 * LDDT_CPT < 256, "a wave's count must fit the 8-bit field of the packed reduction");


struct lddt_thresholds { float t[4]; };

__global__ __launch_bounds__(256) void lddt_pli_counts_kernel(const float* __restrict__ x, const int* __restrict__ lig_idx,
                                                             const int* __restrict__ contact_start,
                                                             const int* __restrict__ contact_atom,
                                                             const float* __restrict__ contact_dist,
                                                             const int* __restrict__ cand_start, const int* __restrict__ cand_atom,
                                                             const lddt_thresholds thr, int* __restrict__ counts, int A, int n_cand) {
    __shared__ unsigned red[2][4];
    const int tid = threadIdx.x, i = blockIdx.x, p = blockIdx.y;
    const float* xp = x + (long long)p * A * 3;
    const int cs = contact_start[i], ce = contact_start[i + 1], ks = cand_start[i], ke = cand_start[i + 1];
    int* out = counts + ((long long)p * n_cand + ks) * 4;
    int c0 = cs, step = 0;
    do {                                   // at least one pass: an atom without contacts stores its zeros
        float cx[LDDT_CPT], cy[LDDT_CPT], cz[LDDT_CPT], cd[LDDT_CPT];
        bool have[LDDT_CPT];
#pragma unroll
        for (int e = 0; e < LDDT_CPT; ++e) {
            const int c = c0 + e * 256 + tid;
            have[e] = c < ce;
            cx[e] = cy[e] = cz[e] = cd[e] = 0.f;
            if (have[e]) {
                const int j = contact_atom[c];
                cx[e] = xp[3 * j]; cy[e] = xp[3 * j + 1]; cz[e] = xp[3 * j + 2]; cd[e] = contact_dist[c];
            }
        }
        for (int k = ks; k < ke; ++k) {
            const int a = lig_idx[cand_atom[k]];
            const float ax = xp[3 * a], ay = xp[3 * a + 1], az = xp[3 * a + 2];
            unsigned packed = 0;
#pragma unroll
            for (int e = 0; e < LDDT_CPT; ++e) {
                const float dx = ax - cx[e], dy = ay - cy[e], dz = az - cz[e];
                const float diff = fabsf(sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx))) - cd[e]);
#pragma unroll
                for (int t = 0; t < 4; ++t) packed += (have[e] && diff < thr.t[t]) ? 1u << (8 * t) : 0u;
            }
            packed = wave_sum(packed);
            unsigned* r = red[step++ & 1];     // two buffers: the readers of one step are done before the step after the next stores
            if ((tid & 63) == 0) r[tid >> 6] = packed;
            __syncthreads();
            if (tid < 4) {
                const int s = (int)((r[0] >> (8 * tid) & 255u) + (r[1] >> (8 * tid) & 255u) + (r[2] >> (8 * tid) & 255u) +
                                    (r[3] >> (8 * tid) & 255u));
                int* o = out + (long long)(k - ks) * 4 + tid;
                *o = c0 == cs ? s : *o + s;
            }
        }
        c0 += LDDT_TILE;
    } while (c0 < ce);
}

__device__ __forceinline__ int total_of(const int* __restrict__ cnt, int c) {
    const int4 v = *reinterpret_cast<const int4*>(cnt + (long long)c * 4);
    return v.x + v.y + v.z + v.w;
}

__global__ __launch_bounds__(256) void lddt_pli_select_kernel(const int* __restrict__ counts, const int* __restrict__ contact_start,
                                                             const int* __restrict__ cand_start,
                                                             const unsigned short* __restrict__ slot_t, float* __restrict__ lddt,
                                                             int* __restrict__ conserved, float* __restrict__ per_atom,
                                                             int* __restrict__ best_perm, int L, int M, int n_cand) {
    __shared__ int tot[LDDT_LDS_CAND];
    __shared__ pd_u64 redk[4];
    __shared__ int redc[4][4];
    const int tid = threadIdx.x, p = blockIdx.x;
    const int* cnt = counts + (long long)p * n_cand * 4;
    const bool in_lds = n_cand <= LDDT_LDS_CAND;
    if (in_lds) {
        for (int c = tid; c < n_cand; c += 256) tot[c] = total_of(cnt, c);
        __syncthreads();
    }
    pd_u64 best = ~0ull;
    for (int m = tid; m < M; m += 256) {
        const unsigned short* sm = slot_t + m;
        int sum = 0;
        if (in_lds) {
#pragma unroll 4
            for (int i = 0; i < L; ++i) sum += tot[cand_start[i] + sm[(long long)i * M]];
        } else {
            for (int i = 0; i < L; ++i) sum += total_of(cnt, cand_start[i] + sm[(long long)i * M]);
        }
        best = pd_key_min(best, ((pd_u64)(0xffffffffu - (unsigned)sum) << 32) | (unsigned)m);
    }
    best = pd_wave_key_min(best);
    if ((tid & 63) == 0) redk[tid >> 6] = best;
    __syncthreads();
    best = pd_key_min(pd_key_min(redk[0], redk[1]), pd_key_min(redk[2], redk[3]));
    const int m_best = (int)(unsigned)(best & 0xffffffffull);
    // the chosen permutation's counts: per atom, and summed per threshold
    int c4[4] = {0, 0, 0, 0};
    for (int i = tid; i < L; i += 256) {
        const int4 v = *reinterpret_cast<const int4*>(cnt + (long long)(cand_start[i] + slot_t[(long long)i * M + m_best]) * 4);
        const int n_i = contact_start[i + 1] - contact_start[i];
        c4[0] += v.x; c4[1] += v.y; c4[2] += v.z; c4[3] += v.w;
        per_atom[(long long)p * L + i] = n_i ? (float)(v.x + v.y + v.z + v.w) / (float)(4 * n_i) : 0.f;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int s = (int)wave_sum((unsigned)c4[t]);
        if ((tid & 63) == 0) redc[tid >> 6][t] = s;
    }
    __syncthreads();
    if (tid < 4) conserved[p * 4 + tid] = redc[0][tid] + redc[1][tid] + redc[2][tid] + redc[3][tid];
    if (tid == 0) {
        const int total = (int)(0xffffffffu - (unsigned)(best >> 32)), n = contact_start[L];
        best_perm[p] = m_best;
        lddt[p] = n ? (float)total / (float)(4 * (long long)n) : 0.f;
    }
}

}  // namespace

PD_EXPORT int pd_lddt_pli_counts(const float* x, const int* lig_idx, const int* contact_start, const int* contact_atom,
                                 const float* contact_dist, const int* cand_start, const int* cand_atom, float thr0, float thr1,
                                 float thr2, float thr3, int* counts, int P, int A, int L, int n_contacts, int n_cand, void* stream) {
    if (!x || !lig_idx || !contact_start || !cand_start || !cand_atom || !counts || ((uintptr_t)counts & 15)) return PD_ERR_ARG;
    if (P <= 0 || A <= 0 || L <= 0 || n_contacts < 0 || n_cand < L) return PD_ERR_ARG;
    if (n_contacts && (!contact_atom || !contact_dist)) return PD_ERR_ARG;
    if (L > LDDT_MAX_L || P > 65535 || (long long)n_cand > (long long)L * L || n_contacts > PD_LDDT_PLI_MAX_CONTACTS)
        return PD_ERR_UNSUPPORTED;
    const lddt_thresholds thr = {{thr0, thr1, thr2, thr3}};
    hipLaunchKernelGGL(lddt_pli_counts_kernel, dim3(L, P), dim3(256), 0, (hipStream_t)stream, x, lig_idx, contact_start, contact_atom,
                       contact_dist, cand_start, cand_atom, thr, counts, A, n_cand);
    return pd_check_launch();
}

PD_EXPORT int pd_lddt_pli_select(const int* counts, const int* contact_start, const int* cand_start, const unsigned short* slot_t,
                                 float* lddt, int* conserved, float* per_atom, int* best_perm, int P, int L, int M, int n_cand,
                                 void* stream) {
    if (!counts || !contact_start || !cand_start || !slot_t || !lddt || !conserved || !per_atom || !best_perm) return PD_ERR_ARG;
    if (((uintptr_t)counts & 15) || P <= 0 || L <= 0 || M <= 0 || n_cand < L) return PD_ERR_ARG;
    if (L > LDDT_MAX_L || M > LDDT_MAX_M || P > 65535 || (long long)n_cand > (long long)L * L) return PD_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(lddt_pli_select_kernel, dim3(P), dim3(256), 0, (hipStream_t)stream, counts, contact_start, cand_start, slot_t,
                       lddt, conserved, per_atom, best_perm, L, M, n_cand);
    return pd_check_launch();
}
