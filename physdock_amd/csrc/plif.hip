// Protein - ligand interaction fingerprint of P poses of one ligand in its receptor: which residues does a pose touch, and how?
// (physdock_amd/interactions.py builds the tables once per system; the same definition stands in its docstring.)
//
// One system: a ligand of L atoms (pose atoms lig_idx[L]; lig_active[i] == 0: the atom takes no part - a hydrogen), the receptor
// atoms - heavy atoms that exist and are not ligand atoms - as a list sorted by residue (CSR: the atoms of residue s are
// res_atom[res_start[s] .. res_start[s + 1]), N = res_start[R] in all; residue ids need not be contiguous in atom order and a
// residue may own no receptor atom), one type byte per pose atom (bit 4 HYDROPHOBIC, bit 5 DONOR, bit 6 ACCEPTOR, as pd_vina_score
// reads it; bits 0 - 3 are not looked at) and one charge byte (bit 0 CATION, bit 1 ANION).
//
// A pair (active ligand atom i, receptor atom j) of a pose with the centre distance
//   r = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)))                       (the r of vina.hip)
// shows one or more of six kinds; bit k of a byte stands for kind k:
//
//   bit  kind            condition                                        threshold (default)
//   0    contact         any pair                                         r < thresholds[0]  (4.0 A)
//   1    hydrophobic     both atoms HYDROPHOBIC                           r < thresholds[1]  (4.5 A)
//   2    hbond_donor     ligand atom DONOR, receptor atom ACCEPTOR        r < thresholds[2]  (3.5 A)
//   3    hbond_acceptor  ligand atom ACCEPTOR, receptor atom DONOR        r < thresholds[2]  (3.5 A)
//   4    cationic        ligand atom CATION, receptor atom ANION          r < thresholds[3]  (4.5 A)
//   5    anionic         ligand atom ANION, receptor atom CATION          r < thresholds[3]  (4.5 A)
//
// Bits 6 and 7 are always 0.  No hydrogens are predicted, so there is no donor - H - acceptor angle test; pi-stacking, pi-cation,
// halogen and metal interactions and water bridges are out of scope (they need ring centroids and normals).
//
//   bits[p][s]         OR over the pairs whose receptor atom lies in residue s
//   ligand_bits[p][i]  OR over the receptor atoms, for ligand atom i; an inactive atom stores 0
//   min_dist[p][s]     the exact minimum of r over the residue's pairs; +inf for a residue without receptor atom or when no ligand
//                      atom is active
//   counts[p][k]       the number of residues whose byte has bit k
//
// The residue side is an OR (and a minimum) over ligand atoms, so it does not change when ligand atoms of equal type and charge
// swap places: it is invariant under the ligand's automorphisms.
//
// Every pair is visited twice, once per reduction.  plif_ligand_kernel: one block per (ligand atom, pose), 256 threads striding
// the receptor list; OR butterfly inside a wave, then the four waves through LDS.  plif_atom_kernel: one thread per (entry of the
// receptor list, pose); the ligand's coordinates and class bytes are staged in LDS (13 KB at L = 1024) and every thread walks
// them in ascending order, writing its atom's byte and minimum into the workspace [P][N].  plif_residue_kernel: one block per
// pose, one thread per residue folds the residue's run of the workspace and counts the kinds (integer sums).  plif_compare_kernel
// (one block per pose) and plif_pairwise_kernel (one thread per pair of poses, PAIR_TILE x PAIR_TILE pairs per block, the rows
// staged in LDS in chunks of 256 bytes) count set bits and do one fp32 division.  No atomics, no scratch memory; OR, minimum and
// integer sums do not depend on their order, every value depends on its own pose (or pair of poses) alone and on no launch
// dimension: results are bit-identical from run to run, whatever P is and wherever a pose sits.
#include "common.h"
#include "physdock_hip.h"

namespace {

constexpr int PLIF_MAX_L = 1024;
constexpr int PLIF_MAX_A = 1 << 22;
constexpr int PLIF_MAX_P = 65535;
constexpr int PAIR_TILE = 16;                 // poses per side of a pairwise block
constexpr int PAIR_WORDS = 64;                // 4-byte words of a row staged per chunk
static_assert(PD_PLIF_KINDS == 6 && PD_PLIF_THRESHOLDS == 4, "the counts the header documents");

struct PlifThresholds {
    float contact, hydrophobic, hbond, ionic;
};

// Class bytes: bit k of (ligand class & receptor class) says that the pair's types allow kind k.
//   ligand:   bit 0 set, 1 HYDROPHOBIC, 2 DONOR,    3 ACCEPTOR, 4 CATION, 5 ANION
//   receptor: bit 0 set, 1 HYDROPHOBIC, 2 ACCEPTOR, 3 DONOR,    4 ANION,  5 CATION
__device__ __forceinline__ unsigned plif_ligand_class(unsigned type, unsigned charge) {
    return 1u | ((type >> 3) & 14u) | ((charge & 3u) << 4);
}
__device__ __forceinline__ unsigned plif_receptor_class(unsigned type, unsigned charge) {
    return 1u | ((type >> 3) & 2u) | ((type >> 4) & 4u) | ((type >> 2) & 8u) | ((charge & 2u) << 3) | ((charge & 1u) << 5);
}
// bit k: r is below the threshold of kind k
__device__ __forceinline__ unsigned plif_near(float r, PlifThresholds t) {
    return (r < t.contact ? 1u : 0u) | (r < t.hydrophobic ? 2u : 0u) | (r < t.hbond ? 12u : 0u) | (r < t.ionic ? 48u : 0u);
}
__device__ __forceinline__ float plif_distance(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
}
// one fp32 division of two integers; 1 where the denominator is 0
__device__ __forceinline__ float plif_ratio(int num, int den) { return den == 0 ? 1.f : (float)num / (float)den; }


__global__ __launch_bounds__(256) void plif_ligand_kernel(const float* __restrict__ x, const int* __restrict__ lig_idx,
                                                         const unsigned char* __restrict__ type,
                                                         const unsigned char* __restrict__ charge,
                                                         const unsigned char* __restrict__ lig_active,
                                                         const int* __restrict__ res_atom, PlifThresholds thr,
                                                         unsigned char* __restrict__ ligand_bits, int A, int L, int N) {
    __shared__ int red[4];
    const int tid = threadIdx.x, i = blockIdx.x, p = blockIdx.y;
    const float* xp = x + (long long)p * A * 3;
    int b = 0;
    if (lig_active[i]) {                                             // uniform over the block
        const int a = lig_idx[i];
        const float ax = xp[3 * a], ay = xp[3 * a + 1], az = xp[3 * a + 2];
        const unsigned lc = plif_ligand_class(type[a], charge[a]);
        for (int n = tid; n < N; n += 256) {
            const int j = res_atom[n];
            const float r = plif_distance(ax, ay, az, xp[3 * j], xp[3 * j + 1], xp[3 * j + 2]);
            b |= (int)(lc & plif_receptor_class(type[j], charge[j]) & plif_near(r, thr));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) b |= __shfl_xor(b, o);
    if ((tid & 63) == 0) red[tid >> 6] = b;
    __syncthreads();
    if (tid == 0) ligand_bits[(long long)p * L + i] = (unsigned char)(red[0] | red[1] | red[2] | red[3]);
}

__global__ __launch_bounds__(256) void plif_atom_kernel(const float* __restrict__ x, const int* __restrict__ lig_idx,
                                                       const unsigned char* __restrict__ type,
                                                       const unsigned char* __restrict__ charge,
                                                       const unsigned char* __restrict__ lig_active,
                                                       const int* __restrict__ res_atom, PlifThresholds thr,
                                                       unsigned char* __restrict__ ws_bits, float* __restrict__ ws_min, int A, int L,
                                                       int N) {
    __shared__ float lx[PLIF_MAX_L * 3];
    __shared__ unsigned char lc[PLIF_MAX_L];                         // 0: the ligand atom is inactive
    const int tid = threadIdx.x, p = blockIdx.y, n = blockIdx.x * 256 + tid;
    const float* xp = x + (long long)p * A * 3;
    for (int i = tid; i < L; i += 256) {
        const int a = lig_idx[i];
        lx[3 * i] = xp[3 * a];
        lx[3 * i + 1] = xp[3 * a + 1];
        lx[3 * i + 2] = xp[3 * a + 2];
        lc[i] = lig_active[i] ? (unsigned char)plif_ligand_class(type[a], charge[a]) : (unsigned char)0;
    }
    __syncthreads();
    if (n >= N) return;
    const int j = res_atom[n];
    const float bx = xp[3 * j], by = xp[3 * j + 1], bz = xp[3 * j + 2];
    const unsigned rc = plif_receptor_class(type[j], charge[j]);
    unsigned b = 0;
    float m = INFINITY;
    for (int i = 0; i < L; ++i) {                                    // every thread reads the same LDS word: a broadcast
        const unsigned c = lc[i];
        if (!c) continue;
        const float r = plif_distance(lx[3 * i], lx[3 * i + 1], lx[3 * i + 2], bx, by, bz);
        b |= c & rc & plif_near(r, thr);
        m = fminf(m, r);
    }
    ws_bits[(long long)p * N + n] = (unsigned char)b;
    ws_min[(long long)p * N + n] = m;
}

__global__ __launch_bounds__(256) void plif_residue_kernel(const unsigned char* __restrict__ ws_bits, const float* __restrict__ ws_min,
                                                          const int* __restrict__ res_start, unsigned char* __restrict__ bits,
                                                          float* __restrict__ min_dist, int* __restrict__ counts, int R, int N) {
    __shared__ int red[4][PD_PLIF_KINDS];
    const int tid = threadIdx.x, p = blockIdx.x;
    const unsigned char* wb = ws_bits + (long long)p * N;
    const float* wm = ws_min + (long long)p * N;
    int cnt[PD_PLIF_KINDS] = {0, 0, 0, 0, 0, 0};
    for (int s = tid; s < R; s += 256) {
        unsigned b = 0;
        float m = INFINITY;
        for (int n = res_start[s], e = res_start[s + 1]; n < e; ++n) {
            b |= wb[n];
            m = fminf(m, wm[n]);
        }
        bits[(long long)p * R + s] = (unsigned char)b;
        min_dist[(long long)p * R + s] = m;
#pragma unroll
        for (int k = 0; k < PD_PLIF_KINDS; ++k) cnt[k] += (int)((b >> k) & 1u);
    }
#pragma unroll
    for (int k = 0; k < PD_PLIF_KINDS; ++k) {
        const int s = wave_sum(cnt[k]);
        if ((tid & 63) == 0) red[tid >> 6][k] = s;
    }
    __syncthreads();
    if (tid < PD_PLIF_KINDS) counts[p * PD_PLIF_KINDS + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

__global__ __launch_bounds__(256) void plif_compare_kernel(const unsigned char* __restrict__ bits, const unsigned char* __restrict__ ref,
                                                          unsigned mask, int* __restrict__ shared, int* __restrict__ n_pose,
                                                          int* __restrict__ n_ref, float* __restrict__ recovery,
                                                          float* __restrict__ tanimoto, int R) {
    __shared__ int red[4][3];
    const int tid = threadIdx.x, p = blockIdx.x;
    const unsigned char* row = bits + (long long)p * R;
    int c[3] = {0, 0, 0};                                            // shared, pose, reference
    for (int s = tid; s < R; s += 256) {
        const unsigned a = row[s] & mask, b = ref[s] & mask;
        c[0] += __popc(a & b);
        c[1] += __popc(a);
        c[2] += __popc(b);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int s = wave_sum(c[k]);
        if ((tid & 63) == 0) red[tid >> 6][k] = s;
    }
    __syncthreads();
    if (tid == 0) {
        const int sh = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
        const int np = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
        const int nr = ((red[0][2] + red[1][2]) + red[2][2]) + red[3][2];
        shared[p] = sh;
        n_pose[p] = np;
        if (p == 0) n_ref[0] = nr;
        recovery[p] = plif_ratio(sh, nr);
        tanimoto[p] = plif_ratio(sh, np + nr - sh);
    }
}

__global__ __launch_bounds__(256) void plif_pairwise_kernel(const unsigned char* __restrict__ bits, unsigned mask4,
                                                           float* __restrict__ tanimoto, int P, int R) {
    __shared__ unsigned rows[2][PAIR_TILE][PAIR_WORDS + 1];          // + 1: the sixteen rows a wave reads lie in sixteen banks
    const int tid = threadIdx.x, tp = tid >> 4, tq = tid & 15;
    const int p0 = blockIdx.y * PAIR_TILE, q0 = blockIdx.x * PAIR_TILE;
    int sh = 0, na = 0, nb = 0;
    for (int c0 = 0; c0 < R; c0 += PAIR_WORDS * 4) {
        __syncthreads();
        for (int e = tid; e < 2 * PAIR_TILE * PAIR_WORDS; e += 256) {
            const int side = e / (PAIR_TILE * PAIR_WORDS), row = (e / PAIR_WORDS) % PAIR_TILE, w = e % PAIR_WORDS;
            const int pose = (side ? q0 : p0) + row;
            unsigned v = 0;
            if (pose < P) {
                const unsigned char* src = bits + (long long)pose * R;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int s = c0 + 4 * w + k;
                    if (s < R) v |= (unsigned)src[s] << (8 * k);
                }
            }
            rows[side][row][w] = v & mask4;
        }
        __syncthreads();
#pragma unroll 8
        for (int w = 0; w < PAIR_WORDS; ++w) {
            const unsigned a = rows[0][tp][w], b = rows[1][tq][w];
            sh += __popc(a & b);
            na += __popc(a);
            nb += __popc(b);
        }
    }
    const int p = p0 + tp, q = q0 + tq;
    if (p < P && q < P) tanimoto[(long long)p * P + q] = plif_ratio(sh, na + nb - sh);
}

inline bool misaligned4(const void* a) { return ((uintptr_t)a & 3) != 0; }

}  // namespace

PD_EXPORT int pd_plif_fingerprint(const float* x, const int* lig_idx, const unsigned char* type, const unsigned char* charge,
                                  const unsigned char* lig_active, const int* res_start, const int* res_atom, const float* thresholds,
                                  unsigned char* ws_bits, float* ws_min, unsigned char* bits, unsigned char* ligand_bits,
                                  float* min_dist, int* counts, int P, int A, int L, int R, int N, void* stream) {
    if (!x || !lig_idx || !type || !charge || !lig_active || !res_start || !thresholds || !bits || !ligand_bits || !min_dist || !counts)
        return PD_ERR_ARG;
    if (P <= 0 || A <= 0 || L <= 0 || R <= 0 || N < 0 || N > A) return PD_ERR_ARG;
    if (N > 0 && (!res_atom || !ws_bits || !ws_min)) return PD_ERR_ARG;
    if (misaligned4(x) || misaligned4(lig_idx) || misaligned4(res_start) || misaligned4(res_atom) || misaligned4(ws_min) ||
        misaligned4(min_dist) || misaligned4(counts))
        return PD_ERR_ARG;
    for (int k = 0; k < PD_PLIF_THRESHOLDS; ++k)
        if (!(thresholds[k] >= 0.f) || !(thresholds[k] <= 3.0e38f)) return PD_ERR_ARG;          // negative, NaN or infinite
    if (L > PLIF_MAX_L || A > PLIF_MAX_A || P > PLIF_MAX_P || R > A) return PD_ERR_UNSUPPORTED;
    const PlifThresholds thr = {thresholds[0], thresholds[1], thresholds[2], thresholds[3]};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(plif_ligand_kernel, dim3(L, P), dim3(256), 0, s, x, lig_idx, type, charge, lig_active, res_atom, thr, ligand_bits,
                       A, L, N);
    if (N > 0)
        hipLaunchKernelGGL(plif_atom_kernel, dim3((N + 255) / 256, P), dim3(256), 0, s, x, lig_idx, type, charge, lig_active, res_atom,
                           thr, ws_bits, ws_min, A, L, N);
    hipLaunchKernelGGL(plif_residue_kernel, dim3(P), dim3(256), 0, s, (const unsigned char*)ws_bits, (const float*)ws_min, res_start,
                       bits, min_dist, counts, R, N);
    return pd_check_launch();
}

PD_EXPORT int pd_plif_compare(const unsigned char* bits, const unsigned char* ref_bits, int kind_mask, int* shared, int* n_pose,
                              int* n_ref, float* recovery, float* tanimoto, int P, int R, void* stream) {
    if (!bits || !ref_bits || !shared || !n_pose || !n_ref || !recovery || !tanimoto) return PD_ERR_ARG;
    if (P <= 0 || R <= 0 || kind_mask < 0 || kind_mask >= (1 << PD_PLIF_KINDS)) return PD_ERR_ARG;
    if (misaligned4(shared) || misaligned4(n_pose) || misaligned4(n_ref) || misaligned4(recovery) || misaligned4(tanimoto))
        return PD_ERR_ARG;
    if (P > PLIF_MAX_P || R > PLIF_MAX_A) return PD_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(plif_compare_kernel, dim3(P), dim3(256), 0, (hipStream_t)stream, bits, ref_bits, (unsigned)kind_mask, shared,
                       n_pose, n_ref, recovery, tanimoto, R);
    return pd_check_launch();
}

PD_EXPORT int pd_plif_pairwise(const unsigned char* bits, int kind_mask, float* tanimoto, int P, int R, void* stream) {
    if (!bits || !tanimoto) return PD_ERR_ARG;
    if (P <= 0 || R <= 0 || kind_mask < 0 || kind_mask >= (1 << PD_PLIF_KINDS)) return PD_ERR_ARG;
    if (misaligned4(tanimoto)) return PD_ERR_ARG;
    if (P > PLIF_MAX_P || R > PLIF_MAX_A) return PD_ERR_UNSUPPORTED;
    const int tiles = (P + PAIR_TILE - 1) / PAIR_TILE;
    hipLaunchKernelGGL(plif_pairwise_kernel, dim3(tiles, tiles), dim3(256), 0, (hipStream_t)stream, bits, 0x01010101u * (unsigned)kind_mask,
                       tanimoto, P, R);
    return pd_check_launch();
}
