// Vina-style receptor - ligand interaction score of P poses of one ligand in its receptor, with its analytic gradient on the
// ligand atoms (physdock_amd/scoring.py builds the type table once per system).  The functional form is the intermolecular part
// of the AutoDock Vina scoring function (Trott & Olson, J. Comput. Chem. 2010), heavy atoms only.  The sum runs over every active
// ligand atom i (pose atom lig_idx[i]) and every receptor atom j (rec_mask) of the same pose:
//
//   r = |x_i - x_j| = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));  the pair counts iff r < 8;  d = r - (R_i + R_j)
//   X-Score radii R by class (bits 0 - 3 of the type byte): C 1.9, N 1.8, O 1.7, P 2.1, S 2.0, F 1.5, Cl 1.8, Br 2.0, I 2.2, any
//   other element (metals, class 9 and above) 1.2
//
//   term          per pair                                                                      weight
//   gauss1        exp(-(d / 0.5)^2)                                                             -0.0356
//   gauss2        exp(-((d - 3) / 2)^2)                                                         -0.00516
//   repulsion     d^2 if d < 0, else 0                                                          +0.840
//   hydrophobic   both atoms hydrophobic (bit 4): 1 if d <= 0.5; 1.5 - d for 0.5 < d < 1.5; 0 beyond   -0.0351
//   hbond         one atom a donor (bit 5), the other an acceptor (bit 6): 1 if d <= -0.7; -d / 0.7 for -0.7 < d < 0; 0 beyond   -0.587
//
//   inter[p]  = sum_t w_t terms[p][t]                       score[p] = inter[p] / (1 + 0.0585 n_rot)          (kcal/mol)
//   forces[p][i] = -d inter[p] / d x_i                      (not scaled by the n_rot factor; a pair with r == 0 contributes 0)
//
// expf, not the fast intrinsic.  Out of scope: Vina's intramolecular term and any fit of the weights to this model's poses.
//
// Two kernels, no atomics, no scratch memory.  vina_atom_kernel: one block per (ligand atom, pose), 256 threads striding the
// pose's atoms; a thread keeps the five terms and the three gradient components in registers, the block reduces them in a fixed
// order (butterfly inside a wave, then waves 0 .. 3 in one thread) and one thread stores atom_terms[p][i][5] and forces[p][i][3].
// An inactive ligand atom stores zeros.  vina_pose_kernel: one block per pose; per_atom[p][i] is the weighted sum of atom i's five
// terms, terms[p][t] the sum over the atoms in ascending order (one thread per term), inter and score follow from the five sums.
// Every value depends on its own pose alone and on no launch dimension: results are bit-identical from run to run, whatever the
// number of poses in the call and wherever a pose sits among them.
#include "common.h"
#include "physdock_hip.h"

namespace {

constexpr int VINA_MAX_L = 1024;
constexpr int VINA_MAX_A = 1 << 22;
constexpr float VINA_CUTOFF = 8.0f;
constexpr float W_GAUSS1 = -0.0356f, W_GAUSS2 = -0.00516f, W_REPULSION = 0.840f, W_HYDROPHOBIC = -0.0351f, W_HBOND = -0.587f;
constexpr float VINA_ROT = 0.0585f;
static_assert(PD_VINA_TERMS == 5, "the term count the header documents");

__device__ const float VINA_RADIUS[16] = {1.9f, 1.8f, 1.7f, 2.1f, 2.0f, 1.5f, 1.8f, 2.0f, 2.2f, 1.2f, 1.2f, 1.2f, 1.2f, 1.2f, 1.2f, 1.2f};

__global__ __launch_bounds__(256) void vina_atom_kernel(const float* __restrict__ x, const int* __restrict__ lig_idx,
                                                       const unsigned char* __restrict__ type,
                                                       const unsigned char* __restrict__ rec_mask,
                                                       const unsigned char* __restrict__ lig_active,
                                                       float* __restrict__ atom_terms, float* __restrict__ forces, int A, int L) {
    __shared__ float red[4][8];
    const int tid = threadIdx.x, i = blockIdx.x, p = blockIdx.y;
    const float* xp = x + (long long)p * A * 3;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};          // gauss1, gauss2, repulsion, hydrophobic, hbond, d inter / d x_i
    if (lig_active[i]) {                                             // uniform over the block
        const int a = lig_idx[i];
        const float ax = xp[3 * a], ay = xp[3 * a + 1], az = xp[3 * a + 2];
        const unsigned ti = type[a];
        const float ri = VINA_RADIUS[ti & 15];
        for (int j = tid; j < A; j += 256) {
            if (!rec_mask[j]) continue;
            const float dx = ax - xp[3 * j], dy = ay - xp[3 * j + 1], dz = az - xp[3 * j + 2];
            const float r = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
            if (!(r < VINA_CUTOFF)) continue;
            const unsigned tj = type[j];
            const float d = r - (ri + VINA_RADIUS[tj & 15]);
            const float q1 = d * 2.f, q2 = (d - 3.f) * 0.5f;
            const float g1 = expf(-(q1 * q1)), g2 = expf(-(q2 * q2));
            float de = W_GAUSS1 * (-4.f * q1 * g1) + W_GAUSS2 * (-q2 * g2);          // d inter / d d of this pair
            acc[0] += g1;
            acc[1] += g2;
            if (d < 0.f) {
                acc[2] += d * d;
                de += W_REPULSION * (2.f * d);
            }
            if (ti & tj & 16u) {
                if (d <= 0.5f) {
                    acc[3] += 1.f;
                } else if (d < 1.5f) {
                    acc[3] += 1.5f - d;
                    de -= W_HYDROPHOBIC;
                }
            }
            if (((ti & 32u) && (tj & 64u)) || ((ti & 64u) && (tj & 32u))) {
                if (d <= -0.7f) {
                    acc[4] += 1.f;
                } else if (d < 0.f) {
                    acc[4] += -d / 0.7f;
                    de -= W_HBOND / 0.7f;
                }
            }
            if (r > 0.f) {
                const float s = de / r;
                acc[5] = fmaf(s, dx, acc[5]);
                acc[6] = fmaf(s, dy, acc[6]);
                acc[7] = fmaf(s, dz, acc[7]);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float s = wave_sum(acc[e]);
        if ((tid & 63) == 0) red[tid >> 6][e] = s;
    }
    __syncthreads();
    if (tid < 8) {
        const float s = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
        const long long o = (long long)p * L + i;
        if (tid < 5) atom_terms[o * 5 + tid] = s;
        else if (forces) forces[o * 3 + (tid - 5)] = -s;
    }
}

__global__ __launch_bounds__(256) void vina_pose_kernel(const float* __restrict__ atom_terms, float n_rot, float* __restrict__ terms,
                                                       float* __restrict__ inter, float* __restrict__ score,
                                                       float* __restrict__ per_atom, int L) {
    __shared__ float tot[5];
    const int tid = threadIdx.x, p = blockIdx.x;
    const float* at = atom_terms + (long long)p * L * 5;
    for (int i = tid; i < L; i += 256) {
        const float* t = at + i * 5;
        per_atom[(long long)p * L + i] = (((W_GAUSS1 * t[0] + W_GAUSS2 * t[1]) + W_REPULSION * t[2]) + W_HYDROPHOBIC * t[3]) + W_HBOND * t[4];
    }
    if (tid < 5) {
        float s = 0.f;
        for (int i = 0; i < L; ++i) s += at[i * 5 + tid];             // ascending atoms
        tot[tid] = s;
        terms[p * 5 + tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        const float e = (((W_GAUSS1 * tot[0] + W_GAUSS2 * tot[1]) + W_REPULSION * tot[2]) + W_HYDROPHOBIC * tot[3]) + W_HBOND * tot[4];
        inter[p] = e;
        score[p] = e / (1.f + VINA_ROT * n_rot);
    }
}

}  // namespace

PD_EXPORT int pd_vina_score(const float* x, const int* lig_idx, const unsigned char* type, const unsigned char* rec_mask,
                            const unsigned char* lig_active, float n_rot, float* atom_terms, float* terms, float* inter, float* score,
                            float* per_atom, float* forces, int P, int A, int L, void* stream) {
    if (!x || !lig_idx || !type || !rec_mask || !lig_active || !atom_terms || !terms || !inter || !score || !per_atom) return PD_ERR_ARG;
    if (P <= 0 || A <= 0 || L <= 0 || !(n_rot >= 0.f)) return PD_ERR_ARG;
    if ((((uintptr_t)x | (uintptr_t)lig_idx | (uintptr_t)atom_terms | (uintptr_t)terms | (uintptr_t)inter | (uintptr_t)score |
          (uintptr_t)per_atom | (uintptr_t)forces) & 3) != 0)
        return PD_ERR_ARG;
    if (L > VINA_MAX_L || A > VINA_MAX_A || P > 65535) return PD_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(vina_atom_kernel, dim3(L, P), dim3(256), 0, (hipStream_t)stream, x, lig_idx, type, rec_mask, lig_active,
                       atom_terms, forces, A, L);
    hipLaunchKernelGGL(vina_pose_kernel, dim3(P), dim3(256), 0, (hipStream_t)stream, (const float*)atom_terms, n_rot, terms, inter,
                       score, per_atom, L);
    return pd_check_launch();
}
