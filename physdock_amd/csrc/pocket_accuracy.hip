// PocketAccuracy: did the model draw the right POCKET?  The lDDT of the ligand pocket (lDDT-LP) and the pocket RMSDs of P poses of one
// system against one ground truth (physdock_amd/pocket_accuracy.py builds the tables once per system; tests/pocket_accuracy_ref.py is
// the written definition).  With the pocket atoms i (the receptor atoms of the residues near the ligand in the ground truth), their
// pairs N(i) (receptor atoms of another residue within the inclusion radius there) and d_ref(i,j), all distances in float64 from the
// fp32 coordinates:
//
//   conserved_t(i,j) = | |p_i - p_j| - d_ref(i,j) | < thr[t]                           (t = 0 .. 3)
//   step 1           per pocket residue r with interchangeable atom names (ASP OD1/OD2, ...): A_r = the conserved (pair, threshold)
//                    entries of the rows of r's atoms as given, B_r the same with r's swap pairs exchanged in the pose and every other
//                    residue as given; r is swapped iff B_r > A_r
//   step 2           all counts again with every chosen swap applied at once, on the i side and the j side:
//                    lddt_lp = sum_t C_t / (4 n_pairs), residue_lddt the same per pocket residue (0 without pairs)
//   fit              Horn's quaternion of the pose's pocket CA atoms on the reference's (proper rotations only, horn_lambda_max of
//                    geom3.h): ref ~ R(quat) pose + t; ca / backbone / heavy / per-residue RMSD under that ONE transform, swaps applied
//
// Three kernels, no atomics, nothing read back.  pocket_counts_kernel<STEP>: one block of 256 threads per (pocket residue, pose).  The
// block walks the rows of the residue's atoms one after the other, each row in tiles of 256 pairs (a row of any length), a thread
// keeps integer counts in registers and the block reduces them once at its end.  STEP 1 counts both namings of the residue and stores
// the decision, STEP 2 reads the decisions of the pose and stores the residue's four counts in the workspace.  pocket_fit_kernel: one
// block per pose; the finite check over the atoms the tables name, the integer totals, then the float64 sums of the fit (every thread
// adds its residues' atoms in ascending order, then the fixed tree of block_sum_d), the 4x4 eigen-solve (every thread the same) and
// the deviations.  A value depends on its own pose and the tables alone: bit-identical from launch to launch and whatever the batch.
#include "common.h"
#include "geom3.h"
#include "physdock_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int PA_MAX_ATOMS = PD_POCKET_ACCURACY_MAX_ATOMS;
constexpr int PA_MAX_RESIDUES = PD_POCKET_ACCURACY_MAX_RESIDUES;
constexpr int PA_MAX_POSES = 65535;        // blockIdx.y
constexpr int PA_TILE = 256;               // pairs of a row taken at a time: one per thread
constexpr double PA_FLAT = 1e-8;           // a CA set whose middle scatter eigenvalue is at most this share of the largest is a line
static_assert(PA_TILE == PD_POCKET_ACCURACY_TILE, "the constant the header documents");

struct pa_thresholds { double t[4]; };
enum { PA_CA = 1, PA_BACKBONE = 2 };

__device__ __forceinline__ double pa_dist(Vec3 a, Vec3 b) {
    const Vec3 d = sub(a, b);
    return sqrt(fma(d.z, d.z, fma(d.y, d.y, d.x * d.x)));
}

// sum of one int per thread of a 256-thread block, returned to every thread (red holds 4 ints)
__device__ __forceinline__ int pa_block_sum_i(int v, int* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

template <int STEP>
__global__ __launch_bounds__(256) void pocket_counts_kernel(const float* __restrict__ x, const int* __restrict__ patom,
                                                           const int* __restrict__ patom_partner, const int* __restrict__ res_atom_start,
                                                           const int* __restrict__ pair_start, const int* __restrict__ pair_atom,
                                                           const double* __restrict__ pair_dist, const int* __restrict__ atom_partner,
                                                           const int* __restrict__ atom_slot, const pa_thresholds thr,
                                                           int* __restrict__ swapped, int* __restrict__ res_counts, int A, int Rp) {
    __shared__ int red[4];
    const int tid = threadIdx.x, r = blockIdx.x, p = blockIdx.y;
    const float* xp = x + (long long)p * A * 3;
    const int* sw = swapped + (long long)p * Rp;
    const int s0 = res_atom_start[r], s1 = res_atom_start[r + 1];
    bool swappable = false;
    for (int s = s0; s < s1; ++s) swappable |= patom_partner[s] != patom[s];
    if (STEP == 1 && !swappable) {
        if (tid == 0) swapped[(long long)p * Rp + r] = 0;
        return;
    }
    const bool own = STEP == 2 && sw[r] != 0;
    int c[4] = {0, 0, 0, 0};           // STEP 1: c[0] = as given, c[1] = exchanged, both summed over the thresholds
    for (int s = s0; s < s1; ++s) {
        const int i = patom[s], ip = patom_partner[s];
        const Vec3 pi = load3(xp + 3 * (own ? ip : i));
        const Vec3 qi = load3(xp + 3 * ip);                              // STEP 1: the atom under the other naming
        const int e1 = pair_start[s + 1];
        for (int e = pair_start[s] + tid; e < e1; e += PA_TILE) {
            int j = pair_atom[e];
            const double dref = pair_dist[e];
            if (STEP == 2) {
                const int slot = atom_slot[j];
                if (slot >= 0 && sw[slot] != 0) j = atom_partner[j];
            }
            const Vec3 pj = load3(xp + 3 * j);
            const double diff = fabs(pa_dist(pi, pj) - dref);
            if (STEP == 2) {
#pragma unroll
                for (int t = 0; t < 4; ++t) c[t] += diff < thr.t[t] ? 1 : 0;
            } else {
                const double other = ip == i ? diff : fabs(pa_dist(qi, pj) - dref);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    c[0] += diff < thr.t[t] ? 1 : 0;
                    c[1] += other < thr.t[t] ? 1 : 0;
                }
            }
        }
    }
    if (STEP == 1) {
        const int given = pa_block_sum_i(c[0], red), other = pa_block_sum_i(c[1], red);
        if (tid == 0) swapped[(long long)p * Rp + r] = other > given ? 1 : 0;
    } else {
        int* out = res_counts + ((long long)p * Rp + r) * 4;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int v = pa_block_sum_i(c[t], red);
            if (tid == 0) out[t] = v;
        }
    }
}

__global__ __launch_bounds__(256) void pocket_fit_kernel(const float* __restrict__ x, const int* __restrict__ patom,
                                                        const int* __restrict__ patom_partner, const unsigned char* __restrict__ patom_kind,
                                                        const double* __restrict__ patom_ref, const int* __restrict__ res_atom_start,
                                                        const int* __restrict__ pair_start, const int* __restrict__ named,
                                                        const int* __restrict__ res_counts, float* __restrict__ lddt_lp,
                                                        float* __restrict__ residue_lddt, int* __restrict__ conserved,
                                                        int* __restrict__ swapped, float* __restrict__ rmsd, float* __restrict__ residue_rmsd,
                                                        double* __restrict__ quat, double* __restrict__ trans, unsigned char* __restrict__ ok,
                                                        unsigned char* __restrict__ fit_ok, int A, int Np, int Rp, int n_named) {
    __shared__ int redi[4];
    __shared__ double redd[4];
    const int tid = threadIdx.x, p = blockIdx.x;
    const float* xp = x + (long long)p * A * 3;
    int* sw = swapped + (long long)p * Rp;
    const int* cnt = res_counts + (long long)p * Rp * 4;
    const float nanf_ = __int_as_float(0x7fc00000);
    const double nand = __longlong_as_double(0x7ff8000000000000ll);
    int bad = 0;
    for (int k = tid; k < n_named; k += 256) {
        const int a = named[k];
        if (!finite3(xp[3 * a], xp[3 * a + 1], xp[3 * a + 2])) bad = 1;
    }
    bad = __syncthreads_or(bad);
    if (bad) {
        for (int r = tid; r < Rp; r += 256) {
            sw[r] = 0;
            residue_lddt[(long long)p * Rp + r] = nanf_;
            residue_rmsd[(long long)p * Rp + r] = nanf_;
        }
        if (tid < 4) { conserved[p * 4 + tid] = 0; quat[p * 4 + tid] = nand; }
        if (tid < 3) { rmsd[p * 3 + tid] = nanf_; trans[p * 3 + tid] = nand; }
        if (tid == 0) { lddt_lp[p] = nanf_; ok[p] = 0; fit_ok[p] = 0; }
        return;
    }
    // the integer totals
    int c4[4] = {0, 0, 0, 0};
    for (int r = tid; r < Rp; r += 256) {
        const int4 v = *reinterpret_cast<const int4*>(cnt + 4 * r);
        const int n_r = pair_start[res_atom_start[r + 1]] - pair_start[res_atom_start[r]];
        c4[0] += v.x; c4[1] += v.y; c4[2] += v.z; c4[3] += v.w;
        const long long tot = (long long)v.x + v.y + v.z + v.w;
        residue_lddt[(long long)p * Rp + r] = n_r ? (float)((double)tot / (4.0 * (double)n_r)) : 0.f;
    }
    long long total = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        c4[t] = pa_block_sum_i(c4[t], redi);
        total += c4[t];
    }
    if (tid < 4) conserved[p * 4 + tid] = tid == 0 ? c4[0] : (tid == 1 ? c4[1] : (tid == 2 ? c4[2] : c4[3]));
    if (tid == 0) {
        const int n = pair_start[Np];
        lddt_lp[p] = n ? (float)((double)total / (4.0 * (double)n)) : 0.f;
        ok[p] = 1;
    }
    // the fit: centroids of the CA atoms
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int n_ca = 0, n_bb = 0;
    for (int r = tid; r < Rp; r += 256) {
        const bool swp = sw[r] != 0;
        for (int k = res_atom_start[r]; k < res_atom_start[r + 1]; ++k) {
            const int kind = patom_kind[k];
            n_bb += (kind & PA_BACKBONE) ? 1 : 0;
            if (!(kind & PA_CA)) continue;
            const Vec3 a = load3(xp + 3 * (swp ? patom_partner[k] : patom[k])), b = load3(patom_ref + 3 * k);
            s[0] += a.x; s[1] += a.y; s[2] += a.z; s[3] += b.x; s[4] += b.y; s[5] += b.z;
            ++n_ca;
        }
    }
    n_ca = pa_block_sum_i(n_ca, redi);
    n_bb = pa_block_sum_i(n_bb, redi);
#pragma unroll
    for (int e = 0; e < 6; ++e) s[e] = block_sum_d(s[e], redd);
    bool fit = n_ca >= 3;
    const double inv = 1.0 / (double)(n_ca > 0 ? n_ca : 1);
    const Vec3 ca = {s[0] * inv, s[1] * inv, s[2] * inv}, cb = {s[3] * inv, s[4] * inv, s[5] * inv};
    // covariance S[3 x + y] = sum a_x b_y and the two scatter matrices (xx, yy, zz, xy, xz, yz) of the centred CA sets
    double S[9], Ma[6], Mb[6];
#pragma unroll
    for (int e = 0; e < 9; ++e) S[e] = 0.0;
#pragma unroll
    for (int e = 0; e < 6; ++e) Ma[e] = Mb[e] = 0.0;
    for (int r = tid; r < Rp; r += 256) {
        const bool swp = sw[r] != 0;
        for (int k = res_atom_start[r]; k < res_atom_start[r + 1]; ++k) {
            if (!(patom_kind[k] & PA_CA)) continue;
            const Vec3 a = sub(load3(xp + 3 * (swp ? patom_partner[k] : patom[k])), ca), b = sub(load3(patom_ref + 3 * k), cb);
            S[0] = fma(a.x, b.x, S[0]); S[1] = fma(a.x, b.y, S[1]); S[2] = fma(a.x, b.z, S[2]);
            S[3] = fma(a.y, b.x, S[3]); S[4] = fma(a.y, b.y, S[4]); S[5] = fma(a.y, b.z, S[5]);
            S[6] = fma(a.z, b.x, S[6]); S[7] = fma(a.z, b.y, S[7]); S[8] = fma(a.z, b.z, S[8]);
            Ma[0] = fma(a.x, a.x, Ma[0]); Ma[1] = fma(a.y, a.y, Ma[1]); Ma[2] = fma(a.z, a.z, Ma[2]);
            Ma[3] = fma(a.x, a.y, Ma[3]); Ma[4] = fma(a.x, a.z, Ma[4]); Ma[5] = fma(a.y, a.z, Ma[5]);
            Mb[0] = fma(b.x, b.x, Mb[0]); Mb[1] = fma(b.y, b.y, Mb[1]); Mb[2] = fma(b.z, b.z, Mb[2]);
            Mb[3] = fma(b.x, b.y, Mb[3]); Mb[4] = fma(b.x, b.z, Mb[4]); Mb[5] = fma(b.y, b.z, Mb[5]);
        }
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) S[e] = block_sum_d(S[e], redd);
#pragma unroll
    for (int e = 0; e < 6; ++e) { Ma[e] = block_sum_d(Ma[e], redd); Mb[e] = block_sum_d(Mb[e], redd); }
    // a point or a line has no unique superposition: the middle eigenvalue of the scatter matrix (cyclic Jacobi, as validity.hip)
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const double* M = side ? Mb : Ma;
        double a00 = M[0], a11 = M[1], a22 = M[2], a01 = M[3], a02 = M[4], a12 = M[5];
#pragma unroll 1
        for (int sweep = 0; sweep < 10; ++sweep) {
            jacobi(a00, a11, a01, a02, a12);
            jacobi(a00, a22, a02, a01, a12);
            jacobi(a11, a22, a12, a01, a02);
        }
        const double lo = fmin(a00, fmin(a11, a22)), hi = fmax(a00, fmax(a11, a22)), mid = a00 + a11 + a22 - lo - hi;
        if (!(mid > PA_FLAT * hi)) fit = false;
    }
    if (!fit) {
        for (int r = tid; r < Rp; r += 256) residue_rmsd[(long long)p * Rp + r] = nanf_;
        if (tid < 4) quat[p * 4 + tid] = nand;
        if (tid < 3) { rmsd[p * 3 + tid] = nanf_; trans[p * 3 + tid] = nand; }
        if (tid == 0) fit_ok[p] = 0;
        return;
    }
    double q[4];
    horn_lambda_max<true>(S, q);
    const double w = q[0], qx = q[1], qy = q[2], qz = q[3];
    const double R00 = 1.0 - 2.0 * (qy * qy + qz * qz), R01 = 2.0 * (qx * qy - w * qz), R02 = 2.0 * (qx * qz + w * qy);
    const double R10 = 2.0 * (qx * qy + w * qz), R11 = 1.0 - 2.0 * (qx * qx + qz * qz), R12 = 2.0 * (qy * qz - w * qx);
    const double R20 = 2.0 * (qx * qz - w * qy), R21 = 2.0 * (qy * qz + w * qx), R22 = 1.0 - 2.0 * (qx * qx + qy * qy);
    const Vec3 t = {cb.x - (R00 * ca.x + R01 * ca.y + R02 * ca.z), cb.y - (R10 * ca.x + R11 * ca.y + R12 * ca.z),
                    cb.z - (R20 * ca.x + R21 * ca.y + R22 * ca.z)};
    double d_ca = 0.0, d_bb = 0.0, d_all = 0.0;
    for (int r = tid; r < Rp; r += 256) {
        const bool swp = sw[r] != 0;
        const int k0 = res_atom_start[r], k1 = res_atom_start[r + 1];
        double d_res = 0.0;
        for (int k = k0; k < k1; ++k) {
            const int kind = patom_kind[k];
            const Vec3 a = load3(xp + 3 * (swp ? patom_partner[k] : patom[k])), b = load3(patom_ref + 3 * k);
            const double ex = (R00 * a.x + R01 * a.y + R02 * a.z) + t.x - b.x, ey = (R10 * a.x + R11 * a.y + R12 * a.z) + t.y - b.y,
                         ez = (R20 * a.x + R21 * a.y + R22 * a.z) + t.z - b.z;
            const double d2 = fma(ez, ez, fma(ey, ey, ex * ex));
            d_res += d2;
            if (kind & PA_CA) d_ca += d2;
            if (kind & PA_BACKBONE) d_bb += d2;
        }
        d_all += d_res;
        residue_rmsd[(long long)p * Rp + r] = k1 > k0 ? (float)sqrt(d_res / (double)(k1 - k0)) : nanf_;
    }
    d_ca = block_sum_d(d_ca, redd);
    d_bb = block_sum_d(d_bb, redd);
    d_all = block_sum_d(d_all, redd);
    if (tid == 0) {
        rmsd[p * 3] = (float)sqrt(d_ca / (double)n_ca);
        rmsd[p * 3 + 1] = n_bb ? (float)sqrt(d_bb / (double)n_bb) : nanf_;
        rmsd[p * 3 + 2] = (float)sqrt(d_all / (double)Np);
        quat[p * 4] = w; quat[p * 4 + 1] = qx; quat[p * 4 + 2] = qy; quat[p * 4 + 3] = qz;
        trans[p * 3] = t.x; trans[p * 3 + 1] = t.y; trans[p * 3 + 2] = t.z;
        fit_ok[p] = 1;
    }
}

}  // namespace

PD_EXPORT int pd_pocket_accuracy_workspace_numel(int P, int Rp) {
    if (P < 1 || Rp < 1) return PD_ERR_ARG;
    if (P > PA_MAX_POSES || Rp > PA_MAX_RESIDUES) return PD_ERR_UNSUPPORTED;
    return P * Rp * 4;                     // at most 65535 * 1024 * 4 < 2^31
}

PD_EXPORT int pd_pocket_accuracy(const float* x, const int* patom, const int* patom_partner, const unsigned char* patom_kind,
                                 const double* patom_ref, const int* res_atom_start, const int* pair_start, const int* pair_atom,
                                 const double* pair_dist, const int* atom_partner, const int* atom_slot, const int* named, double thr0,
                                 double thr1, double thr2, double thr3, int* ws, long long ws_numel, float* lddt_lp, float* residue_lddt,
                                 int* conserved, int* swapped, float* rmsd, float* residue_rmsd, double* quat, double* t, unsigned char* ok,
                                 unsigned char* fit_ok, int P, int A, int Np, int Rp, int n_pairs, int n_named, void* stream) {
    if (!x || !patom || !patom_partner || !patom_kind || !patom_ref || !res_atom_start || !pair_start || !atom_partner || !atom_slot ||
        !named || !ws || !lddt_lp || !residue_lddt || !conserved || !swapped || !rmsd || !residue_rmsd || !quat || !t || !ok || !fit_ok)
        return PD_ERR_ARG;
    if (P < 1 || A < 1 || Np < 1 || Rp < 1 || Rp > Np || n_pairs < 0 || n_named < Np) return PD_ERR_ARG;
    if (A <= PA_MAX_ATOMS && (Np > A || n_named > A)) return PD_ERR_ARG;
    if (n_pairs && (!pair_atom || !pair_dist)) return PD_ERR_ARG;
    if (!(thr0 > 0.0) || !(thr1 > 0.0) || !(thr2 > 0.0) || !(thr3 > 0.0)) return PD_ERR_ARG;
    if (pd_misaligned(x, 4) || pd_misaligned(patom, 4) || pd_misaligned(patom_partner, 4) || pd_misaligned(patom_ref, 8) ||
        pd_misaligned(res_atom_start, 4) || pd_misaligned(pair_start, 4) || pd_misaligned(pair_atom, 4) || pd_misaligned(pair_dist, 8) ||
        pd_misaligned(atom_partner, 4) || pd_misaligned(atom_slot, 4) || pd_misaligned(named, 4) || pd_misaligned(ws, 16) ||
        pd_misaligned(lddt_lp, 4) || pd_misaligned(residue_lddt, 4) || pd_misaligned(conserved, 4) || pd_misaligned(swapped, 4) ||
        pd_misaligned(rmsd, 4) || pd_misaligned(residue_rmsd, 4) || pd_misaligned(quat, 8) || pd_misaligned(t, 8))
        return PD_ERR_ARG;
    if (A > PA_MAX_ATOMS || Rp > PA_MAX_RESIDUES || P > PA_MAX_POSES) return PD_ERR_UNSUPPORTED;
    if (ws_numel < (long long)P * Rp * 4) return PD_ERR_ARG;
    const pa_thresholds thr = {{thr0, thr1, thr2, thr3}};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pocket_counts_kernel<1>, dim3(Rp, P), dim3(256), 0, s, x, patom, patom_partner, res_atom_start, pair_start, pair_atom,
                       pair_dist, atom_partner, atom_slot, thr, swapped, ws, A, Rp);
    hipLaunchKernelGGL(pocket_counts_kernel<2>, dim3(Rp, P), dim3(256), 0, s, x, patom, patom_partner, res_atom_start, pair_start, pair_atom,
                       pair_dist, atom_partner, atom_slot, thr, swapped, ws, A, Rp);
    hipLaunchKernelGGL(pocket_fit_kernel, dim3(P), dim3(256), 0, s, x, patom, patom_partner, patom_kind, patom_ref, res_atom_start, pair_start,
                       named, (const int*)ws, lddt_lp, residue_lddt, conserved, swapped, rmsd, residue_rmsd, quat, t, ok, fit_ok, A, Np, Rp,
                       n_named);
    return pd_check_launch();
}
