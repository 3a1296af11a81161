// Ligand burial and interface area of P poses of one ligand in its receptor: how much of the ligand lies inside the protein, and
// which residues form the pocket wall?  Solvent-accessible surface area by point counting (Shrake & Rupley 1973), heavy atoms only.
// (physdock_amd/surface.py builds the tables once per system; the same definition stands in its docstring.)
// Two caveats: the model predicts no hydrogens, so absolute areas are not comparable with all-atom tools; and the default radii and
// probe are this package's defaults and have not been validated on real complexes.
//
// One system, over the A atoms of a pose: cls [A], one byte per atom - 0 ignored (padding, an atom that does not exist, an inactive
// ligand atom), 1 receptor, 2 ligand; radius [A] (A, fp32); probe (A, 1.4 by default); unit [n][3], n unit vectors, the golden
// spiral computed in float64 on the host and rounded to fp32:
//   t = k + 0.5,  z = 1 - 2 t / n,  phi = t pi (3 - sqrt 5),  u_k = (sqrt(1 - z^2) cos phi, sqrt(1 - z^2) sin phi, z),  0 <= k < n.
//
// For pose p and atom i of class c != 0, with R_i = radius_i + probe:
//   the point       p_ik = x_i + R_i u_k                        (per coordinate fmaf(R_i, u, x_i))
//   atom j covers it iff j != i (by INDEX, not by distance), cls_j != 0 and |p_ik - x_j| < R_j, evaluated as
//                   fmaf(dz, dz, fmaf(dy, dy, dx * dx)) < R_j * R_j   with d = p_ik - x_j
//   same_k          any covering j has class c;        other_k   any covering j has the other class
//   n_free[i]   = #{k : !same_k}                        the exposure within the atom's own molecule
//   n_bound[i]  = #{k : !same_k && !other_k}            the exposure in the complex
//   n_buried[i] = n_free[i] - n_bound[i]
//   area(m, i)  = (float)m * ((12.566370614359172f * (R_i * R_i)) / (float)n)       m points of atom i, in A^2
//
//   free_points[p][s]      n_free of ligand atom lig_idx[s]; 0 for an inactive one
//   buried_points[p][a]    n_buried of every atom; 0 for an ignored atom and for a receptor atom no ligand atom can reach
//   per_atom[p][s]         area(n_buried, lig_idx[s])
//   totals[t][p]           t = 0 ligand_free  = sum over s of area(n_free),   1 ligand_bound = sum of area(n_bound),
//                          2 ligand_buried = sum of area(n_buried),           3 buried_fraction = buried / free (0 where free == 0),
//                          4 buried_polar / 5 buried_apolar: ligand_buried split by polar[s] != 0,
//                          6 receptor_buried = sum over the receptor atoms of area(n_buried),
//                          7 interface_area = (ligand_buried + receptor_buried) / 2
//   residue_buried[p][r]   sum of area(n_buried) over the receptor atoms of residue r (res_atom[res_start[r] .. res_start[r + 1]))
//   interface_residues[p]  the number of residues with residue_buried > 0
//
// sasa_point_kernel: one block of 256 threads per (atom, pose).  An ignored atom stores 0 and leaves.  A receptor atom first looks
// at the L ligand atoms only: if none lies within R_i + R_j + slack of it no ligand atom can cover a point, n_buried is 0 and the
// block leaves (the exit is uniform over the block; in a 2048-atom pocket it ends most of the blocks).  Otherwise the block
// scans the pose in runs of 256 atoms and collects those within reach, (R_i + R_j) (1 + 2^-13) + 0.01 A of x_i - a superset of the
// atoms that can cover a point for coordinates up to 10^4 A, never a subset - into an LDS list (x, y, z, R_j^2, 1 = same class /
// 2 = other) by wave ballot and popcount.  The list buffer holds 2 LIST entries; whenever it holds LIST or more it is walked and
// emptied, so no input is truncated: a point's two flags stay in registers from walk to walk.  Walk: the block is split into G
// groups of 256 / G threads (G = 4 for n <= 64, 2 for n <= 128, else 1); thread t of group g owns the points k = t, t + 256 / G,
// ... (at most four) and tests them against the entries e = g, g + G, ... with broadcast LDS reads; for G > 1 the groups' flags are
// ORed through LDS at the end.  The counts are integer sums (wave butterfly, then the four waves).  "Any" and integer sums do not
// depend on their order.
// sasa_pose_kernel: one block per pose.  Areas from the counts; the ligand's five sums in ascending ligand order (one thread
// each); the receptor total in ascending atom order (one wave: 64 atoms at a time, the non-zero terms added lane by lane - adding
// +0 to a non-negative sum changes nothing, so zero terms are skipped); a residue's sum in the ascending order of its run.  No
// atomics, no allocation; every value depends on its own pose alone and on no launch dimension: results are bit-identical from run
// to run, whatever P is and wherever a pose sits.
#include "common.h"
#include "physdock_hip.h"

namespace {

constexpr int SASA_MAX_L = 1024;
constexpr int SASA_MAX_A = 1 << 22;
constexpr int SASA_MAX_P = 65535;
constexpr int LIST = PD_SASA_LIST;                // the list is walked whenever it holds this many entries; a run adds at most 256
constexpr int POINTS_PER_THREAD = PD_SASA_MAX_POINTS / 256;
constexpr float FOUR_PI = 12.566370614359172f;
constexpr float REACH_REL = 1.0001220703125f;     // 1 + 2^-13
constexpr float REACH_ABS = 0.01f;
static_assert(LIST == 256 && PD_SASA_MAX_POINTS == 1024 && PD_SASA_TOTALS == 8, "the numbers the header documents");

__device__ __forceinline__ float sasa_dist2(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}
__device__ __forceinline__ float sasa_reach2(float Ri, float Rj) {
    const float r = fmaf(Ri + Rj, REACH_REL, REACH_ABS);
    return r * r;
}
// area of m points of an atom with R = radius + probe
__device__ __forceinline__ float sasa_area(int m, float R, float n) { return (float)m * ((FOUR_PI * (R * R)) / n); }

__global__ __launch_bounds__(256) void sasa_point_kernel(const float* __restrict__ x, const unsigned char* __restrict__ cls,
                                                        const float* __restrict__ radius, const float* __restrict__ unit,
                                                        const int* __restrict__ lig_idx, float probe, int* __restrict__ ws_free,
                                                        int* __restrict__ buried_points, int A, int L, int n) {
    __shared__ float ex[2 * LIST], ey[2 * LIST], ez[2 * LIST], er2[2 * LIST];
    __shared__ int ef[2 * LIST];
    __shared__ int wcnt[2][4];
    __shared__ int gflag[256];
    __shared__ int red[4][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = blockIdx.x, p = blockIdx.y;
    const float* xp = x + (long long)p * A * 3;
    const long long out = (long long)p * A + i;
    const int c = cls[i];
    if (c == 0) {                                                    // uniform over the block
        if (tid == 0) {
            ws_free[out] = 0;
            buried_points[out] = 0;
        }
        return;
    }
    const float ax = xp[3 * i], ay = xp[3 * i + 1], az = xp[3 * i + 2];
    const float Ri = radius[i] + probe;
    if (c == 1) {                                                    // a receptor atom: can any ligand atom cover a point of it?
        int near = 0;
        for (int s = tid; s < L; s += 256) {
            const int a = lig_idx[s];
            if (cls[a] != 2) continue;
            near |= sasa_dist2(ax, ay, az, xp[3 * a], xp[3 * a + 1], xp[3 * a + 2]) < sasa_reach2(Ri, radius[a] + probe) ? 1 : 0;
        }
        if (!__syncthreads_or(near)) {                               // uniform over the block
            if (tid == 0) {
                ws_free[out] = 0;
                buried_points[out] = 0;
            }
            return;
        }
    }
    // the points this thread owns, and their flags (bit 0 same, bit 1 other)
    const int G = n <= 64 ? 4 : (n <= 128 ? 2 : 1), T = 256 / G, g = tid / T, t = tid - g * T;
    float px[POINTS_PER_THREAD], py[POINTS_PER_THREAD], pz[POINTS_PER_THREAD];
    int flag[POINTS_PER_THREAD];
#pragma unroll
    for (int m = 0; m < POINTS_PER_THREAD; ++m) {
        const int k = t + m * T;
        const bool has = k < n && (G == 1 || m == 0);
        const int kk = has ? k : 0;
        px[m] = fmaf(Ri, unit[3 * kk], ax);
        py[m] = fmaf(Ri, unit[3 * kk + 1], ay);
        pz[m] = fmaf(Ri, unit[3 * kk + 2], az);
        flag[m] = 0;
    }
    int count = 0;                                                   // entries in the list: uniform over the block
    const int M = (n + T - 1) / T;                                   // points per thread: uniform
    for (int j0 = 0, run = 0; j0 < A; j0 += 256, ++run) {
        const int j = j0 + tid;
        int cj = 0;
        float bx = 0.f, by = 0.f, bz = 0.f, Rj = 0.f;
        if (j < A && j != i) cj = cls[j];
        if (cj != 0) {
            bx = xp[3 * j], by = xp[3 * j + 1], bz = xp[3 * j + 2];
            Rj = radius[j] + probe;
            if (!(sasa_dist2(ax, ay, az, bx, by, bz) < sasa_reach2(Ri, Rj))) cj = 0;
        }
        const unsigned long long mask = __ballot(cj != 0);
        if (lane == 0) wcnt[run & 1][wave] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int v = wcnt[run & 1][w];
            before += w < wave ? v : 0;
            total += v;
        }
        if (cj != 0) {
            const int e = count + before + __popcll(mask & ((1ull << lane) - 1ull));            // count < LIST: e < 2 LIST
            ex[e] = bx, ey[e] = by, ez[e] = bz, er2[e] = Rj * Rj;
            ef[e] = cj == c ? 1 : 2;
        }
        count += total;
        if (count < LIST && j0 + 256 < A) continue;                  // room for another run, and there is one: uniform
        __syncthreads();                                             // the list is complete
        for (int e = g; e < count; e += G) {
            const float qx = ex[e], qy = ey[e], qz = ez[e], r2 = er2[e];
            const int f = ef[e];
#pragma unroll
            for (int m = 0; m < POINTS_PER_THREAD; ++m)
                if (m < M) flag[m] |= sasa_dist2(px[m], py[m], pz[m], qx, qy, qz) < r2 ? f : 0;
        }
        count = 0;
        __syncthreads();                                             // the list may be written again
    }
    if (G > 1) {                                                     // uniform: OR the groups' flags of a point
        gflag[tid] = flag[0];
        __syncthreads();
        int f = 0;
        for (int q = 0; q < G; ++q) f |= gflag[q * T + t];
        flag[0] = f;
    }
    int n_free = 0, n_bound = 0;
#pragma unroll
    for (int m = 0; m < POINTS_PER_THREAD; ++m) {
        const bool has = t + m * T < n && g == 0 && (G == 1 || m == 0);
        n_free += has && !(flag[m] & 1) ? 1 : 0;
        n_bound += has && flag[m] == 0 ? 1 : 0;
    }
    n_free = wave_sum(n_free);
    n_bound = wave_sum(n_bound);
    if (lane == 0) red[wave][0] = n_free, red[wave][1] = n_bound;
    __syncthreads();
    if (tid == 0) {
        const int fr = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
        const int bo = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
        ws_free[out] = fr;
        buried_points[out] = fr - bo;
    }
}

__global__ __launch_bounds__(256) void sasa_pose_kernel(const unsigned char* __restrict__ cls, const float* __restrict__ radius,
                                                       const int* __restrict__ lig_idx, const unsigned char* __restrict__ polar,
                                                       const int* __restrict__ res_start, const int* __restrict__ res_atom,
                                                       float probe, const int* __restrict__ ws_free,
                                                       const int* __restrict__ buried_points, int* __restrict__ free_points,
                                                       float* __restrict__ per_atom, float* __restrict__ totals,
                                                       float* __restrict__ residue_buried, int* __restrict__ interface_residues,
                                                       int P, int A, int L, int R, int n) {
    __shared__ float tot[6];                                         // free, bound, buried, polar, apolar, receptor
    __shared__ int red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = blockIdx.x;
    const int* fr = ws_free + (long long)p * A;
    const int* bu = buried_points + (long long)p * A;
    const float fn = (float)n;
    for (int s = tid; s < L; s += 256) {
        const int a = lig_idx[s];
        free_points[(long long)p * L + s] = fr[a];
        per_atom[(long long)p * L + s] = sasa_area(bu[a], radius[a] + probe, fn);
    }
    int n_res = 0;
    for (int r = tid; r < R; r += 256) {
        float sum = 0.f;
        for (int q = res_start[r], e = res_start[r + 1]; q < e; ++q) {              // ascending atoms of the residue
            const int a = res_atom[q];
            sum += sasa_area(bu[a], radius[a] + probe, fn);
        }
        residue_buried[(long long)p * R + r] = sum;
        n_res += sum > 0.f ? 1 : 0;
    }
    n_res = wave_sum(n_res);
    if (lane == 0) red[wave] = n_res;
    if (wave == 0) {                                                 // the receptor total, ascending atoms, 64 at a time
        float sum = 0.f;
        for (int a0 = 0; a0 < A; a0 += 64) {
            const int a = a0 + lane;
            float term = 0.f;
            if (a < A && cls[a] == 1) {
                const int m = bu[a];
                if (m != 0) term = sasa_area(m, radius[a] + probe, fn);
            }
            unsigned long long mask = __ballot(term != 0.f);
            while (mask) {                                           // uniform over the wave
                const int src = __ffsll((long long)mask) - 1;
                sum += __shfl(term, src);
                mask &= mask - 1ull;
            }
        }
        if (lane == 0) tot[5] = sum;
    } else if (wave == 1 && lane < 5) {                              // the ligand's sums, ascending ligand atoms
        float sum = 0.f;
        for (int s = 0; s < L; ++s) {
            const int a = lig_idx[s];
            const int f = fr[a], b = bu[a];
            const bool pol = polar[s] != 0;
            const int m = lane == 0 ? f : (lane == 1 ? f - b : (lane == 2 ? b : (lane == 3 ? (pol ? b : 0) : (pol ? 0 : b))));
            sum += sasa_area(m, radius[a] + probe, fn);
        }
        tot[lane] = sum;
    }
    __syncthreads();
    if (tid == 0) {
        interface_residues[p] = ((red[0] + red[1]) + red[2]) + red[3];
        totals[0 * (long long)P + p] = tot[0];
        totals[1 * (long long)P + p] = tot[1];
        totals[2 * (long long)P + p] = tot[2];
        totals[3 * (long long)P + p] = tot[0] > 0.f ? tot[2] / tot[0] : 0.f;
        totals[4 * (long long)P + p] = tot[3];
        totals[5 * (long long)P + p] = tot[4];
        totals[6 * (long long)P + p] = tot[5];
        totals[7 * (long long)P + p] = (tot[2] + tot[5]) * 0.5f;
    }
}

}  // namespace

PD_EXPORT int pd_buried_surface(const float* x, const unsigned char* cls, const float* radius, const float* unit, const int* lig_idx,
                                const unsigned char* polar, const int* res_start, const int* res_atom, float probe, int* ws_free,
                                int* free_points, int* buried_points, float* per_atom, float* totals, float* residue_buried,
                                int* interface_residues, int P, int A, int L, int R, int N, int n_points, void* stream) {
    if (!x || !cls || !radius || !unit || !lig_idx || !polar || !res_start || !ws_free || !free_points || !buried_points || !per_atom ||
        !totals || !residue_buried || !interface_residues)
        return PD_ERR_ARG;
    if (P <= 0 || A <= 0 || L <= 0 || R <= 0 || N < 0 || N > A || n_points <= 0) return PD_ERR_ARG;
    if (N > 0 && !res_atom) return PD_ERR_ARG;
    if (!(probe >= 0.f) || !(probe <= 3.0e38f)) return PD_ERR_ARG;                                // negative, NaN or infinite
    if ((((uintptr_t)x | (uintptr_t)radius | (uintptr_t)unit | (uintptr_t)lig_idx | (uintptr_t)res_start | (uintptr_t)res_atom |
          (uintptr_t)ws_free | (uintptr_t)free_points | (uintptr_t)buried_points | (uintptr_t)per_atom | (uintptr_t)totals |
          (uintptr_t)residue_buried | (uintptr_t)interface_residues) & 3) != 0)
        return PD_ERR_ARG;
    if (n_points > PD_SASA_MAX_POINTS || L > SASA_MAX_L || A > SASA_MAX_A || P > SASA_MAX_P || R > A) return PD_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sasa_point_kernel, dim3(A, P), dim3(256), 0, s, x, cls, radius, unit, lig_idx, probe, ws_free, buried_points, A, L,
                       n_points);
    hipLaunchKernelGGL(sasa_pose_kernel, dim3(P), dim3(256), 0, s, cls, radius, lig_idx, polar, res_start, res_atom, probe,
                       (const int*)ws_free, (const int*)buried_points, free_points, per_atom, totals, residue_buried, interface_residues,
                       P, A, L, R, n_points);
    return pd_check_launch();
}
