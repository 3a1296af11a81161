// PoseBusters-style geometry checks of P poses of one ligand in its receptor (physdock_amd/validity.py builds the tables once per
// ligand).  With x_a the position of ligand atom a (pose atom lig_idx[a]), r its van der Waals radius and d(a,b) = |x_a - x_b|:
//
//   val[p][0], [1] = min, max over bonded pairs (a,b) of       d(a,b) / d12_ref
//   val[p][2], [3] = min, max over 1-3 pairs (a,b) of          d(a,b) / d13_ref            (a 1-3 distance pins the bond angle)
//   val[p][4]      = min over a < b, far[a][b], both active of d(a,b) / (r_a + r_b)
//   val[p][5]      = min over active a, receptor atoms j of    d(a,j) / (r_a + r_j)        worst[p] = the (a, j) that attains it
//   val[p][6]      = min over the same pairs of                d(a,j)                      (Angstrom: the "floated away" signal)
//   val[p][7]      = max over planar groups g and their atoms a of |n_g . (x_a - c_g)|     (Angstrom)
//
// c_g is the centroid of group g and n_g the unit eigenvector of the smallest eigenvalue of its covariance matrix
// C = (1/n) sum (x_a - c_g)(x_a - c_g)^T: the normal of the least-squares plane.  A group whose second eigenvalue is at most
// 1e-10 of its largest (collinear or coincident atoms: no plane is defined) reports 0.  Empty sets report 1 (columns 0 - 3),
// +inf (4 - 6), 0 (7) and worst = (-1, -1).  flags[p] is the bit mask of the thresholds applied to the stored val[p] (bit order
// of pd_validity_thresholds); an empty set sets no bit (column 6 flags only a finite distance).
//
// Two kernels, no atomics, no scratch memory.  validity_receptor_kernel: one block per (tile of REC_TILE pose atoms, pose).  The
// ligand is gathered into LDS once per block, 16 bytes per atom (x, y, z, radius - negated for an inactive atom - in ONE
// ds_read_b128, the same address for all lanes: a broadcast); every thread owns one pose atom and walks the ligand in ascending
// order.  Every pair's value is d = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx))) and d / (r_a + r_j) wherever it is computed, and
// the minimum is exact: the key (bits of the ratio, a, j) is ordered as the triple is because ratios are non-negative, so the
// result does not depend on the tile size or the launch and the lexicographically smallest (a, j) wins a tie.  A block stores
// its two partial minima to ws[p][tile]; validity_pose_kernel (one block per pose) takes their minimum, computes the checks
// inside the ligand (fp32; column 7 in double: one thread per group, eigenvalues by cyclic Jacobi on the 3x3 covariance, the normal
// as the largest cross product of two rows of C - lambda I) and the flags.
#include "common.h"
#include "geom3.h"
#include "physdock_hip.h"

namespace {

constexpr int VAL_MAX_L = 1024;        // ligand atoms: 16 KiB of LDS, and 10 bits of the key
constexpr int VAL_MAX_G = 256;         // planar groups: one thread of the pose kernel each
constexpr int VAL_GROUP = 8;           // atoms per planar group (rows of `planar`, padded with -1)
constexpr int VAL_MAX_A = 1 << 22;     // pose atoms: 22 bits of the key
constexpr int REC_TILE = 256;          // pose atoms per block of the receptor kernel (PD_VALIDITY_REC_TILE of the header)
static_assert(REC_TILE == PD_VALIDITY_REC_TILE, "the workspace size the header documents");

__device__ __forceinline__ float dist(const f32x4 a, const f32x4 b) {
    const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
}

// the ligand of pose p into LDS: (x, y, z, +radius) of an active atom, (x, y, z, -radius) of an inactive one
__device__ __forceinline__ void stage_ligand(f32x4* sm, const float* __restrict__ xp, const int* __restrict__ lig_idx,
                                             const float* __restrict__ radius, const unsigned char* __restrict__ lig_active, int L) {
    for (int a = threadIdx.x; a < L; a += blockDim.x) {
        const int k = lig_idx[a];
        const float r = radius[k];
        const f32x4 v = {xp[3 * k], xp[3 * k + 1], xp[3 * k + 2], lig_active[a] ? r : -r};
        sm[a] = v;
    }
}

__global__ __launch_bounds__(REC_TILE) void validity_receptor_kernel(const float* __restrict__ x, const int* __restrict__ lig_idx,
                                                                    const float* __restrict__ radius,
                                                                    const unsigned char* __restrict__ rec_mask,
                                                                    const unsigned char* __restrict__ lig_active,
                                                                    pd_u64* __restrict__ ws, int A, int L) {
    extern __shared__ f32x4 sm[];          // [L]
    __shared__ pd_u64 red[REC_TILE / 64][2];
    const int tid = threadIdx.x, tile = blockIdx.x, p = blockIdx.y;
    const float* xp = x + (long long)p * A * 3;
    stage_ligand(sm, xp, lig_idx, radius, lig_active, L);
    __syncthreads();
    const int j = tile * REC_TILE + tid;
    pd_u64 kr = PD_KEY_NONE, kd = PD_KEY_NONE;   // (ratio, a, j) and (distance, -)
    if (j < A && rec_mask[j]) {
        const f32x4 xj = {xp[3 * j], xp[3 * j + 1], xp[3 * j + 2], 0.f};
        const float rj = radius[j];
        float best = __uint_as_float(0x7f800000u), dmin = best;
        int best_a = -1;
        for (int a = 0; a < L; ++a) {
            const f32x4 xa = sm[a];
            if (!(xa[3] > 0.f)) continue;
            const float d = dist(xa, xj), q = d / (xa[3] + rj);
            dmin = fminf(dmin, d);
            if (q < best) { best = q; best_a = a; }          // ascending a: the smallest a keeps an exact tie
        }
        if (best_a >= 0) kr = ((pd_u64)__float_as_uint(best) << 32) | ((unsigned)best_a << 22) | (unsigned)j;
        kd = ((pd_u64)__float_as_uint(dmin) << 32) | 0xffffffffu;
    }
    kr = pd_wave_key_min(kr);
    kd = pd_wave_key_min(kd);
    if ((tid & 63) == 0) { red[tid >> 6][0] = kr; red[tid >> 6][1] = kd; }
    __syncthreads();
    if (tid < 2) {
        pd_u64 k = red[0][tid];
#pragma unroll
        for (int w = 1; w < REC_TILE / 64; ++w) k = pd_key_min(k, red[w][tid]);
        ws[((long long)p * gridDim.x + tile) * 2 + tid] = k;
    }
}

// largest distance (Angstrom) of a group's atoms to its least-squares plane, in double; 0 for a group without a plane
__device__ __forceinline__ double group_planarity(const f32x4* sm, const int* __restrict__ grp) {
    double cx = 0.0, cy = 0.0, cz = 0.0;
    int n = 0;
#pragma unroll
    for (int e = 0; e < VAL_GROUP; ++e) {
        const int a = grp[e];
        if (a < 0) continue;
        const f32x4 v = sm[a];
        cx += (double)v[0]; cy += (double)v[1]; cz += (double)v[2];
        ++n;
    }
    if (n < 4) return 0.0;                  // three points always lie in a plane
    cx /= n; cy /= n; cz /= n;
    double c00 = 0.0, c11 = 0.0, c22 = 0.0, c01 = 0.0, c02 = 0.0, c12 = 0.0;
#pragma unroll
    for (int e = 0; e < VAL_GROUP; ++e) {
        const int a = grp[e];
        if (a < 0) continue;
        const f32x4 v = sm[a];
        const double dx = (double)v[0] - cx, dy = (double)v[1] - cy, dz = (double)v[2] - cz;
        c00 += dx * dx; c11 += dy * dy; c22 += dz * dz; c01 += dx * dy; c02 += dx * dz; c12 += dy * dz;
    }
    c00 /= n; c11 /= n; c22 /= n; c01 /= n; c02 /= n; c12 /= n;
    // (this tail is also in receptor_geometry.hip: as a shared function it changes the instructions of both kernels)
    double a00 = c00, a11 = c11, a22 = c22, a01 = c01, a02 = c02, a12 = c12;
#pragma unroll 1
    for (int sweep = 0; sweep < 10; ++sweep) {          // cyclic Jacobi converges quadratically: 3x3 is done after five or six
        jacobi(a00, a11, a01, a02, a12);
        jacobi(a00, a22, a02, a01, a12);
        jacobi(a11, a22, a12, a01, a02);
    }
    const double lo = fmin(a00, fmin(a11, a22)), hi = fmax(a00, fmax(a11, a22)), mid = a00 + a11 + a22 - lo - hi;
    if (!(mid > 1e-10 * hi)) return 0.0;
    // the plane's normal spans the null space of C - lo I, whose rows span the plane: the largest cross product of two rows
    const double r00 = c00 - lo, r11 = c11 - lo, r22 = c22 - lo;
    const double ux = c01 * c12 - c02 * r11, uy = c02 * c01 - r00 * c12, uz = r00 * r11 - c01 * c01;        // row 0 x row 1
    const double vx = c01 * r22 - c02 * c12, vy = c02 * c02 - r00 * r22, vz = r00 * c12 - c01 * c02;        // row 0 x row 2
    const double wx = r11 * r22 - c12 * c12, wy = c12 * c02 - c01 * r22, wz = c01 * c12 - r11 * c02;        // row 1 x row 2
    const double nu = ux * ux + uy * uy + uz * uz, nv = vx * vx + vy * vy + vz * vz, nw = wx * wx + wy * wy + wz * wz;
    const bool pv = nv > nu;
    double nx = pv ? vx : ux, ny = pv ? vy : uy, nz = pv ? vz : uz, nn = pv ? nv : nu;
    const bool pw = nw > nn;
    nx = pw ? wx : nx; ny = pw ? wy : ny; nz = pw ? wz : nz; nn = pw ? nw : nn;
    if (!(nn > 0.0)) return 0.0;
    const double inv = 1.0 / sqrt(nn);
    double out = 0.0;
#pragma unroll
    for (int e = 0; e < VAL_GROUP; ++e) {
        const int a = grp[e];
        if (a < 0) continue;
        const f32x4 v = sm[a];
        out = fmax(out, fabs(nx * ((double)v[0] - cx) + ny * ((double)v[1] - cy) + nz * ((double)v[2] - cz)) * inv);
    }
    return out;
}

__global__ __launch_bounds__(256) void validity_pose_kernel(const float* __restrict__ x, const int* __restrict__ lig_idx,
                                                           const float* __restrict__ radius,
                                                           const unsigned char* __restrict__ lig_active,
                                                           const int* __restrict__ pair12, const float* __restrict__ d12_ref,
                                                           const int* __restrict__ pair13, const float* __restrict__ d13_ref,
                                                           const unsigned char* __restrict__ far, const int* __restrict__ planar,
                                                           const pd_validity_thresholds thr, const pd_u64* __restrict__ ws,
                                                           float* __restrict__ val, int* __restrict__ worst,
                                                           int* __restrict__ flags, int A, int L, int n12, int n13, int G,
                                                           int ntiles) {
    extern __shared__ f32x4 sm[];          // [L]
    __shared__ float redf[4][6];
    __shared__ pd_u64 redk[4][2];
    const int tid = threadIdx.x, p = blockIdx.x;
    const float INF = __uint_as_float(0x7f800000u);
    stage_ligand(sm, x + (long long)p * A * 3, lig_idx, radius, lig_active, L);
    __syncthreads();
    float lo12 = INF, hi12 = 0.f, lo13 = INF, hi13 = 0.f, clash = INF, plane = 0.f;
    for (int k = tid; k < n12; k += 256) {
        const float q = dist(sm[pair12[2 * k]], sm[pair12[2 * k + 1]]) / d12_ref[k];
        lo12 = fminf(lo12, q); hi12 = fmaxf(hi12, q);
    }
    for (int k = tid; k < n13; k += 256) {
        const float q = dist(sm[pair13[2 * k]], sm[pair13[2 * k + 1]]) / d13_ref[k];
        lo13 = fminf(lo13, q); hi13 = fmaxf(hi13, q);
    }
    for (int k = tid; k < L * L; k += 256) {
        const int a = k / L, b = k - a * L;
        if (a >= b || !far[k]) continue;
        const f32x4 xa = sm[a], xb = sm[b];
        if (xa[3] > 0.f && xb[3] > 0.f) clash = fminf(clash, dist(xa, xb) / (xa[3] + xb[3]));
    }
    if (tid < G) plane = (float)group_planarity(sm, planar + tid * VAL_GROUP);
    pd_u64 kr = PD_KEY_NONE, kd = PD_KEY_NONE;
    for (int t = tid; t < ntiles; t += 256) {
        kr = pd_key_min(kr, ws[((long long)p * ntiles + t) * 2]);
        kd = pd_key_min(kd, ws[((long long)p * ntiles + t) * 2 + 1]);
    }
    lo12 = wave_min(lo12); hi12 = wave_max(hi12); lo13 = wave_min(lo13); hi13 = wave_max(hi13);
    clash = wave_min(clash); plane = wave_max(plane);
    kr = pd_wave_key_min(kr); kd = pd_wave_key_min(kd);
    if ((tid & 63) == 0) {
        float* r = redf[tid >> 6];
        r[0] = lo12; r[1] = hi12; r[2] = lo13; r[3] = hi13; r[4] = clash; r[5] = plane;
        redk[tid >> 6][0] = kr; redk[tid >> 6][1] = kd;
    }
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < 4; ++w) {
        lo12 = fminf(lo12, redf[w][0]); hi12 = fmaxf(hi12, redf[w][1]); lo13 = fminf(lo13, redf[w][2]); hi13 = fmaxf(hi13, redf[w][3]);
        clash = fminf(clash, redf[w][4]); plane = fmaxf(plane, redf[w][5]);
        kr = pd_key_min(kr, redk[w][0]); kd = pd_key_min(kd, redk[w][1]);
    }
    if (n12 == 0) lo12 = hi12 = 1.f;
    if (n13 == 0) lo13 = hi13 = 1.f;
    const float rec = __uint_as_float((unsigned)(kr >> 32)), rec_d = __uint_as_float((unsigned)(kd >> 32));
    const unsigned pair = (unsigned)kr;
    float* v = val + (long long)p * 8;
    v[0] = lo12; v[1] = hi12; v[2] = lo13; v[3] = hi13; v[4] = clash; v[5] = rec; v[6] = rec_d; v[7] = plane;
    worst[2 * p] = kr == PD_KEY_NONE ? -1 : (int)(pair >> 22);
    worst[2 * p + 1] = kr == PD_KEY_NONE ? -1 : (int)(pair & (VAL_MAX_A - 1));
    int f = 0;
    if (lo12 < thr.bond_lo || hi12 > thr.bond_hi) f |= 1;
    if (lo13 < thr.angle_lo || hi13 > thr.angle_hi) f |= 2;
    if (clash < thr.internal_clash) f |= 4;
    if (rec < thr.receptor_clash) f |= 8;
    if (plane > thr.planarity) f |= 16;
    if (rec_d > thr.detached && rec_d < INF) f |= 32;
    flags[p] = f;
}

}  // namespace

PD_EXPORT int pd_pose_validity_workspace_numel(int P, int A) {
    if (P <= 0 || A <= 0) return PD_ERR_ARG;
    if (A > VAL_MAX_A || P > 65535) return PD_ERR_UNSUPPORTED;
    return P * ((A + REC_TILE - 1) / REC_TILE) * 2;          // at most 65535 * 2^14 * 2 < 2^31
}

PD_EXPORT int pd_pose_validity(const float* x, const int* lig_idx, const float* radius, const unsigned char* rec_mask,
                               const unsigned char* lig_active, const int* pair12, const float* d12_ref, const int* pair13,
                               const float* d13_ref, const unsigned char* far, const int* planar, pd_validity_thresholds thr,
                               unsigned long long* ws, float* val, int* worst, int* flags, int P, int A, int L, int n12, int n13,
                               int G, void* stream) {
    if (!x || !lig_idx || !radius || !rec_mask || !lig_active || !far || !ws || !val || !worst || !flags) return PD_ERR_ARG;
    if (P <= 0 || A <= 0 || L <= 0 || n12 < 0 || n13 < 0 || G < 0) return PD_ERR_ARG;
    if ((n12 && (!pair12 || !d12_ref)) || (n13 && (!pair13 || !d13_ref)) || (G && !planar)) return PD_ERR_ARG;
    if (L > VAL_MAX_L || G > VAL_MAX_G || A > VAL_MAX_A || P > 65535) return PD_ERR_UNSUPPORTED;
    const int ntiles = (A + REC_TILE - 1) / REC_TILE;
    hipLaunchKernelGGL(validity_receptor_kernel, dim3(ntiles, P), dim3(REC_TILE), (size_t)L * sizeof(f32x4), (hipStream_t)stream,
                       x, lig_idx, radius, rec_mask, lig_active, (pd_u64*)ws, A, L);
    hipLaunchKernelGGL(validity_pose_kernel, dim3(P), dim3(256), (size_t)L * sizeof(f32x4), (hipStream_t)stream,
                       x, lig_idx, radius, lig_active, pair12, d12_ref, pair13, d13_ref, far, planar, thr, (const pd_u64*)ws, val,
                       worst, flags, A, L, n12, n13, G, ntiles);
    return pd_check_launch();
}
