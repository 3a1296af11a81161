// Stereochemistry checks of the RECEPTOR of P poses (physdock_amd/receptor_geometry.py builds the tables once per system from the
// residue and atom names and a reference structure; tests/receptor_geometry_ref.py is the float64 restatement).  With x_a the fp32
// position of pose atom a, d(a,b) = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx))) and r a van der Waals radius:
//
//   bit 0 bond_lengths   term (a, b), reference length l:  q = d(a,b) / l (fp32);            fails unless bond_lo <= q <= bond_hi
//   bit 1 bond_angles    the same for the 1-3 pairs and angle_lo, angle_hi                    (a 1-3 distance pins the bond angle)
//   bit 2 chirality      term (c, a, b, e), sign s = +-1:  V = (x_a - x_c) . ((x_b - x_c) x (x_e - x_c)) in double; fails unless
//                        s V > 0; the term's value is s V
//   bit 3 peptide_twist  term (CA, C, N', CA'): w = the dihedral below, in degrees; value t = min(|w|, 180 - |w|); fails when t > twist
//   bit 4 cis_flip       the same term, where the reference is trans (|w_ref| > 150, decided on the host): fails when |w| < cis
//   bit 5 planarity      term = a group of 4 .. 10 atoms: value = the largest distance of an atom to the group's least-squares plane
//                        (double; centroid c, normal = the eigenvector of the smallest eigenvalue of the covariance matrix, cyclic
//                        Jacobi, the normal as the largest cross product of two rows of C - lambda I - the method of validity.hip; 0
//                        when the second eigenvalue is at most 1e-10 of the largest); fails when the fp32 value > planarity
//   bit 6 clash          pair i < j, both active (radius > 0), not in the exclusion list: q = d(i,j) / (r_i + r_j) (fp32); fails when
//                        q < clash
//
// A term one of whose coordinates is not finite fails (its first bit: a peptide term fails bit 3) and reports a sentinel: +inf
// (bits 0, 1, 3, 5), -inf (bit 2); a clash pair with such an atom fails and reports q = 0.  Per pose:
//
//   val[p][0..3]  min, max of the bond values; min, max of the 1-3 values      (1 without terms)
//   val[p][4]     min of q over the clash pairs (+inf without pairs);  worst[p] = the (i, j) that attains it, the smallest (i, j) on an
//                 exact tie ((-1, -1) without pairs): the minimum of the key (bits of q, i, j), exact because q >= 0
//   val[p][5]     max of the planarity values (0 without groups)     val[p][6]  max of the twist values (0 without peptide terms)
//   val[p][7]     the number of failing chirality terms, as a float
//   counts[p][b]  failing terms of bit b (b = 6: failing pairs i < j), int32;  flags[p] bit b = counts[p][b] > 0
//   residue_flags[p][r]  OR of the fail bits of the terms that hold an atom of residue r (CSR res_term), bit 6 when an atom of r
//                 (CSR res_atom) has atom_clash;  atom_clash[p][i] = 1 when atom i is in a failing pair (as i or as j)
//   term_val[p][t], term_fail[p][t]  every term's value (fp32) and fail bits (the bit mask itself)
//
// The dihedral of (p0, p1, p2, p3), in double from the fp32 coordinates: b1 = p1 - p0, b2 = p2 - p1, b3 = p3 - p2, m = b1 x b2,
// n = b2 x b3, w = atan2(|b2| b1 . n, m . n) in degrees, rounded to fp32 once; NaN when an index is -1, a coordinate is not finite or
// |m| < 1e-6 or |n| < 1e-6.  pd_receptor_dihedrals writes it for the [R][7][4] index table (phi, psi, omega, chi1 - chi4).
//
// Four kernels, no atomics, every result bit-identical from launch to launch and whatever the number of poses.  rg_clash_kernel: one
// block of 256 threads per (tile of 256 atoms, pose); a thread owns atom i and walks ALL atoms j (not a triangle: every atom gets its
// own minimum, count and bit without a cross-block OR) in tiles staged in LDS as (x, y, z, radius) - x = NaN for an atom with a
// non-finite coordinate, radius < 0 for an inactive one - read with one ds_read_b128 per j, the same address for all lanes.  The inner
// test is d2 >= lim (r_i + r_j)^2 on squared distances with lim = 1.0001 max(best^2, clash^2), a superset of "q < best or q < clash";
// only a pair that passes it consults the exclusion list (CSR per atom over the partners with a higher index) and computes q.
// rg_terms_kernel: one thread per (term, pose).  rg_reduce_kernel: one block per pose, minima / maxima / integer sums (any order gives
// the same bits) and the residue bytes through the two CSRs.  rg_dihedral_kernel: one thread per (residue, angle, pose).
#include "common.h"
#include "geom3.h"
#include "physdock_hip.h"

namespace {

constexpr int RG_MAX_A = 4096;         // atoms: 12 bits of the key each for i and j
constexpr int RG_MAX_R = 4096;         // residues
constexpr int RG_MAX_T = 1 << 20;      // terms
constexpr int RG_WIDTH = 10;           // atoms per term row (PD_RECEPTOR_TERM_WIDTH of the header)
constexpr int RG_TILE = 256;
static_assert(RG_WIDTH == PD_RECEPTOR_TERM_WIDTH, "the row width the header documents");
constexpr double RAD2DEG = 57.295779513082320876798154814105;

__device__ __forceinline__ bool excluded(const int* __restrict__ excl_start, const int* __restrict__ excl_atom, int i, int j) {
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    for (int k = excl_start[lo]; k < excl_start[lo + 1]; ++k)
        if (excl_atom[k] == hi) return true;
    return false;
}

__global__ __launch_bounds__(RG_TILE) void rg_clash_kernel(const float* __restrict__ x, const float* __restrict__ radius,
                                                          const int* __restrict__ excl_start, const int* __restrict__ excl_atom,
                                                          float clash, pd_u64* __restrict__ akey, int* __restrict__ acount,
                                                          unsigned char* __restrict__ atom_clash, int A) {
    __shared__ f32x4 sm[RG_TILE];
    const int tid = threadIdx.x, i = blockIdx.x * RG_TILE + tid, p = blockIdx.y;
    const float* xp = x + (long long)p * A * 3;
    const float INF = __uint_as_float(0x7f800000u), QNAN = __uint_as_float(0x7fc00000u);
    float xi = 0.f, yi = 0.f, zi = 0.f, ri = -1.f;
    if (i < A) {
        xi = xp[3 * i]; yi = xp[3 * i + 1]; zi = xp[3 * i + 2]; ri = radius[i];
        if (!finite3(xi, yi, zi)) xi = QNAN;
    }
    const bool active = ri > 0.f;
    const float clash2 = clash * clash;
    float best = INF, lim = INF;
    int best_j = -1, count = 0, bit = 0;
    for (int j0 = 0; j0 < A; j0 += RG_TILE) {
        __syncthreads();
        {
            const int j = j0 + tid;
            f32x4 v = {0.f, 0.f, 0.f, -1.f};
            if (j < A) {
                v[0] = xp[3 * j]; v[1] = xp[3 * j + 1]; v[2] = xp[3 * j + 2]; v[3] = radius[j];
                if (!finite3(v[0], v[1], v[2])) v[0] = QNAN;
            }
            sm[tid] = v;
        }
        __syncthreads();
        if (!active) continue;
        const int n = A - j0 < RG_TILE ? A - j0 : RG_TILE;
        for (int jj = 0; jj < n; ++jj) {
            const f32x4 v = sm[jj];
            if (!(v[3] > 0.f)) continue;                     // an inactive atom: the same for every lane
            const float dx = xi - v[0], dy = yi - v[1], dz = zi - v[2];
            const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)), s = ri + v[3];
            if (d2 >= lim * (s * s)) continue;               // (a NaN distance passes on)
            const int j = j0 + jj;
            if (j == i || excluded(excl_start, excl_atom, i, j)) continue;
            float q = sqrtf(d2) / s;
            if (!(q == q)) q = 0.f;                          // an atom without a position: the pair fails and reports 0
            if (q < best) {                                  // ascending j: the smallest j keeps an exact tie
                best = q; best_j = j;
                lim = fmaxf(best * best, clash2) * 1.0001f;
            }
            if (q < clash) { bit = 1; count += j > i; }
        }
    }
    if (i < A) {
        const unsigned lo = best_j < i ? best_j : i, hi = best_j < i ? i : best_j;
        akey[(long long)p * A + i] = best_j < 0 ? PD_KEY_NONE : ((pd_u64)__float_as_uint(best) << 32) | (lo << 12) | hi;
        acount[(long long)p * A + i] = count;
        atom_clash[(long long)p * A + i] = (unsigned char)bit;
    }
}

// position of atom a of a pose in double; ok turns false when a < 0 or a coordinate is not finite
__device__ __forceinline__ Vec3 load(const float* __restrict__ xp, int a, bool& ok) {
    if (a < 0) { ok = false; return {0.0, 0.0, 0.0}; }
    const float u = xp[3 * a], v = xp[3 * a + 1], w = xp[3 * a + 2];
    ok = ok && finite3(u, v, w);
    return {(double)u, (double)v, (double)w};
}

// the dihedral of four atoms in degrees (double), NaN where it is not defined
__device__ __forceinline__ double dihedral_deg(const float* __restrict__ xp, const int* __restrict__ idx) {
    bool ok = true;
    const Vec3 p0 = load(xp, idx[0], ok), p1 = load(xp, idx[1], ok), p2 = load(xp, idx[2], ok), p3 = load(xp, idx[3], ok);
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    if (!ok) return nan;
    const Vec3 b1 = sub(p1, p0), b2 = sub(p2, p1), b3 = sub(p3, p2), m = cross(b1, b2), n = cross(b2, b3);
    if (!(dot(m, m) >= 1e-12) || !(dot(n, n) >= 1e-12)) return nan;
    return atan2(sqrt(dot(b2, b2)) * dot(b1, n), dot(m, n)) * RAD2DEG;
}

// largest distance of a group's atoms to its least-squares plane, in double; 0 for a group without a plane, +inf for one with a
// coordinate that is not finite
__device__ __forceinline__ double group_planarity(const float* __restrict__ xp, const int* __restrict__ grp) {
    double cx = 0.0, cy = 0.0, cz = 0.0;
    int n = 0;
    bool ok = true;
#pragma unroll 1
    for (int e = 0; e < RG_WIDTH; ++e) {
        if (grp[e] < 0) continue;
        const Vec3 v = load(xp, grp[e], ok);
        cx += v.x; cy += v.y; cz += v.z;
        ++n;
    }
    if (!ok) return __longlong_as_double(0x7ff0000000000000LL);
    if (n < 4) return 0.0;
    cx /= n; cy /= n; cz /= n;
    double c00 = 0.0, c11 = 0.0, c22 = 0.0, c01 = 0.0, c02 = 0.0, c12 = 0.0;
#pragma unroll 1
    for (int e = 0; e < RG_WIDTH; ++e) {
        if (grp[e] < 0) continue;
        const Vec3 v = load(xp, grp[e], ok);
        const double dx = v.x - cx, dy = v.y - cy, dz = v.z - cz;
        c00 += dx * dx; c11 += dy * dy; c22 += dz * dz; c01 += dx * dy; c02 += dx * dz; c12 += dy * dz;
    }
    c00 /= n; c11 /= n; c22 /= n; c01 /= n; c02 /= n; c12 /= n;
    // (this tail is also in validity.hip: as a shared function it changes the instructions of both kernels)
    double a00 = c00, a11 = c11, a22 = c22, a01 = c01, a02 = c02, a12 = c12;
#pragma unroll 1
    for (int sweep = 0; sweep < 10; ++sweep) {
        jacobi(a00, a11, a01, a02, a12);
        jacobi(a00, a22, a02, a01, a12);
        jacobi(a11, a22, a12, a01, a02);
    }
    const double lo = fmin(a00, fmin(a11, a22)), hi = fmax(a00, fmax(a11, a22)), mid = a00 + a11 + a22 - lo - hi;
    if (!(mid > 1e-10 * hi)) return 0.0;
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
#pragma unroll 1
    for (int e = 0; e < RG_WIDTH; ++e) {
        if (grp[e] < 0) continue;
        const Vec3 v = load(xp, grp[e], ok);
        out = fmax(out, fabs(nx * (v.x - cx) + ny * (v.y - cy) + nz * (v.z - cz)) * inv);
    }
    return out;
}

// the first term of every kind: bonds from 0, 1-3 pairs from o[0], centres from o[1], peptide terms from o[2], groups from o[3] to T
struct rg_offsets { int o[4]; };

__global__ __launch_bounds__(256) void rg_terms_kernel(const float* __restrict__ x, const int* __restrict__ term_atoms,
                                                      const float* __restrict__ term_ref, const rg_offsets off,
                                                      const pd_receptor_thresholds thr, float* __restrict__ term_val,
                                                      unsigned char* __restrict__ term_fail, int A, int T) {
    const int t = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
    if (t >= T) return;
    const float* xp = x + (long long)p * A * 3;
    const int* at = term_atoms + (long long)t * RG_WIDTH;
    const float INF = __uint_as_float(0x7f800000u);
    float value;
    int fail;
    if (t < off.o[1]) {
        const int a = at[0], b = at[1];
        const float dx = xp[3 * a] - xp[3 * b], dy = xp[3 * a + 1] - xp[3 * b + 1], dz = xp[3 * a + 2] - xp[3 * b + 2];
        float q = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx))) / term_ref[t];
        if (!isfinite(q)) q = INF;
        const bool bond = t < off.o[0];
        value = q;
        fail = (q >= (bond ? thr.bond_lo : thr.angle_lo) && q <= (bond ? thr.bond_hi : thr.angle_hi)) ? 0 : (bond ? 1 : 2);
    } else if (t < off.o[2]) {
        bool ok = true;
        const Vec3 c = load(xp, at[0], ok), va = sub(load(xp, at[1], ok), c), vb = sub(load(xp, at[2], ok), c), ve = sub(load(xp, at[3], ok), c);
        const double sv = dot(va, cross(vb, ve)) * (double)term_ref[t];
        value = ok ? (float)sv : -INF;
        fail = (ok && sv > 0.0) ? 0 : 4;
    } else if (t < off.o[3]) {
        const double w = dihedral_deg(xp, at);
        if (w == w) {
            const double aw = fabs(w), tw = fmin(aw, 180.0 - aw);
            value = (float)tw;
            fail = (tw > (double)thr.twist ? 8 : 0) | ((term_ref[t] > 0.5f && aw < (double)thr.cis) ? 16 : 0);
        } else {
            value = INF;
            fail = 8;
        }
    } else {
        value = (float)group_planarity(xp, at);
        fail = value > thr.planarity ? 32 : 0;
    }
    term_val[(long long)p * T + t] = value;
    term_fail[(long long)p * T + t] = (unsigned char)fail;
}

__global__ __launch_bounds__(256) void rg_reduce_kernel(const float* __restrict__ term_val, const unsigned char* __restrict__ term_fail,
                                                       const rg_offsets off, const pd_u64* __restrict__ akey,
                                                       const int* __restrict__ acount, const unsigned char* __restrict__ atom_clash,
                                                       const int* __restrict__ res_term_start, const int* __restrict__ res_term,
                                                       const int* __restrict__ res_atom_start, const int* __restrict__ res_atom,
                                                       float* __restrict__ val, int* __restrict__ worst, int* __restrict__ counts,
                                                       int* __restrict__ flags, unsigned char* __restrict__ residue_flags, int A, int R,
                                                       int T) {
    __shared__ float redf[4][6];
    __shared__ int redi[4][7];
    __shared__ pd_u64 redk[4];
    const int tid = threadIdx.x, p = blockIdx.x;
    const float INF = __uint_as_float(0x7f800000u);
    const float* tv = term_val + (long long)p * T;
    const unsigned char* tf = term_fail + (long long)p * T;
    float f[6] = {INF, 0.f, INF, 0.f, 0.f, 0.f};      // min, max bond; min, max 1-3; max plane; max twist
    int c[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int t = tid; t < T; t += 256) {
        const float v = tv[t];
        const int b = tf[t];
        if (t < off.o[0]) { f[0] = fminf(f[0], v); f[1] = fmaxf(f[1], v); }
        else if (t < off.o[1]) { f[2] = fminf(f[2], v); f[3] = fmaxf(f[3], v); }
        else if (t < off.o[2]) {}
        else if (t < off.o[3]) f[5] = fmaxf(f[5], v);
        else f[4] = fmaxf(f[4], v);
#pragma unroll
        for (int k = 0; k < 6; ++k) c[k] += (b >> k) & 1;
    }
    pd_u64 key = PD_KEY_NONE;
    for (int a = tid; a < A; a += 256) {
        key = pd_key_min(key, akey[(long long)p * A + a]);
        c[6] += acount[(long long)p * A + a];
    }
    for (int r = tid; r < R; r += 256) {
        int byte = 0;
        for (int k = res_term_start[r]; k < res_term_start[r + 1]; ++k) byte |= tf[res_term[k]];
        for (int k = res_atom_start[r]; k < res_atom_start[r + 1]; ++k)
            if (atom_clash[(long long)p * A + res_atom[k]]) byte |= 64;
        residue_flags[(long long)p * R + r] = (unsigned char)byte;
    }
    f[0] = wave_min(f[0]); f[1] = wave_max(f[1]); f[2] = wave_min(f[2]); f[3] = wave_max(f[3]); f[4] = wave_max(f[4]); f[5] = wave_max(f[5]);
#pragma unroll
    for (int k = 0; k < 7; ++k) c[k] = wave_sum(c[k]);
    key = pd_wave_key_min(key);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) redf[tid >> 6][k] = f[k];
#pragma unroll
        for (int k = 0; k < 7; ++k) redi[tid >> 6][k] = c[k];
        redk[tid >> 6] = key;
    }
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < 4; ++w) {
        f[0] = fminf(f[0], redf[w][0]); f[1] = fmaxf(f[1], redf[w][1]); f[2] = fminf(f[2], redf[w][2]); f[3] = fmaxf(f[3], redf[w][3]);
        f[4] = fmaxf(f[4], redf[w][4]); f[5] = fmaxf(f[5], redf[w][5]);
#pragma unroll
        for (int k = 0; k < 7; ++k) c[k] += redi[w][k];
        key = pd_key_min(key, redk[w]);
    }
    if (off.o[0] == 0) f[0] = f[1] = 1.f;
    if (off.o[1] == off.o[0]) f[2] = f[3] = 1.f;
    float* v = val + (long long)p * 8;
    v[0] = f[0]; v[1] = f[1]; v[2] = f[2]; v[3] = f[3];
    v[4] = __uint_as_float((unsigned)(key >> 32)); v[5] = f[4]; v[6] = f[5]; v[7] = (float)c[2];
    const unsigned pair = (unsigned)key;
    worst[2 * p] = key == PD_KEY_NONE ? -1 : (int)(pair >> 12);
    worst[2 * p + 1] = key == PD_KEY_NONE ? -1 : (int)(pair & (RG_MAX_A - 1));
    int fl = 0;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        counts[p * 7 + k] = c[k];
        fl |= (c[k] > 0) << k;
    }
    flags[p] = fl;
}

__global__ __launch_bounds__(256) void rg_dihedral_kernel(const float* __restrict__ x, const int* __restrict__ dih,
                                                         float* __restrict__ angles, int A, int n) {
    const int k = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
    if (k >= n) return;
    angles[(long long)p * n + k] = (float)dihedral_deg(x + (long long)p * A * 3, dih + 4 * k);
}

}  // namespace

PD_EXPORT int pd_receptor_geometry_workspace_numel(int P, int A) {
    if (P <= 0 || A <= 0) return PD_ERR_ARG;
    if (A > RG_MAX_A || P > 65535) return PD_ERR_UNSUPPORTED;
    return P * A + (P * A + 1) / 2;                     // keys, then counts: at most 65535 * 4096 * 1.5 < 2^31
}

PD_EXPORT int pd_receptor_geometry(const float* x, const float* radius, const int* excl_start, const int* excl_atom,
                                   const int* term_atoms, const float* term_ref, int n_bonds, int n_angles, int n_centres,
                                   int n_peptides, int n_groups, const int* res_term_start, const int* res_term,
                                   const int* res_atom_start, const int* res_atom, pd_receptor_thresholds thr,
                                   unsigned long long* ws, float* val, int* worst, int* counts, int* flags,
                                   unsigned char* residue_flags, unsigned char* atom_clash, float* term_val, unsigned char* term_fail,
                                   int P, int A, int R, void* stream) {
    if (!x || !radius || !excl_start || !res_term_start || !res_atom_start || !ws || !val || !worst || !counts || !flags || !atom_clash)
        return PD_ERR_ARG;
    if (P <= 0 || A <= 0 || R < 0 || n_bonds < 0 || n_angles < 0 || n_centres < 0 || n_peptides < 0 || n_groups < 0) return PD_ERR_ARG;
    if (R > 0 && !residue_flags) return PD_ERR_ARG;
    if (A > RG_MAX_A || R > RG_MAX_R || P > 65535) return PD_ERR_UNSUPPORTED;
    const long long T64 = (long long)n_bonds + n_angles + n_centres + n_peptides + n_groups;
    if (T64 > RG_MAX_T) return PD_ERR_UNSUPPORTED;
    const int T = (int)T64;
    if (T && (!term_atoms || !term_ref || !term_val || !term_fail)) return PD_ERR_ARG;
    rg_offsets off;
    off.o[0] = n_bonds; off.o[1] = off.o[0] + n_angles; off.o[2] = off.o[1] + n_centres; off.o[3] = off.o[2] + n_peptides;
    pd_u64* akey = (pd_u64*)ws;
    int* acount = (int*)(akey + (long long)P * A);
    hipLaunchKernelGGL(rg_clash_kernel, dim3((A + RG_TILE - 1) / RG_TILE, P), dim3(RG_TILE), 0, (hipStream_t)stream, x, radius,
                       excl_start, excl_atom, thr.clash, akey, acount, atom_clash, A);
    if (T)
        hipLaunchKernelGGL(rg_terms_kernel, dim3((T + 255) / 256, P), dim3(256), 0, (hipStream_t)stream, x, term_atoms, term_ref, off,
                           thr, term_val, term_fail, A, T);
    hipLaunchKernelGGL(rg_reduce_kernel, dim3(P), dim3(256), 0, (hipStream_t)stream, (const float*)term_val,
                       (const unsigned char*)term_fail, off, (const pd_u64*)akey, (const int*)acount, (const unsigned char*)atom_clash,
                       res_term_start, res_term, res_atom_start, res_atom, val, worst, counts, flags, residue_flags, A, R, T);
    return pd_check_launch();
}

PD_EXPORT int pd_receptor_dihedrals(const float* x, const int* dih, float* angles, int P, int A, int R, void* stream) {
    if (!x || !dih || !angles || P <= 0 || A <= 0 || R <= 0) return PD_ERR_ARG;
    if (A > RG_MAX_A || R > RG_MAX_R || P > 65535) return PD_ERR_UNSUPPORTED;
    const int n = R * 7;
    hipLaunchKernelGGL(rg_dihedral_kernel, dim3((n + 255) / 256, P), dim3(256), 0, (hipStream_t)stream, x, dih, angles, A, n);
    return pd_check_launch();
}
