// Float64 3-vector geometry shared by the pose kernels: a vector of three doubles, the Jacobi rotation of the plane fits and the 4x4
// cyclic Jacobi of Horn's superposition quaternion.
#pragma once
#include <hip/hip_runtime.h>

struct Vec3 {
    double x, y, z;
};
__device__ __forceinline__ Vec3 sub(Vec3 a, Vec3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ Vec3 add(Vec3 a, Vec3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ Vec3 neg(Vec3 a) { return {-a.x, -a.y, -a.z}; }
__device__ __forceinline__ double dot(Vec3 a, Vec3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ Vec3 cross(Vec3 a, Vec3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ Vec3 load3(const double* p) { return {p[0], p[1], p[2]}; }
__device__ __forceinline__ Vec3 load3(const float* p) { return {(double)p[0], (double)p[1], (double)p[2]}; }
__device__ __forceinline__ bool finite3(float a, float b, float c) { return isfinite(a) && isfinite(b) && isfinite(c); }
__device__ __forceinline__ bool finite3(Vec3 v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z); }

// one Jacobi rotation of the symmetric 3x3 matrix in the (p, q) plane: app, aqq the diagonal entries, apq the entry it annihilates,
// arp, arq the entries of the third row.  Values only (the callers take the eigenvector from a cross product): no indexing, no stack.
__device__ __forceinline__ void jacobi(double& app, double& aqq, double& apq, double& arp, double& arq) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app -= t * apq;
    aqq += t * apq;
    apq = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp; arq = rq;
}

// ---- Horn's quaternion of a superposition (bestfit_rmsd.hip, pocket_accuracy.hip)
constexpr int HORN_MAX_SWEEPS = 50;     // cyclic Jacobi converges quadratically: a 4x4 is done after six to eight

// One Jacobi rotation in the (P, Q) plane of the symmetric 4x4 matrix a (upper triangle) and, with VEC, of the eigenvector matrix v:
// the formulas of Rutishauser / Numerical Recipes.  Compile-time indices only: everything stays in registers.
template <int P, int Q, bool VEC>
__host__ __device__ __forceinline__ void horn_rotate(double (&a)[4][4], double (&v)[4][4], int sweep) {
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    const double g = 100.0 * fabs(apq);
    if (sweep > 3 && fabs(a[P][P]) + g == fabs(a[P][P]) && fabs(a[Q][Q]) + g == fabs(a[Q][Q])) {
        a[P][Q] = 0.0;
        return;
    }
    const double h = a[Q][Q] - a[P][P];
    double t;
    if (fabs(h) + g == fabs(h)) {
        t = apq / h;
    } else {
        const double theta = 0.5 * h / apq;
        t = 1.0 / (fabs(theta) + sqrt(1.0 + theta * theta));
        if (theta < 0.0) t = -t;
    }
    const double c = 1.0 / sqrt(1.0 + t * t), s = t * c, tau = s / (1.0 + c);
    a[P][P] -= t * apq;
    a[Q][Q] += t * apq;
    a[P][Q] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r == P || r == Q) continue;
        double& arp = r < P ? a[r][P] : a[P][r];
        double& arq = r < Q ? a[r][Q] : a[Q][r];
        const double x = arp, y = arq;
        arp = x - s * (y + x * tau);
        arq = y + s * (x - y * tau);
    }
    if (VEC) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double x = v[r][P], y = v[r][Q];
            v[r][P] = x - s * (y + x * tau);
            v[r][Q] = y + s * (x - y * tau);
        }
    }
}

// lambda_max of Horn's matrix N of the covariance S[3 x + y] = sum_k a[k][x] b[k][y]; with VEC also its unit eigenvector q = (w, x, y,
// z), first non-zero component positive (the first of equal eigenvalues)
template <bool VEC>
__host__ __device__ inline double horn_lambda_max(const double (&S)[9], double* q) {
    const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
    double a[4][4], v[4][4];
    a[0][0] = Sxx + Syy + Szz; a[0][1] = Syz - Szy;       a[0][2] = Szx - Sxz;        a[0][3] = Sxy - Syx;
    a[1][1] = Sxx - Syy - Szz; a[1][2] = Sxy + Syx;       a[1][3] = Szx + Sxz;
    a[2][2] = -Sxx + Syy - Szz; a[2][3] = Syz + Szy;
    a[3][3] = -Sxx - Syy + Szz;
    a[1][0] = a[2][0] = a[2][1] = a[3][0] = a[3][1] = a[3][2] = 0.0;      // (the lower triangle is never read)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) v[r][c] = r == c ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < HORN_MAX_SWEEPS; ++sweep) {
        const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[0][3]) + fabs(a[1][2]) + fabs(a[1][3]) + fabs(a[2][3]);
        if (off == 0.0) break;
        horn_rotate<0, 1, VEC>(a, v, sweep);
        horn_rotate<0, 2, VEC>(a, v, sweep);
        horn_rotate<0, 3, VEC>(a, v, sweep);
        horn_rotate<1, 2, VEC>(a, v, sweep);
        horn_rotate<1, 3, VEC>(a, v, sweep);
        horn_rotate<2, 3, VEC>(a, v, sweep);
    }
    double lam = a[0][0];
    int best = 0;
    if (a[1][1] > lam) { lam = a[1][1]; best = 1; }
    if (a[2][2] > lam) { lam = a[2][2]; best = 2; }
    if (a[3][3] > lam) { lam = a[3][3]; best = 3; }
    if (VEC) {
        double w = 0.0, x = 0.0, y = 0.0, z = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c == best) { w = v[0][c]; x = v[1][c]; y = v[2][c]; z = v[3][c]; }
        const double inv = 1.0 / sqrt(w * w + x * x + y * y + z * z);
        const double lead = w != 0.0 ? w : (x != 0.0 ? x : (y != 0.0 ? y : z));
        const double sgn = lead < 0.0 ? -inv : inv;
        q[0] = w * sgn; q[1] = x * sgn; q[2] = y * sgn; q[3] = z * sgn;
    }
    return lam;
}
