// Float64 3-vector geometry shared by the pose kernels: a vector of three doubles and the Jacobi rotation of the plane fits.
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
