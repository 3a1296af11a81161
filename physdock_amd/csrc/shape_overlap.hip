// Gaussian shape and feature ("colour") overlap of molecules, Grant, Gallardo & Pickup 1996 at first order (physdock_amd/shape.py
// builds the tables; tests/shape_overlap_ref.py is the written definition of everything below, in float64 NumPy).  It needs no
// atom correspondence: the two sides may be different ligands in one frame.
//
// Atom i carries the Gaussian p exp(-a_i |r - x_i|^2), p = 2 sqrt 2, a_i = kappa / R_i^2 (the host forms a_i; the kernels never see
// kappa).  O(A,B) = sum_i sum_j p^2 exp(-a_i a_j d_ij^2 / (a_i + a_j)) (pi / (a_i + a_j))^(3/2).  A feature is a kind (0 .. 5) and the
// float64 mean of its member atoms; features are Gaussians of the one exponent `color_alpha`, and only equal kinds overlap: C(A,B).
// shape_tanimoto = O_AB / (O_AA + O_BB - O_AB), color_tanimoto likewise (0 where its denominator is 0), combo their sum.
//
// pd_shape_prepare  : one block per structure.  Gathers the named atoms as float64, forms the feature points and the self-overlaps
//                     O_AA, C_AA into the side's workspace: per structure 3 L + 3 F + 2 doubles.  A non-finite named atom makes both
//                     self-overlaps NaN, and every score of that structure NaN with them.
// pd_shape_overlap  : one block per (row, tile of 16 columns); the row's atoms and feature points sit in LDS.  The pairwise form
//                     computes the columns >= row and mirrors them.
// pd_shape_overlay  : (workspace: per (row, column, start) 16 + 3 L doubles) one block per (row, column, start) maximises O(move(A, s), B) over rigid motions with the BFGS of
//                     vina_refine.hip at zero torsions (same chart, line search, constants and stopping rules); a second launch picks
//                     the best of the five starts and scores colour there.
//
// Every sum is `block_overlap` (or, with the gradient, `ov_evaluate`): wave w takes the row atoms w, w + 4, ..., its lanes stride the
// column atoms, a butterfly adds the lanes, the wave adds its atoms in ascending order and the four waves are added in order.  No
// atomics; the order depends on (L, M) alone, so results are bit-identical from launch to launch and whatever else is in the batch.
// block_overlap is not inlined: the self-overlap of the preparation and the diagonal of the pairwise form run the same instructions,
// which is what makes that diagonal exactly 1.
#include "common.h"
#include "geom3.h"
#include "physdock_hip.h"

namespace {

constexpr int NT = 256, TILE = 16;
constexpr int SO_MAX_L = 1024, SO_MAX_F = 1024, SO_MAX_N = 65535, SO_MAX_A = 1 << 22;
constexpr int OV_MAX_L = 256, OV_STARTS = 5, OV_REC = 16;
constexpr double SO_PI = 3.14159265358979323846;
constexpr double FUNCTOL = 1e-4, MOVETOL = 1e-7, EPS_ = 3e-8;            // the constants of vina_refine.hip / mmff.hip

// one prepared side: `ws` as pd_shape_prepare left it, the atoms' exponents, the features' kinds
struct Side { const double* ws; const double* alpha; const int* kind; int n, L, F; };
__device__ __host__ __forceinline__ long long side_stride(int L, int F) { return 3ll * (L + F) + 2; }

// a set of Gaussians: centres [n][3], exponents (NULL: all `ca`), kinds (NULL: all pairs overlap)
struct Mol { const double* pts; const double* alpha; const int* kind; int n; };

// the overlap of two Gaussians at squared distance d2; k = a_i a_j / (a_i + a_j), the exponent's factor (the gradient needs it)
__device__ __forceinline__ double gauss_pair(double ai, double aj, double d2, double& k) {
    const double s = ai + aj, q = SO_PI / s;
    k = ai * aj / s;
    return 8.0 * exp(-k * d2) * (q * sqrt(q));
}

// sum over the pairs of a and b, in every thread.  All NT threads; red holds 4 doubles; share [a.n] (or NULL) gets each a atom's part.
__device__ __noinline__ double block_overlap(const Mol a, const Mol b, double ca, double* red, double* share) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc = 0.0;
    for (int i = wave; i < a.n; i += NT / 64) {
        const Vec3 p = load3(a.pts + 3 * i);
        const double ai = a.alpha ? a.alpha[i] : ca;
        const int ki = a.kind ? a.kind[i] : 0;
        double s = 0.0;
        for (int j = lane; j < b.n; j += 64) {
            if (a.kind && b.kind[j] != ki) continue;
            const Vec3 d = sub(p, load3(b.pts + 3 * j));
            double k;
            s += gauss_pair(ai, b.alpha ? b.alpha[j] : ca, dot(d, d), k);
        }
        s = wave_sum(s);
        if (share && lane == 0) share[i] = s;
        acc += s;                                                        // ascending atoms of this wave
    }
    __syncthreads();                                                     // red is free again
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(NT) void shape_prepare_kernel(const float* __restrict__ x, const int* __restrict__ lig_idx,
                                                           const double* __restrict__ alpha, const int* __restrict__ feat_start,
                                                           const int* __restrict__ feat_atom, const int* __restrict__ feat_kind,
                                                           double ca, double* ws, int A, int L, int F) {
    __shared__ double red[4];
    const int tid = threadIdx.x;
    double* pts = ws + (long long)blockIdx.x * side_stride(L, F);
    double* fp = pts + 3 * L;
    const float* xp = x + (long long)blockIdx.x * A * 3;
    int bad = 0;
    for (int i = tid; i < L; i += NT) {
        const float* v = xp + 3ll * lig_idx[i];
        bad |= !finite3(v[0], v[1], v[2]);
        pts[3 * i] = (double)v[0]; pts[3 * i + 1] = (double)v[1]; pts[3 * i + 2] = (double)v[2];
    }
    bad = __syncthreads_or(bad);                                         // (also publishes pts to the block)
    for (int f = tid; f < F; f += NT) {
        const int q0 = feat_start[f], q1 = feat_start[f + 1];
        double sx = 0.0, sy = 0.0, sz = 0.0;
        for (int q = q0; q < q1; ++q) {
            const int i = feat_atom[q];
            sx += pts[3 * i]; sy += pts[3 * i + 1]; sz += pts[3 * i + 2];
        }
        const double n = (double)(q1 - q0);
        fp[3 * f] = sx / n; fp[3 * f + 1] = sy / n; fp[3 * f + 2] = sz / n;
    }
    __syncthreads();
    const double o = block_overlap({pts, alpha, nullptr, L}, {pts, alpha, nullptr, L}, ca, red, nullptr);
    const double c = block_overlap({fp, nullptr, feat_kind, F}, {fp, nullptr, feat_kind, F}, ca, red, nullptr);
    if (tid == 0) {
        fp[3 * F] = bad ? nan("") : o;
        fp[3 * F + 1] = bad ? nan("") : c;
    }
}

struct Scores { double st, ct, combo; };
__device__ __forceinline__ Scores tanimoto(double o, double c, const double* sa, const double* sb) {
    if (isnan(sa[0]) || isnan(sb[0])) return {nan(""), nan(""), nan("")};
    const double st = o / (sa[0] + sb[0] - o), dc = sa[1] + sb[1] - c;
    const double ct = dc > 0.0 ? c / dc : 0.0;
    return {st, ct, st + ct};
}

struct OverlapOut { double *o_ab, *c_ab; float *st, *ct, *combo; };
__device__ __forceinline__ void write_pair(const OverlapOut& w, long long e, double o, double c, const double* sa, const double* sb) {
    const Scores s = tanimoto(o, c, sa, sb);
    const bool bad = isnan(s.st);
    if (w.o_ab) w.o_ab[e] = bad ? s.st : o;
    if (w.c_ab) w.c_ab[e] = bad ? s.st : c;
    if (w.st) w.st[e] = (float)s.st;
    if (w.ct) w.ct[e] = (float)s.ct;
    if (w.combo) w.combo[e] = (float)s.combo;
}

__global__ __launch_bounds__(NT) void shape_overlap_kernel(const Side a, const Side b, double ca, int pairwise, const OverlapOut w,
                                                           double* __restrict__ share) {
    extern __shared__ double sm[];
    __shared__ double red[4];
    const int tid = threadIdx.x, row = blockIdx.y, c0 = blockIdx.x * TILE;
    if (pairwise && c0 + TILE <= row) return;                            // every column of the tile lies below the diagonal
    const long long sa = side_stride(a.L, a.F), sb = side_stride(b.L, b.F);
    const double* ra = a.ws + row * sa;
    for (int i = tid; i < 3 * (a.L + a.F); i += NT) sm[i] = ra[i];
    __syncthreads();
    const double* self_a = ra + 3 * (a.L + a.F);
    const int c1 = min(c0 + TILE, b.n);
    for (int col = c0; col < c1; ++col) {
        if (pairwise && col < row) continue;
        const double* rb = b.ws + col * sb;
        const double o = block_overlap({sm, a.alpha, nullptr, a.L}, {rb, b.alpha, nullptr, b.L}, ca, red, share ? share + (long long)row * a.L : nullptr);
        const double c = block_overlap({sm + 3 * a.L, nullptr, a.kind, a.F}, {rb + 3 * b.L, nullptr, b.kind, b.F}, ca, red, nullptr);
        const double* self_b = rb + 3 * (b.L + b.F);
        if (share && (isnan(self_a[0]) || isnan(self_b[0])))             // a NaN structure: its whole row of shares (after block_overlap's barriers)
            for (int i = tid; i < a.L; i += NT) share[(long long)row * a.L + i] = nan("");
        if (tid == 0) {
            write_pair(w, (long long)row * b.n + col, o, c, self_a, self_b);
            if (pairwise && col != row) write_pair(w, (long long)col * b.n + row, o, c, self_b, self_a);
        }
    }
}

// ------------------------------------------------------------------ the overlay
// O(y, B) in every thread; gy (LDS) = dE/dy of E = -O.  All NT threads with y complete; gy complete on return.
__device__ double ov_evaluate(const double* y, const double* aa, int L, const double* bp, const double* ab, int M, double* gy, double* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc = 0.0;
    for (int i = wave; i < L; i += NT / 64) {
        const Vec3 p = load3(y + 3 * i);
        const double ai = aa[i];
        double e = 0.0, gx = 0.0, gyy = 0.0, gz = 0.0;
        for (int j = lane; j < M; j += 64) {
            const Vec3 d = sub(p, load3(bp + 3 * j));
            double k;
            const double t = gauss_pair(ai, ab[j], dot(d, d), k);
            const double wgt = 2.0 * k * t;
            e += t;
            gx += wgt * d.x; gyy += wgt * d.y; gz += wgt * d.z;
        }
        e = wave_sum(e); gx = wave_sum(gx); gyy = wave_sum(gyy); gz = wave_sum(gz);
        if (lane == 0) { gy[3 * i] = gx; gy[3 * i + 1] = gyy; gy[3 * i + 2] = gz; }
        acc += e;
    }
    __syncthreads();
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// cen[3] (LDS) = the unweighted centroid of y.  All threads; returns after a barrier.
__device__ void ov_centroid(const double* y, int L, double* cen) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave < 3) {
        double s = 0.0;
        for (int i = lane; i < L; i += 64) s += y[3 * i + wave];
        s = wave_sum(s);
        if (lane == 0) cen[wave] = s / (double)L;
    }
    __syncthreads();
}

// gg[6] (LDS) = (sum_i g_i, sum_i (y_i - c) x g_i).  All threads; barrier at the end.
__device__ void ov_generalised(const double* y, const double* gy, int L, double* cen, double* gg) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    ov_centroid(y, L, cen);
    for (int c = wave; c < 6; c += NT / 64) {
        double acc = 0.0;
        if (c < 3) {
            for (int i = lane; i < L; i += 64) acc += gy[3 * i + c];
        } else {
            const int a = (c - 2) % 3, b = (c - 1) % 3;                  // component c - 3 of r x g = r_a g_b - r_b g_a
            const double ca = cen[a], cb = cen[b];
            for (int i = lane; i < L; i += 64) acc += (y[3 * i + a] - ca) * gy[3 * i + b] - (y[3 * i + b] - cb) * gy[3 * i + a];
        }
        acc = wave_sum(acc);
        if (lane == 0) gg[c] = acc;
    }
    __syncthreads();
}

// y (LDS) = move(pos, s): rotation by the vector s[3:6] about the centroid (left in cen when it is not zero), then translation by s[0:3]
__device__ void ov_move(const double* pos, double* y, int L, double* cen, const double* s) {
    const int tid = threadIdx.x;
    for (int i = tid; i < 3 * L; i += NT) y[i] = pos[i];
    __syncthreads();
    const double th = sqrt(s[3] * s[3] + s[4] * s[4] + s[5] * s[5]);
    if (th > 0.0) {                                                      // uniform over the block
        ov_centroid(y, L, cen);
        const double cx = cen[0], cy = cen[1], cz = cen[2];
        const double ux = s[3] / th, uy = s[4] / th, uz = s[5] / th;
        const double sn = sin(th), cs = cos(th);
        for (int i = tid; i < L; i += NT) {
            const double vx = y[3 * i] - cx, vy = y[3 * i + 1] - cy, vz = y[3 * i + 2] - cz;
            const double dt = (vx * ux + vy * uy + vz * uz) * (1.0 - cs);
            y[3 * i] = (cx + ((vx * cs + (uy * vz - uz * vy) * sn) + ux * dt)) + s[0];
            y[3 * i + 1] = (cy + ((vy * cs + (uz * vx - ux * vz) * sn) + uy * dt)) + s[1];
            y[3 * i + 2] = (cz + ((vz * cs + (ux * vy - uy * vx) * sn) + uz * dt)) + s[2];
        }
    } else {
        for (int i = tid; i < L; i += NT) { y[3 * i] += s[0]; y[3 * i + 1] += s[1]; y[3 * i + 2] += s[2]; }
    }
    __syncthreads();
}

// mom (LDS, 9) = the centroid and the six central second moments (xx, yy, zz, xy, xz, yz) / n of pts.  All threads; barrier at the end.
__device__ void ov_moments(const double* pts, int n, double* mom) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    ov_centroid(pts, n, mom);
    for (int c = wave; c < 6; c += NT / 64) {
        const int a = c < 3 ? c : (c == 5 ? 1 : 0), b = c < 3 ? c : (c == 3 ? 1 : 2);
        double acc = 0.0;
        for (int i = lane; i < n; i += 64) acc += (pts[3 * i + a] - mom[a]) * (pts[3 * i + b] - mom[b]);
        acc = wave_sum(acc);
        if (lane == 0) mom[3 + c] = acc / (double)n;
    }
    __syncthreads();
}

// the unit vector that C - lam I annihilates: the largest cross product of two of its rows
__device__ __forceinline__ bool null_vector(const double* m, double lam, Vec3& out) {
    const double r00 = m[0] - lam, r11 = m[1] - lam, r22 = m[2] - lam, c01 = m[3], c02 = m[4], c12 = m[5];
    const Vec3 u = cross({r00, c01, c02}, {c01, r11, c12}), v = cross({r00, c01, c02}, {c02, c12, r22}), w = cross({c01, r11, c12}, {c02, c12, r22});
    const double nu = dot(u, u), nv = dot(v, v), nw = dot(w, w);
    Vec3 n = u;
    double nn = nu;
    if (nv > nn) { n = v; nn = nv; }
    if (nw > nn) { n = w; nn = nw; }
    if (!(nn > 0.0)) return false;
    const double inv = 1.0 / sqrt(nn);
    out = {n.x * inv, n.y * inv, n.z * inv};
    return true;
}

// the sign that makes the largest-magnitude component (the first of equals) positive
__device__ __forceinline__ Vec3 fix_sign(Vec3 v) {
    double big = v.x;
    if (fabs(v.y) > fabs(big)) big = v.y;
    if (fabs(v.z) > fabs(big)) big = v.z;
    return big < 0.0 ? neg(v) : v;
}

// principal axes of the second-moment matrix m (xx, yy, zz, xy, xz, yz), by descending eigenvalue: V[3] right-handed.  false when
// an axis is not determined (fewer than three distinct directions)
__device__ bool principal_axes(const double* m, Vec3* V) {
    double a00 = m[0], a11 = m[1], a22 = m[2], a01 = m[3], a02 = m[4], a12 = m[5];
#pragma unroll 1
    for (int sweep = 0; sweep < 10; ++sweep) {
        jacobi(a00, a11, a01, a02, a12);
        jacobi(a00, a22, a02, a01, a12);
        jacobi(a11, a22, a12, a01, a02);
    }
    const double hi = fmax(a00, fmax(a11, a22)), lo = fmin(a00, fmin(a11, a22)), mid = a00 + a11 + a22 - lo - hi;
    Vec3 v1, v2;
    if (!null_vector(m, hi, v1) || !null_vector(m, mid, v2)) return false;
    const double p = dot(v2, v1);
    v2 = {v2.x - p * v1.x, v2.y - p * v1.y, v2.z - p * v1.z};
    const double n2 = dot(v2, v2);
    if (!(n2 > 0.0)) return false;
    const double inv = 1.0 / sqrt(n2);
    v2 = {v2.x * inv, v2.y * inv, v2.z * inv};
    V[0] = fix_sign(v1); V[1] = fix_sign(v2); V[2] = cross(V[0], V[1]);
    return finite3(V[0]) && finite3(V[1]) && finite3(V[2]);
}

struct OvArgs { int max_iters; double grad_tol, max_step; double* rec; };

// One block per (start, column, row).  rec [n][C][5][OV_REC + 3 L]: O at the end, O at the start, the quaternion, t, iterations,
// evaluations, status, and behind them the fitted atoms [L][3] (not written for a NaN structure).  Every decision is taken by all threads alike from values that are the same in every thread.
__global__ __launch_bounds__(NT) void shape_overlay_kernel(const Side a, const Side b, const OvArgs ar) {
    extern __shared__ double sm[];
    __shared__ double red[4], cen[3], gg[6], ma[9], mb[9];
    const int tid = threadIdx.x, k = blockIdx.x, col = blockIdx.y, row = blockIdx.z, L = a.L, M = b.L;
    double *pos = sm, *y = sm + 3 * L, *gy = sm + 6 * L, *bp = sm + 9 * L, *aa = bp + 3 * M, *ab = aa + L;
    const double* ra = a.ws + row * side_stride(a.L, a.F);
    const double* rb = b.ws + col * side_stride(b.L, b.F);
    double* rec = ar.rec + (((long long)row * b.n + col) * OV_STARTS + k) * (OV_REC + 3ll * L);
    if (isnan(ra[3 * (a.L + a.F)]) || isnan(rb[3 * (b.L + b.F)])) {      // uniform over the block
        if (tid < 12) rec[tid] = tid < 9 ? nan("") : (tid == 11 ? 2.0 : 0.0);
        return;
    }
    for (int i = tid; i < 3 * L; i += NT) pos[i] = ra[i];
    for (int i = tid; i < 3 * M; i += NT) bp[i] = rb[i];
    for (int i = tid; i < L; i += NT) aa[i] = a.alpha[i];
    for (int i = tid; i < M; i += NT) ab[i] = b.alpha[i];
    __syncthreads();
    // ---------------- the start: R [9] row-major and t with x' = R x + t
    double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0};
    if (k < 4) {
        ov_moments(pos, L, ma);
        ov_moments(bp, M, mb);
        Vec3 VA[3], VB[3];
        if (principal_axes(ma + 3, VA) && principal_axes(mb + 3, VB)) {
            const double d[3] = {(k == 0 || k == 1) ? 1.0 : -1.0, (k == 0 || k == 2) ? 1.0 : -1.0, (k == 0 || k == 3) ? 1.0 : -1.0};
            const double va[3][3] = {{VA[0].x, VA[0].y, VA[0].z}, {VA[1].x, VA[1].y, VA[1].z}, {VA[2].x, VA[2].y, VA[2].z}};
            const double vb[3][3] = {{VB[0].x, VB[0].y, VB[0].z}, {VB[1].x, VB[1].y, VB[1].z}, {VB[2].x, VB[2].y, VB[2].z}};
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) R[3 * r + c] = (vb[0][r] * d[0] * va[0][c] + vb[1][r] * d[1] * va[1][c]) + vb[2][r] * d[2] * va[2][c];
        }
        const double cax = ma[0], cay = ma[1], caz = ma[2];
#pragma unroll
        for (int r = 0; r < 3; ++r) t[r] = mb[r] - ((R[3 * r] * cax + R[3 * r + 1] * cay) + R[3 * r + 2] * caz);
        for (int i = tid; i < L; i += NT) {
            const double vx = pos[3 * i] - cax, vy = pos[3 * i + 1] - cay, vz = pos[3 * i + 2] - caz;
            y[3 * i] = mb[0] + ((R[0] * vx + R[1] * vy) + R[2] * vz);
            y[3 * i + 1] = mb[1] + ((R[3] * vx + R[4] * vy) + R[5] * vz);
            y[3 * i + 2] = mb[2] + ((R[6] * vx + R[7] * vy) + R[8] * vz);
        }
        __syncthreads();
        for (int i = tid; i < 3 * L; i += NT) pos[i] = y[i];
    } else {
        for (int i = tid; i < 3 * L; i += NT) y[i] = pos[i];
    }
    __syncthreads();
    // ---------------- the BFGS of vina_refine.hip in six coordinates, every thread holding all of them
    double g[6], xi[6], H[36];
#pragma unroll
    for (int e = 0; e < 36; ++e) H[e] = (e / 6 == e % 6) ? 1.0 : 0.0;
    double fp = -ov_evaluate(y, aa, L, bp, ab, M, gy, red);
    ov_generalised(y, gy, L, cen, gg);
    double gmax = 0.0;
#pragma unroll
    for (int c = 0; c < 6; ++c) { g[c] = gg[c]; xi[c] = -g[c]; gmax = fmax(gmax, fabs(g[c])); }
    const double f0 = fp;
    int it = 0, nev = 1, st = 1;
    if (gmax < ar.grad_tol) st = 0;
    while (st == 1 && it < ar.max_iters) {
        double s2 = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) s2 += xi[c] * xi[c];
        const double s = sqrt(s2);
        if (s > ar.max_step) {
#pragma unroll
            for (int c = 0; c < 6; ++c) xi[c] *= ar.max_step / s;
        }
        double slope = 0.0, ximax = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) { slope += xi[c] * g[c]; ximax = fmax(ximax, fabs(xi[c])); }
        if (!(slope < 0.0)) { st = 2; break; }
        const double lam_min = MOVETOL / ximax;
        double lam = 1.0, lam2 = 0.0, val2 = 0.0, fnew = fp, step[6];
        bool ok = false;
        for (int ls = 0; ls < 1000; ++ls) {
            if (lam < lam_min) break;
#pragma unroll
            for (int c = 0; c < 6; ++c) step[c] = lam * xi[c];
            ov_move(pos, y, L, cen, step);
            fnew = -ov_evaluate(y, aa, L, bp, ab, M, gy, red);
            ++nev;
            if (fnew - fp <= FUNCTOL * lam * slope) { ok = true; break; }
            double tmp;
            if (ls == 0) tmp = -slope / (2.0 * (fnew - fp - slope));
            else {
                const double rhs1 = fnew - fp - lam * slope, rhs2 = val2 - fp - lam2 * slope;
                const double qa = (rhs1 / (lam * lam) - rhs2 / (lam2 * lam2)) / (lam - lam2);
                const double qb = (-lam2 * rhs1 / (lam * lam) + lam * rhs2 / (lam2 * lam2)) / (lam - lam2);
                if (qa == 0.0) tmp = -slope / (2.0 * qb);
                else {
                    const double disc = qb * qb - 3.0 * qa * slope;
                    if (disc < 0.0) tmp = 0.5 * lam;
                    else if (qb <= 0.0) tmp = (-qb + sqrt(disc)) / (3.0 * qa);
                    else tmp = -slope / (qb + sqrt(disc));
                }
                if (tmp > 0.5 * lam) tmp = 0.5 * lam;
            }
            lam2 = lam; val2 = fnew;
            lam = fmax(tmp, 0.1 * lam);
        }
        if (!ok) { st = 2; break; }                                     // "nothing was done": the accepted point stays
        // ---------------- accepted: the transform takes the step (cen is still the centroid the rotation turned about)
        {
            const double th = sqrt(step[3] * step[3] + step[4] * step[4] + step[5] * step[5]);
            if (th > 0.0) {
                const double ux = step[3] / th, uy = step[4] / th, uz = step[5] / th, sn = sin(th), cs = cos(th), oc = 1.0 - cs;
                const double Q[9] = {cs + ux * ux * oc, ux * uy * oc - uz * sn, ux * uz * oc + uy * sn,
                                     uy * ux * oc + uz * sn, cs + uy * uy * oc, uy * uz * oc - ux * sn,
                                     uz * ux * oc - uy * sn, uz * uy * oc + ux * sn, cs + uz * uz * oc};
                const double cc[3] = {cen[0], cen[1], cen[2]};
                double Rn[9], tn[3];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) Rn[3 * r + c] = (Q[3 * r] * R[c] + Q[3 * r + 1] * R[3 + c]) + Q[3 * r + 2] * R[6 + c];
                    tn[r] = (cc[r] + ((Q[3 * r] * (t[0] - cc[0]) + Q[3 * r + 1] * (t[1] - cc[1])) + Q[3 * r + 2] * (t[2] - cc[2]))) + step[r];
                }
#pragma unroll
                for (int e = 0; e < 9; ++e) R[e] = Rn[e];
#pragma unroll
                for (int r = 0; r < 3; ++r) t[r] = tn[r];
            } else {
#pragma unroll
                for (int r = 0; r < 3; ++r) t[r] += step[r];
            }
        }
        __syncthreads();                                                 // cen is read before the next centroid overwrites it
        for (int i = tid; i < 3 * L; i += NT) pos[i] = y[i];
        fp = fnew;
        ++it;
        double g_old[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) g_old[c] = g[c];
        ov_generalised(y, gy, L, cen, gg);                               // (its barriers also publish pos)
        gmax = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) { g[c] = gg[c]; gmax = fmax(gmax, fabs(g[c])); }
        if (gmax < ar.grad_tol) { st = 0; break; }
        // ---------------- BFGS update of the inverse Hessian
        double dg[6], hdg[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) dg[c] = g[c] - g_old[c];
        double fac = 0.0, fae = 0.0, sdg = 0.0, sxi = 0.0;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            double h = 0.0;
#pragma unroll
            for (int c = 0; c < 6; ++c) h += H[6 * r + c] * dg[c];
            hdg[r] = h;
        }
#pragma unroll
        for (int c = 0; c < 6; ++c) { fac += dg[c] * step[c]; fae += dg[c] * hdg[c]; sdg += dg[c] * dg[c]; sxi += step[c] * step[c]; }
        if (fac > sqrt(EPS_ * sdg * sxi)) {
            fac = 1.0 / fac;
            const double fad = 1.0 / fae;
            double v[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) v[c] = fac * step[c] - fad * hdg[c];
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = r; c < 6; ++c) {
                    const double h = H[6 * r + c] + ((fac * step[r]) * step[c] - (fad * hdg[r]) * hdg[c] + (fae * v[r]) * v[c]);
                    H[6 * r + c] = h; H[6 * c + r] = h;                   // kept exactly symmetric
                }
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            double h = 0.0;
#pragma unroll
            for (int c = 0; c < 6; ++c) h += H[6 * r + c] * g[c];
            xi[r] = -h;
        }
    }
    for (int i = tid; i < 3 * L; i += NT) rec[OV_REC + i] = pos[i];      // each thread reads what it wrote
    if (tid == 0) {
        // the unit quaternion of R with w >= 0 (Shepperd's branches)
        const double tr = R[0] + R[4] + R[8];
        double q[4];
        if (tr > 0.0) {
            const double s = 2.0 * sqrt(tr + 1.0);
            q[0] = 0.25 * s; q[1] = (R[7] - R[5]) / s; q[2] = (R[2] - R[6]) / s; q[3] = (R[3] - R[1]) / s;
        } else if (R[0] > R[4] && R[0] > R[8]) {
            const double s = 2.0 * sqrt(1.0 + R[0] - R[4] - R[8]);
            q[0] = (R[7] - R[5]) / s; q[1] = 0.25 * s; q[2] = (R[1] + R[3]) / s; q[3] = (R[2] + R[6]) / s;
        } else if (R[4] > R[8]) {
            const double s = 2.0 * sqrt(1.0 + R[4] - R[0] - R[8]);
            q[0] = (R[2] - R[6]) / s; q[1] = (R[1] + R[3]) / s; q[2] = 0.25 * s; q[3] = (R[5] + R[7]) / s;
        } else {
            const double s = 2.0 * sqrt(1.0 + R[8] - R[0] - R[4]);
            q[0] = (R[3] - R[1]) / s; q[1] = (R[2] + R[6]) / s; q[2] = (R[5] + R[7]) / s; q[3] = 0.25 * s;
        }
        const double qn = (q[0] < 0.0 ? -1.0 : 1.0) / sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
        rec[0] = -fp; rec[1] = -f0;
        rec[2] = q[0] * qn; rec[3] = q[1] * qn; rec[4] = q[2] * qn; rec[5] = q[3] * qn;
        rec[6] = t[0]; rec[7] = t[1]; rec[8] = t[2];
        rec[9] = (double)it; rec[10] = (double)nev; rec[11] = (double)st;
    }
}

struct OverlayOut { double* transform; double* x_fit; float* scores; double *overlap, *overlap_start; int *best_start, *iterations, *evaluations, *status; };

// One block per (column, row): the start with the largest overlap (the lowest index on a tie) and the colour overlap under its transform
__global__ __launch_bounds__(NT) void shape_overlay_select_kernel(const Side a, const Side b, double ca, const double* __restrict__ rec_all,
                                                                  const OverlayOut w) {
    extern __shared__ double sm[];
    __shared__ double red[4];
    const int tid = threadIdx.x, col = blockIdx.x, row = blockIdx.y;
    const long long e = (long long)row * b.n + col;
    const long long rs = OV_REC + 3ll * a.L;                              // one start's record
    const double* rec = rec_all + e * OV_STARTS * rs;
    int best = 0;
    double o = rec[0];
    for (int k = 1; k < OV_STARTS; ++k) {                                // every thread alike
        const double v = rec[k * rs];
        if (v > o) { o = v; best = k; }
    }
    const double* r = rec + best * rs;
    const double qw = r[2], qx = r[3], qy = r[4], qz = r[5];
    const double R[9] = {1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy),
                         2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx),
                         2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)};
    const double* ra = a.ws + row * side_stride(a.L, a.F);
    const double* rb = b.ws + col * side_stride(b.L, b.F);
    const double* fa = ra + 3 * a.L;
    for (int f = tid; f < a.F; f += NT) {
        const double vx = fa[3 * f], vy = fa[3 * f + 1], vz = fa[3 * f + 2];
        sm[3 * f] = ((R[0] * vx + R[1] * vy) + R[2] * vz) + r[6];
        sm[3 * f + 1] = ((R[3] * vx + R[4] * vy) + R[5] * vz) + r[7];
        sm[3 * f + 2] = ((R[6] * vx + R[7] * vy) + R[8] * vz) + r[8];
    }
    __syncthreads();
    const double c = block_overlap({sm, nullptr, a.kind, a.F}, {rb + 3 * b.L, nullptr, b.kind, b.F}, ca, red, nullptr);
    if (w.x_fit) {
        const bool bad = isnan(o);
        for (int i = tid; i < 3 * a.L; i += NT) w.x_fit[e * 3 * a.L + i] = bad ? nan("") : r[OV_REC + i];
    }
    if (tid == 0) {
        const Scores s = tanimoto(o, c, ra + 3 * (a.L + a.F), rb + 3 * (b.L + b.F));
        for (int i = 0; i < 7; ++i) w.transform[e * 7 + i] = r[2 + i];
        w.scores[e * 3] = (float)s.st; w.scores[e * 3 + 1] = (float)s.ct; w.scores[e * 3 + 2] = (float)s.combo;
        w.overlap[e] = o;
        w.overlap_start[e] = rec[4 * rs + 1];
        w.best_start[e] = best;
        w.iterations[e] = (int)r[9]; w.evaluations[e] = (int)r[10]; w.status[e] = (int)r[11];
    }
}

bool aligned(const void* q, uintptr_t a) { return ((uintptr_t)q & (a - 1)) == 0; }

// PD_OK, or the code two prepared sides earn
int check_sides(const double* ws_a, long long ws_a_numel, const double* alpha_a, const int* kind_a, int n, int L, int Fa, const double* ws_b,
                long long ws_b_numel, const double* alpha_b, const int* kind_b, int C, int M, int Fb, double color_alpha, int max_l) {
    if (!ws_a || !ws_b || !alpha_a || !alpha_b) return PD_ERR_ARG;
    if (n <= 0 || C <= 0 || L <= 0 || M <= 0 || Fa < 0 || Fb < 0 || !(color_alpha > 0.0)) return PD_ERR_ARG;
    if ((Fa > 0 && !kind_a) || (Fb > 0 && !kind_b)) return PD_ERR_ARG;
    if (!aligned(ws_a, 8) || !aligned(ws_b, 8) || !aligned(alpha_a, 8) || !aligned(alpha_b, 8) || !aligned(kind_a, 4) || !aligned(kind_b, 4))
        return PD_ERR_ARG;
    if (L > max_l || M > max_l || Fa > SO_MAX_F || Fb > SO_MAX_F || n > SO_MAX_N || C > SO_MAX_N) return PD_ERR_UNSUPPORTED;
    if (ws_a_numel < n * side_stride(L, Fa) || ws_b_numel < C * side_stride(M, Fb)) return PD_ERR_ARG;
    return PD_OK;
}

}  // namespace

PD_EXPORT long long pd_shape_workspace_numel(int n, int L, int F) {
    if (n <= 0 || L <= 0 || F < 0) return PD_ERR_ARG;
    if (L > SO_MAX_L || F > SO_MAX_F || n > SO_MAX_N) return PD_ERR_UNSUPPORTED;
    return n * side_stride(L, F);
}

PD_EXPORT int pd_shape_prepare(const float* x, const int* lig_idx, const double* alpha, const int* feat_start, const int* feat_atom,
                               const int* feat_kind, double color_alpha, double* ws, long long ws_numel, int n, int A, int L, int F,
                               void* stream) {
    if (!x || !lig_idx || !alpha || !ws) return PD_ERR_ARG;
    if (n <= 0 || A <= 0 || L <= 0 || F < 0 || !(color_alpha > 0.0)) return PD_ERR_ARG;
    if (F > 0 && (!feat_start || !feat_atom || !feat_kind)) return PD_ERR_ARG;
    if (!aligned(x, 4) || !aligned(lig_idx, 4) || !aligned(alpha, 8) || !aligned(feat_start, 4) || !aligned(feat_atom, 4) ||
        !aligned(feat_kind, 4) || !aligned(ws, 8))
        return PD_ERR_ARG;
    if (L > SO_MAX_L || F > SO_MAX_F || n > SO_MAX_N || A > SO_MAX_A) return PD_ERR_UNSUPPORTED;
    if (ws_numel < n * side_stride(L, F)) return PD_ERR_ARG;
    hipLaunchKernelGGL(shape_prepare_kernel, dim3(n), dim3(NT), 0, (hipStream_t)stream, x, lig_idx, alpha, feat_start, feat_atom, feat_kind,
                       color_alpha, ws, A, L, F);
    return pd_check_launch();
}

PD_EXPORT int pd_shape_overlap(const double* ws_a, long long ws_a_numel, const double* alpha_a, const int* kind_a, int n, int L, int Fa,
                               const double* ws_b, long long ws_b_numel, const double* alpha_b, const int* kind_b, int C, int M, int Fb,
                               double color_alpha, int pairwise, double* o_ab, double* c_ab, float* shape_tanimoto, float* color_tanimoto,
                               float* combo, double* atom_share, void* stream) {
    const int rc = check_sides(ws_a, ws_a_numel, alpha_a, kind_a, n, L, Fa, ws_b, ws_b_numel, alpha_b, kind_b, C, M, Fb, color_alpha, SO_MAX_L);
    if (rc != PD_OK) return rc;
    if (!aligned(o_ab, 8) || !aligned(c_ab, 8) || !aligned(shape_tanimoto, 4) || !aligned(color_tanimoto, 4) || !aligned(combo, 4) ||
        !aligned(atom_share, 8))
        return PD_ERR_ARG;
    if (pairwise && (ws_a != ws_b || alpha_a != alpha_b || kind_a != kind_b || n != C || L != M || Fa != Fb)) return PD_ERR_ARG;
    if (atom_share && (C != 1 || pairwise)) return PD_ERR_ARG;
    const Side a = {ws_a, alpha_a, kind_a, n, L, Fa}, b = {ws_b, alpha_b, kind_b, C, M, Fb};
    const OverlapOut w = {o_ab, c_ab, shape_tanimoto, color_tanimoto, combo};
    hipLaunchKernelGGL(shape_overlap_kernel, dim3((C + TILE - 1) / TILE, n), dim3(NT), 3 * (size_t)(L + Fa) * sizeof(double),
                       (hipStream_t)stream, a, b, color_alpha, pairwise ? 1 : 0, w, atom_share);
    return pd_check_launch();
}

PD_EXPORT long long pd_shape_overlay_workspace_numel(int n, int C, int L) {
    if (n <= 0 || C <= 0 || L <= 0) return PD_ERR_ARG;
    if (n > SO_MAX_N || C > SO_MAX_N || L > OV_MAX_L) return PD_ERR_UNSUPPORTED;
    return (long long)n * C * OV_STARTS * (OV_REC + 3ll * L);
}

PD_EXPORT int pd_shape_overlay(const double* ws_a, long long ws_a_numel, const double* alpha_a, const int* kind_a, int n, int L, int Fa,
                               const double* ws_b, long long ws_b_numel, const double* alpha_b, const int* kind_b, int C, int M, int Fb,
                               double color_alpha, int max_iters, double grad_tol, double max_step, double* ws, long long ws_numel,
                               double* transform, double* x_fit, float* scores, double* overlap, double* overlap_start, int* best_start,
                               int* iterations, int* evaluations, int* status, void* stream) {
    const int rc = check_sides(ws_a, ws_a_numel, alpha_a, kind_a, n, L, Fa, ws_b, ws_b_numel, alpha_b, kind_b, C, M, Fb, color_alpha, OV_MAX_L);
    if (rc != PD_OK) return rc;
    if (!ws || !transform || !scores || !overlap || !overlap_start || !best_start || !iterations || !evaluations || !status) return PD_ERR_ARG;
    if (max_iters < 0 || !(grad_tol >= 0.0) || !(max_step > 0.0)) return PD_ERR_ARG;
    if (!aligned(ws, 8) || !aligned(transform, 8) || !aligned(x_fit, 8) || !aligned(scores, 4) || !aligned(overlap, 8) || !aligned(overlap_start, 8) ||
        !aligned(best_start, 4) || !aligned(iterations, 4) || !aligned(evaluations, 4) || !aligned(status, 4))
        return PD_ERR_ARG;
    if (ws_numel < pd_shape_overlay_workspace_numel(n, C, L)) return PD_ERR_ARG;
    const Side a = {ws_a, alpha_a, kind_a, n, L, Fa}, b = {ws_b, alpha_b, kind_b, C, M, Fb};
    const OvArgs ar = {max_iters, grad_tol, max_step, ws};
    hipLaunchKernelGGL(shape_overlay_kernel, dim3(OV_STARTS, C, n), dim3(NT), (size_t)(10 * L + 4 * M) * sizeof(double), (hipStream_t)stream,
                       a, b, ar);
    int rl = pd_check_launch();
    if (rl != PD_OK) return rl;
    const OverlayOut w = {transform, x_fit, scores, overlap, overlap_start, best_start, iterations, evaluations, status};
    hipLaunchKernelGGL(shape_overlay_select_kernel, dim3(C, n), dim3(NT), 3 * (size_t)(Fa > 0 ? Fa : 1) * sizeof(double), (hipStream_t)stream,
                       a, b, color_alpha, ws, w);
    return pd_check_launch();
}
