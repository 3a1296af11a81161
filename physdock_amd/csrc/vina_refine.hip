// Local refinement of P poses of one ligand in its rigid receptor, the way `vina --local_only` moves a ligand: as a rigid body and
// about its rotatable bonds (physdock_amd/refine.py builds the tables once per system; tests/vina_refine_ref.py is the written
// definition of everything below, in float64 NumPy).  Bond lengths, angles and rings are preserved by construction.
//
// Energy of a ligand conformation y [L][3], float64 throughout:  E = inter + intra.  Both are the pair function of pd_vina_score
// (vina.hip: gauss1, gauss2, repulsion, hydrophobic, hbond with the published weights, X-Score radii from the type byte, pairs with
// r < 8, a pair at r == 0 without force) - inter over (active ligand atom, receptor atom), intra over the ligand's pairs of active
// atoms more than three bonds apart (Vina's rule), which arrive as the neighbour lists intra_start / intra_atom of every atom.  E is
// not divided by 1 + 0.0585 n_rot.
//
// move(y, s), s in R^(6+T): for k = 0 .. T-1 rotate the atoms of M_k (bit mask rot_mask[k]) by s[6+k] about the axis through
// y[a_k] along y[b_k] - y[a_k] (Rodrigues, on the coordinates as they stand); rotate all atoms about their unweighted centroid by
// the rotation vector s[3:6]; translate by s[0:3].  Generalised gradient at s = 0:  g[0:3] = sum_i dE/dy_i,  g[3:6] = sum_i (y_i - c)
// x dE/dy_i,  g[6+k] = sum_{i in M_k} dE/dy_i . (u_k x (y_i - y[a_k])).
//
// Minimiser: the BFGS / lnsrch of mmff.hip (Numerical Recipes dfpmin as RDKit's BFGSOpt codes it, same constants) in these 6 + T
// coordinates, the chart re-centred at s = 0 after every accepted step (so the `pos` of its tests is the zero vector), no gradient
// scaling, the direction cut to |xi|_2 <= max_step before the line search.  It stops on max|g| < grad_tol (status 0), after
// max_iters accepted steps (1), or when the line search finds nothing (2: the accepted point stays).
//
// Mapping: one block of 256 threads per pose, one launch.  Evaluation: wave w takes the ligand atoms w, w + 4, ...; its 64 lanes
// stride the pose's receptor atoms and the atom's intramolecular neighbours, a butterfly adds the lanes, so atom i's gradient and
// the energies are sums in a fixed order - no atomics, bit-identical from run to run, independent of P.  The 6 + T <= 64
// coordinates of the BFGS vectors live one per lane, in every wave alike: dot products are butterflies and need no barrier.  The
// inverse Hessian and the accepted conformation live in the caller's workspace (per pose (6+T)^2 + 3 L doubles), the conformation
// under evaluation and its Cartesian gradient in LDS (6 L doubles).
#include "common.h"
#include "physdock_hip.h"

namespace {

constexpr int NT = 256;
constexpr int VR_MAX_L = 1024, VR_MAX_A = 1 << 22, VR_MAX_T = PD_VINA_REFINE_MAX_TORSIONS;
constexpr double CUTOFF = 8.0;
constexpr double W_GAUSS1 = -0.0356, W_GAUSS2 = -0.00516, W_REPULSION = 0.840, W_HYDROPHOBIC = -0.0351, W_HBOND = -0.587;
constexpr double FUNCTOL = 1e-4, MOVETOL = 1e-7, EPS_ = 3e-8;
static_assert(VR_MAX_T + 6 == 64, "one lane per coordinate");

__device__ const double VR_RADIUS[16] = {1.9, 1.8, 1.7, 2.1, 2.0, 1.5, 1.8, 2.0, 2.2, 1.2, 1.2, 1.2, 1.2, 1.2, 1.2, 1.2};

struct Tab {
    const int* lig_idx; const unsigned char* type; const unsigned char* rec_mask; const unsigned char* lig_active;
    const int* rot; const unsigned* rot_mask; const int* intra_start; const int* intra_atom;
    int A, L, T;
};

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// one pair at distance r: its weighted energy and d energy / d r
__device__ __forceinline__ void pair_energy(double r, double rsum, unsigned ti, unsigned tj, double& e, double& de) {
    const double d = r - rsum;
    const double q1 = d * 2.0, q2 = (d - 3.0) * 0.5;
    const double g1 = exp(-(q1 * q1)), g2 = exp(-(q2 * q2));
    e = W_GAUSS1 * g1 + W_GAUSS2 * g2;
    de = W_GAUSS1 * (-4.0 * q1 * g1) + W_GAUSS2 * (-q2 * g2);
    if (d < 0.0) {
        e += W_REPULSION * (d * d);
        de += W_REPULSION * (2.0 * d);
    }
    if (ti & tj & 16u) {
        if (d <= 0.5) {
            e += W_HYDROPHOBIC;
        } else if (d < 1.5) {
            e += W_HYDROPHOBIC * (1.5 - d);
            de -= W_HYDROPHOBIC;
        }
    }
    if (((ti & 32u) && (tj & 64u)) || ((ti & 64u) && (tj & 32u))) {
        if (d <= -0.7) {
            e += W_HBOND;
        } else if (d < 0.0) {
            e += W_HBOND * (-d / 0.7);
            de -= W_HBOND / 0.7;
        }
    }
}

// E of the conformation y (LDS) against the receptor rows of xp; the Cartesian gradient goes to gy (LDS, zeros for an inactive
// atom).  Called by all NT threads with y complete; returns with gy complete and (inter, intra) in every thread.
__device__ void evaluate(const Tab& t, const float* __restrict__ xp, const double* y, double* gy, double* red, double& inter,
                         double& intra) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double e_inter = 0.0, e_intra = 0.0;
    for (int i = wave; i < t.L; i += NT / 64) {
        double ei = 0.0, ea = 0.0, gx = 0.0, gyy = 0.0, gz = 0.0;
        if (t.lig_active[i]) {                                           // uniform over the wave
            const double ax = y[3 * i], ay = y[3 * i + 1], az = y[3 * i + 2];
            const unsigned ti = t.type[t.lig_idx[i]];
            const double ri = VR_RADIUS[ti & 15];
            for (int j = lane; j < t.A; j += 64) {
                if (!t.rec_mask[j]) continue;
                const double dx = ax - (double)xp[3 * j], dy = ay - (double)xp[3 * j + 1], dz = az - (double)xp[3 * j + 2];
                const double r = sqrt(dx * dx + dy * dy + dz * dz);
                if (!(r < CUTOFF)) continue;
                const unsigned tj = t.type[j];
                double e, de;
                pair_energy(r, ri + VR_RADIUS[tj & 15], ti, tj, e, de);
                ei += e;
                if (r > 0.0) {
                    const double s = de / r;
                    gx += s * dx; gyy += s * dy; gz += s * dz;
                }
            }
            for (int q = t.intra_start[i] + lane; q < t.intra_start[i + 1]; q += 64) {
                const int j = t.intra_atom[q];
                const double dx = ax - y[3 * j], dy = ay - y[3 * j + 1], dz = az - y[3 * j + 2];
                const double r = sqrt(dx * dx + dy * dy + dz * dz);
                if (!(r < CUTOFF)) continue;
                const unsigned tj = t.type[t.lig_idx[j]];
                double e, de;
                pair_energy(r, ri + VR_RADIUS[tj & 15], ti, tj, e, de);
                if (j > i) ea += e;                                      // a pair is met from both of its atoms
                if (r > 0.0) {
                    const double s = de / r;
                    gx += s * dx; gyy += s * dy; gz += s * dz;
                }
            }
        }
        ei = wave_sum_d(ei); ea = wave_sum_d(ea);
        gx = wave_sum_d(gx); gyy = wave_sum_d(gyy); gz = wave_sum_d(gz);
        if (lane == 0) { gy[3 * i] = gx; gy[3 * i + 1] = gyy; gy[3 * i + 2] = gz; }
        e_inter += ei; e_intra += ea;                                   // ascending atoms of this wave
    }
    __syncthreads();                                                     // red is free again
    if (lane == 0) { red[wave] = e_inter; red[4 + wave] = e_intra; }
    __syncthreads();
    inter = ((red[0] + red[1]) + red[2]) + red[3];
    intra = ((red[4] + red[5]) + red[6]) + red[7];
}

// cen[3] (LDS) = the unweighted centroid of y.  All threads; returns after a barrier.
__device__ void centroid(const double* y, int L, double* cen) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave < 3) {
        double s = 0.0;
        for (int i = lane; i < L; i += 64) s += y[3 * i + wave];
        s = wave_sum_d(s);
        if (lane == 0) cen[wave] = s / (double)L;
    }
    __syncthreads();
}

// gg[6 + T] (LDS) = the generalised gradient of the conformation y with the Cartesian gradient gy.  All threads; barrier at the end.
__device__ void generalised(const Tab& t, const double* y, const double* gy, double* cen, double* gg) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, L = t.L, W = (L + 31) >> 5;
    centroid(y, L, cen);
    const double cx = cen[0], cy = cen[1], cz = cen[2];
    for (int c = wave; c < 6 + t.T; c += NT / 64) {
        double acc = 0.0;
        if (c < 3) {
            for (int i = lane; i < L; i += 64) acc += gy[3 * i + c];
        } else if (c < 6) {
            const int a = (c - 2) % 3, b = (c - 1) % 3;                  // component c - 3 of r x g = r_a g_b - r_b g_a
            const double ca = a == 0 ? cx : (a == 1 ? cy : cz), cb = b == 0 ? cx : (b == 1 ? cy : cz);
            for (int i = lane; i < L; i += 64) acc += (y[3 * i + a] - ca) * gy[3 * i + b] - (y[3 * i + b] - cb) * gy[3 * i + a];
        } else {
            const int k = c - 6, a = t.rot[2 * k], b = t.rot[2 * k + 1];
            const double ax = y[3 * a], ay = y[3 * a + 1], az = y[3 * a + 2];
            double ux = y[3 * b] - ax, uy = y[3 * b + 1] - ay, uz = y[3 * b + 2] - az;
            const double n = sqrt(ux * ux + uy * uy + uz * uz);
            ux /= n; uy /= n; uz /= n;
            for (int i = lane; i < L; i += 64) {
                if (!((t.rot_mask[k * W + (i >> 5)] >> (i & 31)) & 1u)) continue;
                const double vx = y[3 * i] - ax, vy = y[3 * i + 1] - ay, vz = y[3 * i + 2] - az;
                acc += gy[3 * i] * (uy * vz - uz * vy) + gy[3 * i + 1] * (uz * vx - ux * vz) + gy[3 * i + 2] * (ux * vy - uy * vx);
            }
        }
        acc = wave_sum_d(acc);
        if (lane == 0) gg[c] = acc;
    }
    __syncthreads();
}

// y (LDS) = move(pos, lam * xi); xi is this lane's coordinate of the direction (the same in every wave).  All threads; y complete on return.
__device__ void move(const Tab& t, const double* __restrict__ pos, double* y, double* cen, double lam, double xi) {
    const int tid = threadIdx.x, L = t.L, W = (L + 31) >> 5;
    for (int i = tid; i < 3 * L; i += NT) y[i] = pos[i];
    __syncthreads();
    for (int k = 0; k < t.T; ++k) {
        const double th = lam * __shfl(xi, 6 + k);
        const int a = t.rot[2 * k], b = t.rot[2 * k + 1];
        const double ax = y[3 * a], ay = y[3 * a + 1], az = y[3 * a + 2];
        double ux = y[3 * b] - ax, uy = y[3 * b + 1] - ay, uz = y[3 * b + 2] - az;
        __syncthreads();                                                 // the axis is read before b moves
        const double n = sqrt(ux * ux + uy * uy + uz * uz);
        ux /= n; uy /= n; uz /= n;
        const double sn = sin(th), cs = cos(th);
        for (int i = tid; i < L; i += NT) {
            if (!((t.rot_mask[k * W + (i >> 5)] >> (i & 31)) & 1u)) continue;
            const double vx = y[3 * i] - ax, vy = y[3 * i + 1] - ay, vz = y[3 * i + 2] - az;
            const double dt = (vx * ux + vy * uy + vz * uz) * (1.0 - cs);
            y[3 * i] = ax + ((vx * cs + (uy * vz - uz * vy) * sn) + ux * dt);
            y[3 * i + 1] = ay + ((vy * cs + (uz * vx - ux * vz) * sn) + uy * dt);
            y[3 * i + 2] = az + ((vz * cs + (ux * vy - uy * vx) * sn) + uz * dt);
        }
        __syncthreads();
    }
    const double tx = lam * __shfl(xi, 0), ty = lam * __shfl(xi, 1), tz = lam * __shfl(xi, 2);
    const double wx = lam * __shfl(xi, 3), wy = lam * __shfl(xi, 4), wz = lam * __shfl(xi, 5);
    const double th = sqrt(wx * wx + wy * wy + wz * wz);
    if (th > 0.0) {                                                      // uniform over the block
        centroid(y, L, cen);
        const double cx = cen[0], cy = cen[1], cz = cen[2];
        const double ux = wx / th, uy = wy / th, uz = wz / th;
        const double sn = sin(th), cs = cos(th);
        for (int i = tid; i < L; i += NT) {
            const double vx = y[3 * i] - cx, vy = y[3 * i + 1] - cy, vz = y[3 * i + 2] - cz;
            const double dt = (vx * ux + vy * uy + vz * uz) * (1.0 - cs);
            y[3 * i] = (cx + ((vx * cs + (uy * vz - uz * vy) * sn) + ux * dt)) + tx;
            y[3 * i + 1] = (cy + ((vy * cs + (uz * vx - ux * vz) * sn) + uy * dt)) + ty;
            y[3 * i + 2] = (cz + ((vz * cs + (ux * vy - uy * vx) * sn) + uz * dt)) + tz;
        }
    } else {
        for (int i = tid; i < L; i += NT) { y[3 * i] += tx; y[3 * i + 1] += ty; y[3 * i + 2] += tz; }
    }
    __syncthreads();
}

__global__ __launch_bounds__(NT) void vina_refine_energy_kernel(const Tab t, const float* __restrict__ x, double* __restrict__ energy,
                                                                double* __restrict__ inter, double* __restrict__ intra,
                                                                double* __restrict__ grad, double* __restrict__ ggrad) {
    extern __shared__ double sm[];
    __shared__ double red[8], cen[3], gg[64];
    const int tid = threadIdx.x, p = blockIdx.x, L = t.L;
    double* y = sm;
    double* gy = sm + 3 * L;
    const float* xp = x + (long long)p * t.A * 3;
    for (int i = tid; i < 3 * L; i += NT) y[i] = (double)xp[3 * t.lig_idx[i / 3] + i % 3];
    __syncthreads();
    double ei, ea;
    evaluate(t, xp, y, gy, red, ei, ea);
    if (tid == 0) {
        if (energy) energy[p] = ei + ea;
        if (inter) inter[p] = ei;
        if (intra) intra[p] = ea;
    }
    if (grad)
        for (int i = tid; i < 3 * L; i += NT) grad[(long long)p * 3 * L + i] = gy[i];
    if (ggrad) {
        generalised(t, y, gy, cen, gg);
        if (tid < 6 + t.T) ggrad[(long long)p * (6 + t.T) + tid] = gg[tid];
    }
}

__global__ __launch_bounds__(NT) void vina_refine_kernel(const Tab t, const float* __restrict__ x, float* __restrict__ x_out,
                                                         double* __restrict__ ws, int max_iters, double grad_tol, double max_step,
                                                         double* __restrict__ e_start, double* __restrict__ e_end,
                                                         int* __restrict__ iterations, int* __restrict__ evaluations,
                                                         int* __restrict__ status, double* __restrict__ moved,
                                                         double* __restrict__ trace) {
    extern __shared__ double sm[];
    __shared__ double red[8], cen[3], gg[64], sx[64], sh[64], sv[64];
    const int tid = threadIdx.x, lane = tid & 63, p = blockIdx.x, L = t.L, A = t.A, n = 6 + t.T;
    double* y = sm;
    double* gy = sm + 3 * L;
    double* H = ws + (long long)p * ((long long)n * n + 3ll * L);         // inverse Hessian [n][n], kept exactly symmetric
    double* pos = H + n * n;                                             // the accepted conformation [L][3]
    const float* xp = x + (long long)p * A * 3;
    float* ob = x_out + (long long)p * A * 3;
    for (int i = tid; i < 3 * A; i += NT) ob[i] = xp[i];
    for (int i = tid; i < 3 * L; i += NT) {
        const double v = (double)xp[3 * t.lig_idx[i / 3] + i % 3];
        pos[i] = v; y[i] = v;
    }
    for (int e = tid; e < n * n; e += NT) H[e] = (e / n == e % n) ? 1.0 : 0.0;
    __syncthreads();
    double ei, ea;
    evaluate(t, xp, y, gy, red, ei, ea);
    double fp = ei + ea;
    generalised(t, y, gy, cen, gg);
    double g = lane < n ? gg[lane] : 0.0;                                // this lane's coordinate, the same in every wave
    double xi = -g;
    const double f0 = fp;
    int it = 0, nev = 1, st = 1;
    if (trace && tid == 0) trace[(long long)p * (max_iters + 1)] = fp;
    if (wave_max_d(fabs(g)) < grad_tol) st = 0;
    while (st == 1 && it < max_iters) {
        // ---------------- the line search (Numerical Recipes lnsrch)
        const double s = sqrt(wave_sum_d(xi * xi));
        if (s > max_step) xi *= max_step / s;
        const double slope = wave_sum_d(xi * g);
        if (!(slope < 0.0)) { st = 2; break; }
        const double lam_min = MOVETOL / wave_max_d(fabs(xi));
        double lam = 1.0, lam2 = 0.0, val2 = 0.0, fnew = fp;
        bool ok = false;
        for (int ls = 0; ls < 1000; ++ls) {
            if (lam < lam_min) break;
            move(t, pos, y, cen, lam, xi);
            evaluate(t, xp, y, gy, red, ei, ea);
            fnew = ei + ea;
            ++nev;
            if (fnew - fp <= FUNCTOL * lam * slope) { ok = true; break; }
            double tmp;
            if (ls == 0) tmp = -slope / (2.0 * (fnew - fp - slope));
            else {
                const double rhs1 = fnew - fp - lam * slope, rhs2 = val2 - fp - lam2 * slope;
                const double a = (rhs1 / (lam * lam) - rhs2 / (lam2 * lam2)) / (lam - lam2);
                const double b = (-lam2 * rhs1 / (lam * lam) + lam * rhs2 / (lam2 * lam2)) / (lam - lam2);
                if (a == 0.0) tmp = -slope / (2.0 * b);
                else {
                    const double disc = b * b - 3.0 * a * slope;
                    if (disc < 0.0) tmp = 0.5 * lam;
                    else if (b <= 0.0) tmp = (-b + sqrt(disc)) / (3.0 * a);
                    else tmp = -slope / (b + sqrt(disc));
                }
                if (tmp > 0.5 * lam) tmp = 0.5 * lam;
            }
            lam2 = lam; val2 = fnew;
            lam = fmax(tmp, 0.1 * lam);
        }
        if (!ok) { st = 2; break; }                                     // "nothing was done": the accepted point stays
        // ---------------- the step is accepted: y and gy are the new point's
        for (int i = tid; i < 3 * L; i += NT) pos[i] = y[i];
        fp = fnew;
        ++it;
        if (trace && tid == 0) trace[(long long)p * (max_iters + 1) + it] = fp;
        const double step = lam * xi, g_old = g;
        generalised(t, y, gy, cen, gg);                                  // (its barriers also publish pos)
        g = lane < n ? gg[lane] : 0.0;
        if (wave_max_d(fabs(g)) < grad_tol) { st = 0; break; }
        // ---------------- BFGS update of the inverse Hessian
        const double dg = g - g_old;
        double hdg = 0.0;
        for (int j = 0; j < n; ++j) {
            const double v = __shfl(dg, j);
            if (lane < n) hdg += H[j * n + lane] * v;
        }
        double fac = wave_sum_d(dg * step);
        const double fae = wave_sum_d(dg * hdg), sdg = wave_sum_d(dg * dg), sxi = wave_sum_d(step * step);
        __syncthreads();                                                 // every wave has read H
        if (fac > sqrt(EPS_ * sdg * sxi)) {
            fac = 1.0 / fac;
            const double fad = 1.0 / fae;
            if (tid < 64) { sx[tid] = step; sh[tid] = hdg; sv[tid] = fac * step - fad * hdg; }
            __syncthreads();
            for (int e = tid; e < n * n; e += NT) {
                const int r = e / n, c = e - r * n;
                const int i = r < c ? r : c, j = r < c ? c : r;          // the (i <= j) element, mirrored
                H[e] += (fac * sx[i]) * sx[j] - (fad * sh[i]) * sh[j] + (fae * sv[i]) * sv[j];
            }
            __threadfence_block();
            __syncthreads();
        }
        double nx = 0.0;
        for (int j = 0; j < n; ++j) {
            const double v = __shfl(g, j);
            if (lane < n) nx += H[j * n + lane] * v;
        }
        xi = -nx;
        __syncthreads();                                                 // H is read before the next update
    }
    __syncthreads();
    if (trace && tid == 0)
        for (int k = it + 1; k <= max_iters; ++k) trace[(long long)p * (max_iters + 1) + k] = fp;
    double d2 = 0.0;
    for (int i = tid; i < L; i += NT) {
        const int a = t.lig_idx[i];
        const double dx = pos[3 * i] - (double)xp[3 * a], dy = pos[3 * i + 1] - (double)xp[3 * a + 1], dz = pos[3 * i + 2] - (double)xp[3 * a + 2];
        d2 += dx * dx + dy * dy + dz * dz;
        ob[3 * a] = (float)pos[3 * i]; ob[3 * a + 1] = (float)pos[3 * i + 1]; ob[3 * a + 2] = (float)pos[3 * i + 2];
    }
    d2 = wave_sum_d(d2);
    if (lane == 0) red[tid >> 6] = d2;
    __syncthreads();
    if (tid == 0) {
        e_start[p] = f0; e_end[p] = fp;
        iterations[p] = it; evaluations[p] = nev; status[p] = st;
        moved[p] = sqrt((((red[0] + red[1]) + red[2]) + red[3]) / (double)L);
    }
}

bool aligned(const void* q, uintptr_t a) { return ((uintptr_t)q & (a - 1)) == 0; }

// PD_OK, or the code the tables and sizes earn
int check_tables(const float* x, const int* lig_idx, const unsigned char* type, const unsigned char* rec_mask,
                 const unsigned char* lig_active, const int* rot, const unsigned* rot_mask, const int* intra_start,
                 const int* intra_atom, int n_intra, int P, int A, int L, int T) {
    if (!x || !lig_idx || !type || !rec_mask || !lig_active || !intra_start) return PD_ERR_ARG;
    if (P <= 0 || A <= 0 || L <= 0 || T < 0 || n_intra < 0) return PD_ERR_ARG;
    if ((T > 0 && (!rot || !rot_mask)) || (n_intra > 0 && !intra_atom)) return PD_ERR_ARG;
    if (!aligned(x, 4) || !aligned(lig_idx, 4) || !aligned(rot, 4) || !aligned(rot_mask, 4) || !aligned(intra_start, 4) ||
        !aligned(intra_atom, 4))
        return PD_ERR_ARG;
    if (L > VR_MAX_L || T > VR_MAX_T || A > VR_MAX_A || P > 65535) return PD_ERR_UNSUPPORTED;
    return PD_OK;
}

}  // namespace

PD_EXPORT int pd_vina_refine_workspace_numel(int P, int L, int T) {
    if (P <= 0 || L <= 0 || T < 0) return PD_ERR_ARG;
    if (L > VR_MAX_L || T > VR_MAX_T || P > 65535) return PD_ERR_UNSUPPORTED;
    return P * ((6 + T) * (6 + T) + 3 * L);                              // at most 65535 * 7168: an int holds it
}

PD_EXPORT int pd_vina_refine_energy(const float* x, const int* lig_idx, const unsigned char* type, const unsigned char* rec_mask,
                                    const unsigned char* lig_active, const int* rot, const unsigned* rot_mask,
                                    const int* intra_start, const int* intra_atom, int n_intra, double* energy, double* inter,
                                    double* intra, double* grad, double* ggrad, int P, int A, int L, int T, void* stream) {
    const int rc = check_tables(x, lig_idx, type, rec_mask, lig_active, rot, rot_mask, intra_start, intra_atom, n_intra, P, A, L, T);
    if (rc == PD_ERR_ARG) return rc;
    if (!aligned(energy, 8) || !aligned(inter, 8) || !aligned(intra, 8) || !aligned(grad, 8) || !aligned(ggrad, 8)) return PD_ERR_ARG;
    if (rc != PD_OK) return rc;
    const Tab t = {lig_idx, type, rec_mask, lig_active, rot, rot_mask, intra_start, intra_atom, A, L, T};
    hipLaunchKernelGGL(vina_refine_energy_kernel, dim3(P), dim3(NT), 6 * (size_t)L * sizeof(double), (hipStream_t)stream, t, x, energy,
                       inter, intra, grad, ggrad);
    return pd_check_launch();
}

PD_EXPORT int pd_vina_refine(const float* x, const int* lig_idx, const unsigned char* type, const unsigned char* rec_mask,
                             const unsigned char* lig_active, const int* rot, const unsigned* rot_mask, const int* intra_start,
                             const int* intra_atom, int n_intra, int max_iters, double grad_tol, double max_step, double* ws,
                             long long ws_numel, float* x_refined, double* energy_start, double* energy, int* iterations,
                             int* evaluations, int* status, double* moved, double* energy_trace, int P, int A, int L, int T,
                             void* stream) {
    const int rc = check_tables(x, lig_idx, type, rec_mask, lig_active, rot, rot_mask, intra_start, intra_atom, n_intra, P, A, L, T);
    if (rc == PD_ERR_ARG) return rc;
    if (!ws || !x_refined || !energy_start || !energy || !iterations || !evaluations || !status || !moved) return PD_ERR_ARG;
    if (max_iters < 0 || !(grad_tol >= 0.0) || !(max_step > 0.0)) return PD_ERR_ARG;
    if (!aligned(ws, 8) || !aligned(x_refined, 4) || !aligned(energy_start, 8) || !aligned(energy, 8) || !aligned(iterations, 4) ||
        !aligned(evaluations, 4) || !aligned(status, 4) || !aligned(moved, 8) || !aligned(energy_trace, 8))
        return PD_ERR_ARG;
    if (rc != PD_OK) return rc;
    if (ws_numel < (long long)pd_vina_refine_workspace_numel(P, L, T)) return PD_ERR_ARG;
    const Tab t = {lig_idx, type, rec_mask, lig_active, rot, rot_mask, intra_start, intra_atom, A, L, T};
    hipLaunchKernelGGL(vina_refine_kernel, dim3(P), dim3(NT), 6 * (size_t)L * sizeof(double), (hipStream_t)stream, t, x, x_refined, ws,
                       max_iters, grad_tol, max_step, energy_start, energy, iterations, evaluations, status, moved, energy_trace);
    return pd_check_launch();
}
