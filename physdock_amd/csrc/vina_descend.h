// What vina_refine.hip (pd_vina_refine, pd_vina_search) and vina_flex.hip (pd_vina_flex_refine) share: the Vina pair function in
// float64 and the BFGS / lnsrch minimiser in generalised coordinates, one coordinate per lane of a wave.
//
// `descend` is a template over the model `Tab` of its caller, which supplies (found by argument-dependent lookup where the template
// is instantiated):
//     t.rows()                                 the atoms of a conformation (pos and y hold 3 rows() doubles)
//     t.coords()                               n <= 64, the generalised coordinates
//     energy_of(t, xp, y, gy, red)             E of the conformation y (LDS), its Cartesian gradient to gy (LDS); all threads
//     generalised(t, y, gy, cen, gg)           gg[0 .. n-1] (LDS) = the generalised gradient; barrier at the end
//     move(t, pos, y, cen, lam, xi)            y = move(pos, lam * xi), xi this lane's coordinate; y complete on return
#pragma once
#include "common.h"

constexpr int NT = 256;
constexpr double CUTOFF = 8.0;
constexpr double W_GAUSS1 = -0.0356, W_GAUSS2 = -0.00516, W_REPULSION = 0.840, W_HYDROPHOBIC = -0.0351, W_HBOND = -0.587;
constexpr double FUNCTOL = 1e-4, MOVETOL = 1e-7, EPS_ = 3e-8;

static __device__ const double VR_RADIUS[16] = {1.9, 1.8, 1.7, 2.1, 2.0, 1.5, 1.8, 2.0, 2.2, 1.2, 1.2, 1.2, 1.2, 1.2, 1.2, 1.2};

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

// The LDS of a block that minimises: the conformation under evaluation and its Cartesian gradient (3 rows() doubles each, dynamic),
// the scratch of the reductions and of the BFGS update (static).
struct Lds { double *y, *gy, *red, *cen, *gg, *sx, *sh, *sv; };
struct Descent { double f0, fp; int it, nev, st; };                     // E at the start and the end, accepted steps, evaluations, status

// The minimiser: descend from the conformation that `pos` (workspace, [rows][3]) and s.y (LDS) both hold, with a fresh H = I
// (workspace, [n][n]).  All NT threads; on return `pos` holds the accepted conformation (published to the block), `d` the same values
// in every thread.  trace: this descent's max_iters + 1 energies, or NULL.
template <class Tab>
__device__ __forceinline__ void descend(const Tab& t, const float* __restrict__ xp, double* __restrict__ H, double* __restrict__ pos,
                                        const Lds& s_, int max_iters, double grad_tol, double max_step, double* __restrict__ trace,
                                        Descent& d) {
    double *y = s_.y, *gy = s_.gy, *red = s_.red, *cen = s_.cen, *gg = s_.gg, *sx = s_.sx, *sh = s_.sh, *sv = s_.sv;
    const int tid = threadIdx.x, lane = tid & 63, L = t.rows(), n = t.coords();
    for (int e = tid; e < n * n; e += NT) H[e] = (e / n == e % n) ? 1.0 : 0.0;
    __syncthreads();
    double fp = energy_of(t, xp, y, gy, red);
    generalised(t, y, gy, cen, gg);
    double g = lane < n ? gg[lane] : 0.0;                                // this lane's coordinate, the same in every wave
    double xi = -g;
    const double f0 = fp;
    int it = 0, nev = 1, st = 1;
    if (trace && tid == 0) trace[0] = fp;
    if (wave_max(fabs(g)) < grad_tol) st = 0;
    while (st == 1 && it < max_iters) {
        // ---------------- the line search (Numerical Recipes lnsrch)
        const double s = sqrt(wave_sum(xi * xi));
        if (s > max_step) xi *= max_step / s;
        const double slope = wave_sum(xi * g);
        if (!(slope < 0.0)) { st = 2; break; }
        const double lam_min = MOVETOL / wave_max(fabs(xi));
        double lam = 1.0, lam2 = 0.0, val2 = 0.0, fnew = fp;
        bool ok = false;
        for (int ls = 0; ls < 1000; ++ls) {
            if (lam < lam_min) break;
            move(t, pos, y, cen, lam, xi);
            fnew = energy_of(t, xp, y, gy, red);
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
        if (trace && tid == 0) trace[it] = fp;
        const double step = lam * xi, g_old = g;
        generalised(t, y, gy, cen, gg);                                  // (its barriers also publish pos)
        g = lane < n ? gg[lane] : 0.0;
        if (wave_max(fabs(g)) < grad_tol) { st = 0; break; }
        // ---------------- BFGS update of the inverse Hessian
        const double dg = g - g_old;
        double hdg = 0.0;
        for (int j = 0; j < n; ++j) {
            const double v = __shfl(dg, j);
            if (lane < n) hdg += H[j * n + lane] * v;
        }
        double fac = wave_sum(dg * step);
        const double fae = wave_sum(dg * hdg), sdg = wave_sum(dg * dg), sxi = wave_sum(step * step);
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
        for (int k = it + 1; k <= max_iters; ++k) trace[k] = fp;
    d.f0 = f0; d.fp = fp; d.it = it; d.nev = nev; d.st = st;
}
