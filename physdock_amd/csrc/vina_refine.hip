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
//
// pd_vina_search is the Monte-Carlo loop around that minimiser (tests/vina_search_ref.py is its written definition): K independent
// chains per pose, each perturbing one entity per step (translation, rotation or one torsion; Philox draws keyed by seed, pose id,
// chain and step), minimising, applying the Metropolis test and keeping its best.  One block per (pose, chain) with the same LDS
// layout, so that chains whose descents take different numbers of iterations never wait for one another; `descend` (vina_descend.h) is the
// one BFGS both kernels call.  Per chain the workspace holds H, the descent's conformation, cur and best ((6+T)^2 + 9 L doubles) and the
// chain's scalars, which is what makes a search resumable launch by launch.  LDS: 6 L doubles is 48 KB at L = 1024, with the 2 KB of
// static scratch inside the 64 KB a workgroup may have; the chains are latency-bound float64 VALU work, as the refinement is.
#include "common.h"
#include "philox.h"
#include "physdock_hip.h"
#include "vina_descend.h"                                                // the pair function and `descend`, shared with vina_flex.hip

namespace {

constexpr int VR_MAX_L = 1024, VR_MAX_A = 1 << 22, VR_MAX_T = PD_VINA_REFINE_MAX_TORSIONS;
static_assert(VR_MAX_T + 6 == 64, "one lane per coordinate");

struct Tab {
    const int* lig_idx; const unsigned char* type; const unsigned char* rec_mask; const unsigned char* lig_active;
    const int* rot; const unsigned* rot_mask; const int* intra_start; const int* intra_atom;
    int A, L, T;
    __device__ int rows() const { return L; }
    __device__ int coords() const { return 6 + T; }
};

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
        ei = wave_sum(ei); ea = wave_sum(ea);
        gx = wave_sum(gx); gyy = wave_sum(gyy); gz = wave_sum(gz);
        if (lane == 0) { gy[3 * i] = gx; gy[3 * i + 1] = gyy; gy[3 * i + 2] = gz; }
        e_inter += ei; e_intra += ea;                                   // ascending atoms of this wave
    }
    __syncthreads();                                                     // red is free again
    if (lane == 0) { red[wave] = e_inter; red[4 + wave] = e_intra; }
    __syncthreads();
    inter = ((red[0] + red[1]) + red[2]) + red[3];
    intra = ((red[4] + red[5]) + red[6]) + red[7];
}

// E = inter + intra, as `descend` asks for it
__device__ __forceinline__ double energy_of(const Tab& t, const float* __restrict__ xp, const double* y, double* gy, double* red) {
    double ei, ea;
    evaluate(t, xp, y, gy, red, ei, ea);
    return ei + ea;
}

// cen[3] (LDS) = the unweighted centroid of y.  All threads; returns after a barrier.
__device__ void centroid(const double* y, int L, double* cen) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave < 3) {
        double s = 0.0;
        for (int i = lane; i < L; i += 64) s += y[3 * i + wave];
        s = wave_sum(s);
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
        acc = wave_sum(acc);
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
    const Lds s = {sm, sm + 3 * L, red, cen, gg, sx, sh, sv};
    double* H = ws + (long long)p * ((long long)n * n + 3ll * L);         // inverse Hessian [n][n], kept exactly symmetric
    double* pos = H + n * n;                                             // the accepted conformation [L][3]
    const float* xp = x + (long long)p * A * 3;
    float* ob = x_out + (long long)p * A * 3;
    for (int i = tid; i < 3 * A; i += NT) ob[i] = xp[i];
    for (int i = tid; i < 3 * L; i += NT) {
        const double v = (double)xp[3 * t.lig_idx[i / 3] + i % 3];
        pos[i] = v; s.y[i] = v;
    }
    Descent d;
    descend(t, xp, H, pos, s, max_iters, grad_tol, max_step, trace ? trace + (long long)p * (max_iters + 1) : nullptr, d);
    double d2 = 0.0;
    for (int i = tid; i < L; i += NT) {
        const int a = t.lig_idx[i];
        const double dx = pos[3 * i] - (double)xp[3 * a], dy = pos[3 * i + 1] - (double)xp[3 * a + 1], dz = pos[3 * i + 2] - (double)xp[3 * a + 2];
        d2 += dx * dx + dy * dy + dz * dz;
        ob[3 * a] = (float)pos[3 * i]; ob[3 * a + 1] = (float)pos[3 * i + 1]; ob[3 * a + 2] = (float)pos[3 * i + 2];
    }
    d2 = wave_sum(d2);
    if (lane == 0) red[tid >> 6] = d2;
    __syncthreads();
    if (tid == 0) {
        e_start[p] = d.f0; e_end[p] = d.fp;
        iterations[p] = d.it; evaluations[p] = d.nev; status[p] = d.st;
        moved[p] = sqrt((((red[0] + red[1]) + red[2]) + red[3]) / (double)L);
    }
}

// ------------------------------------------------------------------ the Monte-Carlo search (tests/vina_search_ref.py is its definition)
constexpr int VS_SCALARS = 8;                                            // E_cur, E_best, E_start, best_step, accepted, evaluations, 2 spare
constexpr int VS_MAX_K = 64, VS_MAX_BLOCKS = 65535;
constexpr double VS_PI = 3.14159265358979323846;

struct SearchArgs {
    unsigned long long seed;
    int pose0, step0, n_steps, steps_total, K, max_iters;
    double grad_tol, max_step, temperature, translate_amp, rotate_amp;
    float* x_chains; double* energy_chains; double* energy_start; int* best_step; int* accepted; int* evaluations;
    double* trace_energy; int* trace_entity; int* trace_accept; int* trace_iterations; int* trace_status;
};

__device__ __forceinline__ long long vs_stride(int L, int T) { return (long long)(6 + T) * (6 + T) + 9ll * L + VS_SCALARS; }

// One block per (pose, chain): the chain runs its steps step0 + 1 .. step0 + n_steps on its own (step 0, the start descent, when
// step0 == 0).  Its state - cur, best [L][3], E_cur, E_best, E_start and the counters - lives in the workspace between launches, and
// the draws depend on (seed, pose id, chain, step) alone, so a search cut into launches is the same search.  Every decision is taken
// by all threads alike from values that are the same in every thread.
__global__ __launch_bounds__(NT) void vina_search_kernel(const Tab t, const float* __restrict__ x, double* __restrict__ ws,
                                                         const SearchArgs a) {
    extern __shared__ double sm[];
    __shared__ double red[8], cen[3], gg[64], sx[64], sh[64], sv[64];
    const int tid = threadIdx.x, lane = tid & 63, L = t.L, A = t.A, n = 6 + t.T;
    const int p = blockIdx.x / a.K, c = blockIdx.x - p * a.K;
    const Lds s = {sm, sm + 3 * L, red, cen, gg, sx, sh, sv};
    double* H = ws + (long long)blockIdx.x * vs_stride(L, t.T);
    double* pos = H + n * n;                                             // the descent's accepted conformation
    double* cur = pos + 3 * L;
    double* best = cur + 3 * L;
    double* sc = best + 3 * L;
    const float* xp = x + (long long)p * A * 3;
    const long long pc = blockIdx.x;
    const Philox ph{(uint32_t)a.seed, (uint32_t)(a.seed >> 32)};
    const uint32_t q = (uint32_t)(a.pose0 + p);
    double e_cur = 0.0, e_best = 0.0, e_start = 0.0;
    int best_step = 0, accepted = 0, evaluations = 0;
    if (a.step0 > 0) {
        e_cur = sc[0]; e_best = sc[1]; e_start = sc[2];
        best_step = (int)sc[3]; accepted = (int)sc[4]; evaluations = (int)sc[5];
    }
    for (int m = a.step0 > 0 ? a.step0 + 1 : 0; m <= a.step0 + a.n_steps; ++m) {
        int entity = 0;
        double u4 = 0.0;
        if (m == 0) {
            for (int i = tid; i < 3 * L; i += NT) {
                const double v = (double)xp[3 * t.lig_idx[i / 3] + i % 3];
                pos[i] = v; s.y[i] = v;
            }
        } else {
            uint32_t w[4] = {q, (uint32_t)c, (uint32_t)m, 0u}, w4[4] = {q, (uint32_t)c, (uint32_t)m, 1u};
            ph.gen(w); ph.gen(w4);
            entity = (int)(((uint64_t)w[0] * (uint64_t)(2 + t.T)) >> 32);
            const double u1 = ((double)w[1] + 0.5) * 0x1p-32, u2 = ((double)w[2] + 0.5) * 0x1p-32, u3 = ((double)w[3] + 0.5) * 0x1p-32;
            u4 = ((double)w4[0] + 0.5) * 0x1p-32;
            double sl = 0.0;                                             // this lane's coordinate of the proposal s
            if (entity < 2) {
                const int k = lane - 3 * entity;
                const double amp = entity == 0 ? a.translate_amp : a.rotate_amp;
                if (k >= 0 && k < 3) sl = amp * (2.0 * (k == 0 ? u1 : (k == 1 ? u2 : u3)) - 1.0);
            } else if (lane == 6 + entity - 2) {
                sl = VS_PI * (2.0 * u1 - 1.0);
            }
            move(t, cur, s.y, cen, 1.0, sl);                             // y = move(cur, s)
            for (int i = tid; i < 3 * L; i += NT) pos[i] = s.y[i];
        }
        Descent d;
        descend(t, xp, H, pos, s, a.max_iters, a.grad_tol, a.max_step, nullptr, d);
        evaluations += d.nev;
        const double e_new = d.fp;
        const bool finite = isfinite(e_new);
        bool acc, nb;
        if (m == 0) {
            acc = true; nb = true;
            e_start = e_new;
        } else {
            acc = finite && (e_new < e_cur || u4 < exp((e_cur - e_new) / a.temperature));
            nb = finite && e_new < e_best;
            if (acc) ++accepted;
        }
        if (acc) {
            e_cur = e_new;
            for (int i = tid; i < 3 * L; i += NT) cur[i] = pos[i];
        }
        if (nb) {
            e_best = e_new; best_step = m;
            for (int i = tid; i < 3 * L; i += NT) best[i] = pos[i];
        }
        if (tid == 0) {
            if (a.trace_energy) a.trace_energy[pc * (a.steps_total + 1) + m] = e_new;
            if (m > 0) {
                const long long o = pc * a.steps_total + (m - 1);
                if (a.trace_entity) a.trace_entity[o] = entity;
                if (a.trace_accept) a.trace_accept[o] = acc ? 1 : 0;
                if (a.trace_iterations) a.trace_iterations[o] = d.it;
                if (a.trace_status) a.trace_status[o] = d.st;
            }
        }
        __syncthreads();                                                 // cur is published before the next proposal reads it
    }
    for (int i = tid; i < 3 * L; i += NT) a.x_chains[pc * 3 * L + i] = (float)best[i];   // each thread reads what it wrote, or an earlier launch did
    if (tid == 0) {
        sc[0] = e_cur; sc[1] = e_best; sc[2] = e_start;
        sc[3] = (double)best_step; sc[4] = (double)accepted; sc[5] = (double)evaluations;
        a.energy_chains[pc] = e_best; a.energy_start[pc] = e_start;
        a.best_step[pc] = best_step; a.accepted[pc] = accepted; a.evaluations[pc] = evaluations;
    }
}

// One block per pose: the chain with the lowest energy (the lowest index on a tie), and x with that chain's ligand rows.
__global__ __launch_bounds__(NT) void vina_search_select_kernel(const float* __restrict__ x, const int* __restrict__ lig_idx,
                                                                const float* __restrict__ x_chains,
                                                                const double* __restrict__ energy_chains, int* __restrict__ best_chain,
                                                                double* __restrict__ energy, float* __restrict__ x_search, int K,
                                                                int A, int L) {
    const int tid = threadIdx.x, p = blockIdx.x;
    int b = 0;
    double e = energy_chains[(long long)p * K];
    for (int c = 1; c < K; ++c) {                                        // every thread alike
        const double v = energy_chains[(long long)p * K + c];
        if (v < e) { e = v; b = c; }
    }
    const float* xp = x + (long long)p * A * 3;
    float* ob = x_search + (long long)p * A * 3;
    for (int i = tid; i < 3 * A; i += NT) ob[i] = xp[i];
    __syncthreads();                                                     // the ligand rows are overwritten after the copy
    const float* yb = x_chains + ((long long)p * K + b) * 3 * L;
    for (int i = tid; i < 3 * L; i += NT) ob[3 * lig_idx[i / 3] + i % 3] = yb[i];
    if (tid == 0) { best_chain[p] = b; energy[p] = e; }
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

PD_EXPORT long long pd_vina_search_workspace_numel(int P, int K, int L, int T) {
    if (P <= 0 || K <= 0 || L <= 0 || T < 0) return PD_ERR_ARG;
    if (L > VR_MAX_L || T > VR_MAX_T || K > VS_MAX_K || (long long)P * K > VS_MAX_BLOCKS) return PD_ERR_UNSUPPORTED;
    return (long long)P * K * ((long long)(6 + T) * (6 + T) + 9ll * L + VS_SCALARS);
}

PD_EXPORT int pd_vina_search(const float* x, const int* lig_idx, const unsigned char* type, const unsigned char* rec_mask,
                             const unsigned char* lig_active, const int* rot, const unsigned* rot_mask, const int* intra_start,
                             const int* intra_atom, int n_intra, int max_iters, double grad_tol, double max_step,
                             unsigned long long seed, int pose0, int step0, int n_steps, int steps_total, double temperature,
                             double translate_amp, double rotate_amp, double* ws, long long ws_numel, float* x_chains,
                             double* energy_chains, double* energy_start, int* best_step, int* accepted, int* evaluations,
                             double* trace_energy, int* trace_entity, int* trace_accept, int* trace_iterations, int* trace_status,
                             int P, int K, int A, int L, int T, void* stream) {
    const int rc = check_tables(x, lig_idx, type, rec_mask, lig_active, rot, rot_mask, intra_start, intra_atom, n_intra, P, A, L, T);
    if (rc == PD_ERR_ARG) return rc;
    if (!ws || !x_chains || !energy_chains || !energy_start || !best_step || !accepted || !evaluations) return PD_ERR_ARG;
    if (max_iters < 0 || !(grad_tol >= 0.0) || !(max_step > 0.0)) return PD_ERR_ARG;
    if (K < 1 || pose0 < 0 || step0 < 0 || n_steps < 0 || steps_total < 0 || (long long)step0 + n_steps > steps_total) return PD_ERR_ARG;
    if (!(temperature > 0.0) || !(translate_amp >= 0.0) || !(rotate_amp >= 0.0)) return PD_ERR_ARG;
    if (!aligned(ws, 8) || !aligned(x_chains, 4) || !aligned(energy_chains, 8) || !aligned(energy_start, 8) || !aligned(best_step, 4) ||
        !aligned(accepted, 4) || !aligned(evaluations, 4) || !aligned(trace_energy, 8) || !aligned(trace_entity, 4) ||
        !aligned(trace_accept, 4) || !aligned(trace_iterations, 4) || !aligned(trace_status, 4))
        return PD_ERR_ARG;
    if (rc != PD_OK) return rc;
    if (K > VS_MAX_K || (long long)P * K > VS_MAX_BLOCKS || (long long)pose0 + P > 0x7fffffffll) return PD_ERR_UNSUPPORTED;
    if (ws_numel < pd_vina_search_workspace_numel(P, K, L, T)) return PD_ERR_ARG;
    const Tab t = {lig_idx, type, rec_mask, lig_active, rot, rot_mask, intra_start, intra_atom, A, L, T};
    const SearchArgs a = {seed, pose0, step0, n_steps, steps_total, K, max_iters, grad_tol, max_step, temperature, translate_amp,
                          rotate_amp, x_chains, energy_chains, energy_start, best_step, accepted, evaluations, trace_energy,
                          trace_entity, trace_accept, trace_iterations, trace_status};
    hipLaunchKernelGGL(vina_search_kernel, dim3(P * K), dim3(NT), 6 * (size_t)L * sizeof(double), (hipStream_t)stream, t, x, ws, a);
    return pd_check_launch();
}

PD_EXPORT int pd_vina_search_select(const float* x, const int* lig_idx, const float* x_chains, const double* energy_chains,
                                    int* best_chain, double* energy, float* x_search, int P, int K, int A, int L, void* stream) {
    if (!x || !lig_idx || !x_chains || !energy_chains || !best_chain || !energy || !x_search) return PD_ERR_ARG;
    if (P <= 0 || K <= 0 || A <= 0 || L <= 0) return PD_ERR_ARG;
    if (!aligned(x, 4) || !aligned(lig_idx, 4) || !aligned(x_chains, 4) || !aligned(energy_chains, 8) || !aligned(best_chain, 4) ||
        !aligned(energy, 8) || !aligned(x_search, 4))
        return PD_ERR_ARG;
    if (L > VR_MAX_L || A > VR_MAX_A || K > VS_MAX_K || P > VS_MAX_BLOCKS) return PD_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(vina_search_select_kernel, dim3(P), dim3(NT), 0, (hipStream_t)stream, x, lig_idx, x_chains, energy_chains, best_chain,
                       energy, x_search, K, A, L);
    return pd_check_launch();
}
