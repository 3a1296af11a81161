// Local refinement of P poses with flexible receptor side chains, the way `vina --flex` answers a clash: the ligand moves as a rigid
// body and about its rotatable bonds, and chosen side chains turn about their chi bonds, all in one minimisation
// (physdock_amd/flex.py builds the tables once per system; tests/flex_refine_ref.py is the written definition of everything below,
// in float64 NumPy).  Bond lengths, angles and rings are preserved by construction; the backbone and every other residue stay rigid.
//
// Movable rows: M = L + F.  Rows 0 .. L-1 are the ligand atoms of pd_vina_refine's tables, rows L .. M-1 the flexible side-chain
// atoms (mov_idx: their pose indices).  Fixed atoms: fixed_mask, the receptor atoms that are not flexible.
//
// Energy of a conformation y [M][3], float64 throughout:  E = (inter + intra) + receptor, every term the pair function of
// pd_vina_score / pd_vina_refine (vina_descend.h; pairs with r < 8, a pair at r == 0 without force).
//   inter     (active ligand row, fixed atom) and (active ligand row, flexible row)
//   intra     pd_vina_refine's ligand pairs
//   receptor  (flexible row, fixed atom) and (flexible row, flexible row), each more than three bonds apart in the receptor's bond
//             graph (or in different components)
// Movable - movable pairs of all three classes arrive as one neighbour list per row in local indices (pair_start / pair_atom, every
// pair from both of its rows; its class follows from which side of L the two rows lie).  Movable - fixed pairs stream the pose's A
// atoms under fixed_mask; the fixed atoms within three bonds of a flexible row arrive as a short list per row (excl_start /
// excl_atom, pose indices), consulted only for a pair inside the cutoff.  E is not divided by 1 + 0.0585 n_rot.
//
// move(y, s), s in R^(6+T+S): for k = 0 .. T+S-1 rotate the rows of M_k (bit mask rot_mask[k]) by s[6+k] about the axis through
// y[a_k] along y[b_k] - y[a_k] (Rodrigues, on the coordinates as they stand; rows 0 .. T-1 are the ligand's torsions, the others the
// side chains', a on the backbone side, M_k the distal side); rotate the L ligand rows about their unweighted centroid by the
// rotation vector s[3:6]; translate the ligand rows by s[0:3].  Generalised gradient at s = 0:  g[0:3] = sum_{i < L} dE/dy_i,
// g[3:6] = sum_{i < L} (y_i - c) x dE/dy_i,  g[6+k] = sum_{i in M_k} dE/dy_i . (u_k x (y_i - y[a_k])).
//
// Minimiser: `descend` of vina_descend.h - the one pd_vina_refine runs - in these n = 6 + T + S <= 64 coordinates.
//
// Mapping, as pd_vina_refine: one block of 256 threads per pose, one launch.  Wave w takes the rows w, w + 4, ...; its 64 lanes
// stride the pose's atoms and then the row's neighbour list, a butterfly adds the lanes, the wave adds its rows in ascending order
// and the block adds the four waves in order: no atomics, bit-identical from launch to launch and independent of P.  The BFGS
// vectors live one coordinate per lane; H and the accepted conformation in the caller's workspace (per pose n^2 + 3 M doubles); the
// conformation under evaluation and its gradient in LDS (6 M doubles: 48 KB at M = 1024, with 2 KB of static scratch).
//
// pd_vina_flex_search is pd_vina_search's Monte-Carlo loop over this table (tests/flex_search_ref.py is its written definition): K
// chains per pose, each perturbing one entity per step - the ligand's translation, its rotation, one ligand torsion or one chi -
// minimising with `descend` in all 6 + T + S coordinates, applying the Metropolis test to E = (inter + intra) + receptor and keeping
// its best.  One block per (pose, chain), the LDS layout above; per chain the workspace holds H, the descent's conformation, cur and
// best and the chain's scalars (n^2 + 9 M + 8 doubles), which makes a search resumable launch by launch.  The step loop is a copy of
// vina_search_kernel's (vina_refine.hip) with the entity count 2 + T + S and the chi amplitude: the two kernels are kept apart so
// that pd_vina_search's code object does not change.  pd_vina_flex_search_select picks the pose's best chain from the float64 `best`
// of the workspace and evaluates it once more for the parts of E.
#include "common.h"
#include "philox.h"
#include "physdock_hip.h"
#include "vina_descend.h"

namespace {

constexpr int VF_MAX_M = 1024, VF_MAX_A = 1 << 22, VF_MAX_N = PD_VINA_REFINE_MAX_TORSIONS;
static_assert(VF_MAX_N + 6 == 64, "one lane per coordinate");

struct FlexTab {
    const int* mov_idx; const unsigned char* type; const unsigned char* fixed_mask; const unsigned char* active;
    const int* rot; const unsigned* rot_mask; const int* pair_start; const int* pair_atom; const int* excl_start; const int* excl_atom;
    int A, L, M, N;                                                      // pose atoms, ligand rows, movable rows, torsions T + S
    __device__ int rows() const { return M; }
    __device__ int coords() const { return 6 + N; }
};

// E of the conformation y (LDS); the Cartesian gradient goes to gy (LDS, zeros for an inactive row).  Called by all NT threads with
// y complete; returns with gy complete and (inter, intra, receptor) in every thread.
__device__ void evaluate(const FlexTab& t, const float* __restrict__ xp, const double* y, double* gy, double* red, double& inter,
                         double& intra, double& receptor) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, L = t.L;
    double e_inter = 0.0, e_intra = 0.0, e_rec = 0.0;
    for (int i = wave; i < t.M; i += NT / 64) {
        double ef = 0.0, el = 0.0, eh = 0.0, gx = 0.0, gyy = 0.0, gz = 0.0;   // pairs with fixed atoms, with rows < L, with rows >= L
        if (t.active[i]) {                                               // uniform over the wave
            const double ax = y[3 * i], ay = y[3 * i + 1], az = y[3 * i + 2];
            const unsigned ti = t.type[t.mov_idx[i]];
            const double ri = VR_RADIUS[ti & 15];
            const int x0 = i < L ? 0 : t.excl_start[i], x1 = i < L ? 0 : t.excl_start[i + 1];
            for (int j = lane; j < t.A; j += 64) {
                if (!t.fixed_mask[j]) continue;
                const double dx = ax - (double)xp[3 * j], dy = ay - (double)xp[3 * j + 1], dz = az - (double)xp[3 * j + 2];
                const double r = sqrt(dx * dx + dy * dy + dz * dz);
                if (!(r < CUTOFF)) continue;
                bool near = false;                                       // within three bonds of row i
                for (int q = x0; q < x1; ++q) near |= t.excl_atom[q] == j;
                if (near) continue;
                const unsigned tj = t.type[j];
                double e, de;
                pair_energy(r, ri + VR_RADIUS[tj & 15], ti, tj, e, de);
                ef += e;
                if (r > 0.0) {
                    const double s = de / r;
                    gx += s * dx; gyy += s * dy; gz += s * dz;
                }
            }
            for (int q = t.pair_start[i] + lane; q < t.pair_start[i + 1]; q += 64) {
                const int j = t.pair_atom[q];
                const double dx = ax - y[3 * j], dy = ay - y[3 * j + 1], dz = az - y[3 * j + 2];
                const double r = sqrt(dx * dx + dy * dy + dz * dz);
                if (!(r < CUTOFF)) continue;
                const unsigned tj = t.type[t.mov_idx[j]];
                double e, de;
                pair_energy(r, ri + VR_RADIUS[tj & 15], ti, tj, e, de);
                if (j > i) {                                             // a pair is met from both of its rows
                    if (j < L) el += e; else eh += e;
                }
                if (r > 0.0) {
                    const double s = de / r;
                    gx += s * dx; gyy += s * dy; gz += s * dz;
                }
            }
        }
        ef = wave_sum(ef); el = wave_sum(el); eh = wave_sum(eh);
        gx = wave_sum(gx); gyy = wave_sum(gyy); gz = wave_sum(gz);
        if (lane == 0) { gy[3 * i] = gx; gy[3 * i + 1] = gyy; gy[3 * i + 2] = gz; }
        if (i < L) { e_inter += ef + eh; e_intra += el; }               // ascending rows of this wave
        else e_rec += ef + eh;                                           // (j > i >= L: el is zero)
    }
    __syncthreads();                                                     // red is free again
    if (lane == 0) { red[wave] = e_inter; red[4 + wave] = e_intra; red[8 + wave] = e_rec; }
    __syncthreads();
    inter = ((red[0] + red[1]) + red[2]) + red[3];
    intra = ((red[4] + red[5]) + red[6]) + red[7];
    receptor = ((red[8] + red[9]) + red[10]) + red[11];
}

// E = (inter + intra) + receptor, as `descend` asks for it
__device__ __forceinline__ double energy_of(const FlexTab& t, const float* __restrict__ xp, const double* y, double* gy, double* red) {
    double ei, ea, er;
    evaluate(t, xp, y, gy, red, ei, ea, er);
    return (ei + ea) + er;
}

// cen[3] (LDS) = the unweighted centroid of the L ligand rows of y.  All threads; returns after a barrier.
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

// gg[6 + N] (LDS) = the generalised gradient of the conformation y with the Cartesian gradient gy.  All threads; barrier at the end.
__device__ void generalised(const FlexTab& t, const double* y, const double* gy, double* cen, double* gg) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, L = t.L, M = t.M, W = (M + 31) >> 5;
    centroid(y, L, cen);
    const double cx = cen[0], cy = cen[1], cz = cen[2];
    for (int c = wave; c < 6 + t.N; c += NT / 64) {
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
            for (int i = lane; i < M; i += 64) {
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
__device__ void move(const FlexTab& t, const double* __restrict__ pos, double* y, double* cen, double lam, double xi) {
    const int tid = threadIdx.x, L = t.L, M = t.M, W = (M + 31) >> 5;
    for (int i = tid; i < 3 * M; i += NT) y[i] = pos[i];
    __syncthreads();
    for (int k = 0; k < t.N; ++k) {
        const double th = lam * __shfl(xi, 6 + k);
        const int a = t.rot[2 * k], b = t.rot[2 * k + 1];
        const double ax = y[3 * a], ay = y[3 * a + 1], az = y[3 * a + 2];
        double ux = y[3 * b] - ax, uy = y[3 * b + 1] - ay, uz = y[3 * b + 2] - az;
        __syncthreads();                                                 // the axis is read before b moves
        const double n = sqrt(ux * ux + uy * uy + uz * uz);
        ux /= n; uy /= n; uz /= n;
        const double sn = sin(th), cs = cos(th);
        for (int i = tid; i < M; i += NT) {
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

__global__ __launch_bounds__(NT) void vina_flex_energy_kernel(const FlexTab t, const float* __restrict__ x, double* __restrict__ energy,
                                                              double* __restrict__ inter, double* __restrict__ intra,
                                                              double* __restrict__ receptor, double* __restrict__ grad,
                                                              double* __restrict__ ggrad) {
    extern __shared__ double sm[];
    __shared__ double red[12], cen[3], gg[64];
    const int tid = threadIdx.x, p = blockIdx.x, M = t.M;
    double* y = sm;
    double* gy = sm + 3 * M;
    const float* xp = x + (long long)p * t.A * 3;
    for (int i = tid; i < 3 * M; i += NT) y[i] = (double)xp[3 * t.mov_idx[i / 3] + i % 3];
    __syncthreads();
    double ei, ea, er;
    evaluate(t, xp, y, gy, red, ei, ea, er);
    if (tid == 0) {
        if (energy) energy[p] = (ei + ea) + er;
        if (inter) inter[p] = ei;
        if (intra) intra[p] = ea;
        if (receptor) receptor[p] = er;
    }
    if (grad)
        for (int i = tid; i < 3 * M; i += NT) grad[(long long)p * 3 * M + i] = gy[i];
    if (ggrad) {
        generalised(t, y, gy, cen, gg);
        if (tid < 6 + t.N) ggrad[(long long)p * (6 + t.N) + tid] = gg[tid];
    }
}

struct FlexOut {
    float* x_out; double *e_start, *e_end, *inter, *intra, *receptor; int *iterations, *evaluations, *status;
    double *moved, *moved_flex, *trace;
};

__global__ __launch_bounds__(NT) void vina_flex_refine_kernel(const FlexTab t, const float* __restrict__ x, double* __restrict__ ws,
                                                              int max_iters, double grad_tol, double max_step, const FlexOut o) {
    extern __shared__ double sm[];
    __shared__ double red[12], cen[3], gg[64], sx[64], sh[64], sv[64];
    const int tid = threadIdx.x, lane = tid & 63, p = blockIdx.x, L = t.L, M = t.M, A = t.A, n = 6 + t.N;
    const Lds s = {sm, sm + 3 * M, red, cen, gg, sx, sh, sv};
    double* H = ws + (long long)p * ((long long)n * n + 3ll * M);         // inverse Hessian [n][n], kept exactly symmetric
    double* pos = H + n * n;                                             // the accepted conformation [M][3]
    const float* xp = x + (long long)p * A * 3;
    float* ob = o.x_out + (long long)p * A * 3;
    for (int i = tid; i < 3 * A; i += NT) ob[i] = xp[i];
    for (int i = tid; i < 3 * M; i += NT) {
        const double v = (double)xp[3 * t.mov_idx[i / 3] + i % 3];
        pos[i] = v; s.y[i] = v;
    }
    Descent d;
    descend(t, xp, H, pos, s, max_iters, grad_tol, max_step, o.trace ? o.trace + (long long)p * (max_iters + 1) : nullptr, d);
    // the parts of E at the accepted point: one more evaluation, not counted (y may hold a rejected trial of the line search)
    for (int i = tid; i < 3 * M; i += NT) s.y[i] = pos[i];
    __syncthreads();
    double ei, ea, er;
    evaluate(t, xp, s.y, s.gy, red, ei, ea, er);
    __syncthreads();                                                     // red is read before it is written again
    double dl = 0.0, df = 0.0;
    for (int i = tid; i < M; i += NT) {
        const int a = t.mov_idx[i];
        const double dx = pos[3 * i] - (double)xp[3 * a], dy = pos[3 * i + 1] - (double)xp[3 * a + 1], dz = pos[3 * i + 2] - (double)xp[3 * a + 2];
        const double q = dx * dx + dy * dy + dz * dz;
        if (i < L) dl += q; else df += q;
        ob[3 * a] = (float)pos[3 * i]; ob[3 * a + 1] = (float)pos[3 * i + 1]; ob[3 * a + 2] = (float)pos[3 * i + 2];
    }
    dl = wave_sum(dl); df = wave_sum(df);
    if (lane == 0) { red[tid >> 6] = dl; red[4 + (tid >> 6)] = df; }
    __syncthreads();
    if (tid == 0) {
        o.e_start[p] = d.f0; o.e_end[p] = d.fp;
        if (o.inter) o.inter[p] = ei;
        if (o.intra) o.intra[p] = ea;
        if (o.receptor) o.receptor[p] = er;
        o.iterations[p] = d.it; o.evaluations[p] = d.nev; o.status[p] = d.st;
        o.moved[p] = sqrt((((red[0] + red[1]) + red[2]) + red[3]) / (double)L);
        if (o.moved_flex) o.moved_flex[p] = M > L ? sqrt((((red[4] + red[5]) + red[6]) + red[7]) / (double)(M - L)) : 0.0;
    }
}

// ------------------------------------------------------------------ the Monte-Carlo search (tests/flex_search_ref.py is its definition)
constexpr int FS_SCALARS = 8;                                            // E_cur, E_best, E_start, best_step, accepted, evaluations, 2 spare
constexpr int FS_MAX_K = 64, FS_MAX_BLOCKS = 65535;
constexpr double FS_PI = 3.14159265358979323846;

struct FlexSearchArgs {
    unsigned long long seed;
    int pose0, step0, n_steps, steps_total, K, T, max_iters;             // T: the ligand's torsions, the first T of the table
    double grad_tol, max_step, temperature, translate_amp, rotate_amp, chi_amp;
    float* x_chains; double* energy_chains; double* energy_start; int* best_step; int* accepted; int* evaluations;
    double* trace_energy; int* trace_entity; int* trace_accept; int* trace_iterations; int* trace_status;
};

__host__ __device__ __forceinline__ long long fs_stride(int M, int N) { return (long long)(6 + N) * (6 + N) + 9ll * M + FS_SCALARS; }

// One block per (pose, chain): the chain runs its steps step0 + 1 .. step0 + n_steps on its own (step 0, the start descent, when
// step0 == 0).  Its state - cur, best [M][3], E_cur, E_best, E_start and the counters - lives in the workspace between launches, and
// the draws depend on (seed, pose id, chain, step) alone, so a search cut into launches is the same search.  Every decision is taken
// by all threads alike from values that are the same in every thread.
__global__ __launch_bounds__(NT) void vina_flex_search_kernel(const FlexTab t, const float* __restrict__ x, double* __restrict__ ws,
                                                              const FlexSearchArgs a) {
    extern __shared__ double sm[];
    __shared__ double red[12], cen[3], gg[64], sx[64], sh[64], sv[64];
    const int tid = threadIdx.x, lane = tid & 63, M = t.M, A = t.A, n = 6 + t.N;
    const int p = blockIdx.x / a.K, c = blockIdx.x - p * a.K;
    const Lds s = {sm, sm + 3 * M, red, cen, gg, sx, sh, sv};
    double* H = ws + (long long)blockIdx.x * fs_stride(M, t.N);
    double* pos = H + n * n;                                             // the descent's accepted conformation
    double* cur = pos + 3 * M;
    double* best = cur + 3 * M;
    double* sc = best + 3 * M;
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
            for (int i = tid; i < 3 * M; i += NT) {
                const double v = (double)xp[3 * t.mov_idx[i / 3] + i % 3];
                pos[i] = v; s.y[i] = v;
            }
        } else {
            uint32_t w[4] = {q, (uint32_t)c, (uint32_t)m, 0u}, w4[4] = {q, (uint32_t)c, (uint32_t)m, 1u};
            ph.gen(w); ph.gen(w4);
            entity = (int)(((uint64_t)w[0] * (uint64_t)(2 + t.N)) >> 32);
            const double u1 = ((double)w[1] + 0.5) * 0x1p-32, u2 = ((double)w[2] + 0.5) * 0x1p-32, u3 = ((double)w[3] + 0.5) * 0x1p-32;
            u4 = ((double)w4[0] + 0.5) * 0x1p-32;
            double sl = 0.0;                                             // this lane's coordinate of the proposal s
            if (entity < 2) {
                const int k = lane - 3 * entity;
                const double amp = entity == 0 ? a.translate_amp : a.rotate_amp;
                if (k >= 0 && k < 3) sl = amp * (2.0 * (k == 0 ? u1 : (k == 1 ? u2 : u3)) - 1.0);
            } else if (lane == 6 + entity - 2) {
                sl = (entity - 2 < a.T ? FS_PI : a.chi_amp) * (2.0 * u1 - 1.0);   // a ligand torsion, or a chi
            }
            move(t, cur, s.y, cen, 1.0, sl);                             // y = move(cur, s)
            for (int i = tid; i < 3 * M; i += NT) pos[i] = s.y[i];
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
            for (int i = tid; i < 3 * M; i += NT) cur[i] = pos[i];
        }
        if (nb) {
            e_best = e_new; best_step = m;
            for (int i = tid; i < 3 * M; i += NT) best[i] = pos[i];
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
    for (int i = tid; i < 3 * M; i += NT) a.x_chains[pc * 3 * M + i] = (float)best[i];   // each thread reads what it wrote, or an earlier launch did
    if (tid == 0) {
        sc[0] = e_cur; sc[1] = e_best; sc[2] = e_start;
        sc[3] = (double)best_step; sc[4] = (double)accepted; sc[5] = (double)evaluations;
        a.energy_chains[pc] = e_best; a.energy_start[pc] = e_start;
        a.best_step[pc] = best_step; a.accepted[pc] = accepted; a.evaluations[pc] = evaluations;
    }
}

struct FlexSelectOut {
    int* best_chain; double *energy, *inter, *intra, *receptor; float* x_search; double *moved, *moved_flex;
};

// One block per pose: the chain with the lowest E_best of the workspace (the lowest index on a tie), x with that chain's movable rows
// (float64 `best`, rounded once), the parts of its energy from one more evaluation (not counted) and the two RMSDs from the pose.
__global__ __launch_bounds__(NT) void vina_flex_search_select_kernel(const FlexTab t, const float* __restrict__ x,
                                                                     const double* __restrict__ ws, int K, const FlexSelectOut o) {
    extern __shared__ double sm[];
    __shared__ double red[12];
    const int tid = threadIdx.x, lane = tid & 63, p = blockIdx.x, L = t.L, M = t.M, A = t.A, n = 6 + t.N;
    const long long stride = fs_stride(M, t.N), tail = (long long)n * n + 9ll * M;
    int b = 0;
    double e = ws[(long long)p * K * stride + tail + 1];
    for (int c = 1; c < K; ++c) {                                        // every thread alike
        const double v = ws[((long long)p * K + c) * stride + tail + 1];
        if (v < e) { e = v; b = c; }
    }
    const double* best = ws + ((long long)p * K + b) * stride + (long long)n * n + 6ll * M;
    double* y = sm;
    double* gy = sm + 3 * M;
    const float* xp = x + (long long)p * A * 3;
    float* ob = o.x_search + (long long)p * A * 3;
    for (int i = tid; i < 3 * A; i += NT) ob[i] = xp[i];
    for (int i = tid; i < 3 * M; i += NT) y[i] = best[i];
    __syncthreads();                                                     // the movable rows are overwritten after the copy
    double ei, ea, er;
    evaluate(t, xp, y, gy, red, ei, ea, er);
    __syncthreads();                                                     // red is read before it is written again
    double dl = 0.0, df = 0.0;
    for (int i = tid; i < M; i += NT) {
        const int a = t.mov_idx[i];
        const double dx = y[3 * i] - (double)xp[3 * a], dy = y[3 * i + 1] - (double)xp[3 * a + 1], dz = y[3 * i + 2] - (double)xp[3 * a + 2];
        const double q = dx * dx + dy * dy + dz * dz;
        if (i < L) dl += q; else df += q;
        ob[3 * a] = (float)y[3 * i]; ob[3 * a + 1] = (float)y[3 * i + 1]; ob[3 * a + 2] = (float)y[3 * i + 2];
    }
    dl = wave_sum(dl); df = wave_sum(df);
    if (lane == 0) { red[tid >> 6] = dl; red[4 + (tid >> 6)] = df; }
    __syncthreads();
    if (tid == 0) {
        o.best_chain[p] = b; o.energy[p] = (ei + ea) + er;
        if (o.inter) o.inter[p] = ei;
        if (o.intra) o.intra[p] = ea;
        if (o.receptor) o.receptor[p] = er;
        o.moved[p] = sqrt((((red[0] + red[1]) + red[2]) + red[3]) / (double)L);
        if (o.moved_flex) o.moved_flex[p] = M > L ? sqrt((((red[4] + red[5]) + red[6]) + red[7]) / (double)(M - L)) : 0.0;
    }
}

bool aligned(const void* q, uintptr_t a) { return ((uintptr_t)q & (a - 1)) == 0; }

// PD_OK, or the code the tables and sizes earn
int check_tables(const float* x, const int* mov_idx, const unsigned char* type, const unsigned char* fixed_mask,
                 const unsigned char* active, const int* rot, const unsigned* rot_mask, const int* pair_start, const int* pair_atom,
                 int n_pair, const int* excl_start, const int* excl_atom, int n_excl, int P, int A, int L, int F, int T, int S) {
    if (!x || !mov_idx || !type || !fixed_mask || !active || !pair_start || !excl_start) return PD_ERR_ARG;
    if (P <= 0 || A <= 0 || L <= 0 || F < 0 || T < 0 || S < 0 || n_pair < 0 || n_excl < 0) return PD_ERR_ARG;
    if ((T + (long long)S > 0 && (!rot || !rot_mask)) || (n_pair > 0 && !pair_atom) || (n_excl > 0 && !excl_atom)) return PD_ERR_ARG;
    if (!aligned(x, 4) || !aligned(mov_idx, 4) || !aligned(rot, 4) || !aligned(rot_mask, 4) || !aligned(pair_start, 4) ||
        !aligned(pair_atom, 4) || !aligned(excl_start, 4) || !aligned(excl_atom, 4))
        return PD_ERR_ARG;
    if ((long long)L + F > VF_MAX_M || (long long)T + S > VF_MAX_N || A > VF_MAX_A || P > 65535) return PD_ERR_UNSUPPORTED;
    return PD_OK;
}

}  // namespace

PD_EXPORT int pd_vina_flex_workspace_numel(int P, int M, int N) {
    if (P <= 0 || M <= 0 || N < 0) return PD_ERR_ARG;
    if (M > VF_MAX_M || N > VF_MAX_N || P > 65535) return PD_ERR_UNSUPPORTED;
    return P * ((6 + N) * (6 + N) + 3 * M);                              // at most 65535 * 7168: an int holds it
}

PD_EXPORT int pd_vina_flex_energy(const float* x, const int* mov_idx, const unsigned char* type, const unsigned char* fixed_mask,
                                  const unsigned char* active, const int* rot, const unsigned* rot_mask, const int* pair_start,
                                  const int* pair_atom, int n_pair, const int* excl_start, const int* excl_atom, int n_excl,
                                  double* energy, double* inter, double* intra, double* receptor, double* grad, double* ggrad, int P,
                                  int A, int L, int F, int T, int S, void* stream) {
    const int rc = check_tables(x, mov_idx, type, fixed_mask, active, rot, rot_mask, pair_start, pair_atom, n_pair, excl_start, excl_atom,
                                n_excl, P, A, L, F, T, S);
    if (rc == PD_ERR_ARG) return rc;
    if (!aligned(energy, 8) || !aligned(inter, 8) || !aligned(intra, 8) || !aligned(receptor, 8) || !aligned(grad, 8) || !aligned(ggrad, 8))
        return PD_ERR_ARG;
    if (rc != PD_OK) return rc;
    const FlexTab t = {mov_idx, type, fixed_mask, active, rot, rot_mask, pair_start, pair_atom, excl_start, excl_atom, A, L, L + F, T + S};
    hipLaunchKernelGGL(vina_flex_energy_kernel, dim3(P), dim3(NT), 6 * (size_t)(L + F) * sizeof(double), (hipStream_t)stream, t, x, energy,
                       inter, intra, receptor, grad, ggrad);
    return pd_check_launch();
}

PD_EXPORT int pd_vina_flex_refine(const float* x, const int* mov_idx, const unsigned char* type, const unsigned char* fixed_mask,
                                  const unsigned char* active, const int* rot, const unsigned* rot_mask, const int* pair_start,
                                  const int* pair_atom, int n_pair, const int* excl_start, const int* excl_atom, int n_excl,
                                  int max_iters, double grad_tol, double max_step, double* ws, long long ws_numel, float* x_refined,
                                  double* energy_start, double* energy, double* inter, double* intra, double* receptor,
                                  int* iterations, int* evaluations, int* status, double* moved, double* moved_flex,
                                  double* energy_trace, int P, int A, int L, int F, int T, int S, void* stream) {
    const int rc = check_tables(x, mov_idx, type, fixed_mask, active, rot, rot_mask, pair_start, pair_atom, n_pair, excl_start, excl_atom,
                                n_excl, P, A, L, F, T, S);
    if (rc == PD_ERR_ARG) return rc;
    if (!ws || !x_refined || !energy_start || !energy || !iterations || !evaluations || !status || !moved) return PD_ERR_ARG;
    if (max_iters < 0 || !(grad_tol >= 0.0) || !(max_step > 0.0)) return PD_ERR_ARG;
    if (!aligned(ws, 8) || !aligned(x_refined, 4) || !aligned(energy_start, 8) || !aligned(energy, 8) || !aligned(inter, 8) ||
        !aligned(intra, 8) || !aligned(receptor, 8) || !aligned(iterations, 4) || !aligned(evaluations, 4) || !aligned(status, 4) ||
        !aligned(moved, 8) || !aligned(moved_flex, 8) || !aligned(energy_trace, 8))
        return PD_ERR_ARG;
    if (rc != PD_OK) return rc;
    if (ws_numel < (long long)pd_vina_flex_workspace_numel(P, L + F, T + S)) return PD_ERR_ARG;
    const FlexTab t = {mov_idx, type, fixed_mask, active, rot, rot_mask, pair_start, pair_atom, excl_start, excl_atom, A, L, L + F, T + S};
    const FlexOut o = {x_refined, energy_start, energy, inter, intra, receptor, iterations, evaluations, status, moved, moved_flex,
                       energy_trace};
    hipLaunchKernelGGL(vina_flex_refine_kernel, dim3(P), dim3(NT), 6 * (size_t)(L + F) * sizeof(double), (hipStream_t)stream, t, x, ws,
                       max_iters, grad_tol, max_step, o);
    return pd_check_launch();
}

PD_EXPORT long long pd_vina_flex_search_workspace_numel(int P, int K, int M, int N) {
    if (P <= 0 || K <= 0 || M <= 0 || N < 0) return PD_ERR_ARG;
    if (M > VF_MAX_M || N > VF_MAX_N || K > FS_MAX_K || (long long)P * K > FS_MAX_BLOCKS) return PD_ERR_UNSUPPORTED;
    return (long long)P * K * fs_stride(M, N);
}

PD_EXPORT int pd_vina_flex_search(const float* x, const int* mov_idx, const unsigned char* type, const unsigned char* fixed_mask,
                                  const unsigned char* active, const int* rot, const unsigned* rot_mask, const int* pair_start,
                                  const int* pair_atom, int n_pair, const int* excl_start, const int* excl_atom, int n_excl,
                                  int max_iters, double grad_tol, double max_step, unsigned long long seed, int pose0, int step0,
                                  int n_steps, int steps_total, double temperature, double translate_amp, double rotate_amp,
                                  double chi_amp, double* ws, long long ws_numel, float* x_chains, double* energy_chains,
                                  double* energy_start, int* best_step, int* accepted, int* evaluations, double* trace_energy,
                                  int* trace_entity, int* trace_accept, int* trace_iterations, int* trace_status, int P, int K, int A,
                                  int L, int F, int T, int S, void* stream) {
    const int rc = check_tables(x, mov_idx, type, fixed_mask, active, rot, rot_mask, pair_start, pair_atom, n_pair, excl_start, excl_atom,
                                n_excl, P, A, L, F, T, S);
    if (rc == PD_ERR_ARG) return rc;
    if (!ws || !x_chains || !energy_chains || !energy_start || !best_step || !accepted || !evaluations) return PD_ERR_ARG;
    if (max_iters < 0 || !(grad_tol >= 0.0) || !(max_step > 0.0)) return PD_ERR_ARG;
    if (K < 1 || pose0 < 0 || step0 < 0 || n_steps < 0 || steps_total < 0 || (long long)step0 + n_steps > steps_total) return PD_ERR_ARG;
    if (!(temperature > 0.0) || !(translate_amp >= 0.0) || !(rotate_amp >= 0.0) || !(chi_amp >= 0.0)) return PD_ERR_ARG;
    if (!aligned(ws, 8) || !aligned(x_chains, 4) || !aligned(energy_chains, 8) || !aligned(energy_start, 8) || !aligned(best_step, 4) ||
        !aligned(accepted, 4) || !aligned(evaluations, 4) || !aligned(trace_energy, 8) || !aligned(trace_entity, 4) ||
        !aligned(trace_accept, 4) || !aligned(trace_iterations, 4) || !aligned(trace_status, 4))
        return PD_ERR_ARG;
    if (rc != PD_OK) return rc;
    if (K > FS_MAX_K || (long long)P * K > FS_MAX_BLOCKS || (long long)pose0 + P > 0x7fffffffll) return PD_ERR_UNSUPPORTED;
    if (ws_numel < pd_vina_flex_search_workspace_numel(P, K, L + F, T + S)) return PD_ERR_ARG;
    const FlexTab t = {mov_idx, type, fixed_mask, active, rot, rot_mask, pair_start, pair_atom, excl_start, excl_atom, A, L, L + F, T + S};
    const FlexSearchArgs a = {seed, pose0, step0, n_steps, steps_total, K, T, max_iters, grad_tol, max_step, temperature, translate_amp,
                              rotate_amp, chi_amp, x_chains, energy_chains, energy_start, best_step, accepted, evaluations, trace_energy,
                              trace_entity, trace_accept, trace_iterations, trace_status};
    hipLaunchKernelGGL(vina_flex_search_kernel, dim3(P * K), dim3(NT), 6 * (size_t)(L + F) * sizeof(double), (hipStream_t)stream, t, x, ws,
                       a);
    return pd_check_launch();
}

PD_EXPORT int pd_vina_flex_search_select(const float* x, const int* mov_idx, const unsigned char* type, const unsigned char* fixed_mask,
                                         const unsigned char* active, const int* rot, const unsigned* rot_mask, const int* pair_start,
                                         const int* pair_atom, int n_pair, const int* excl_start, const int* excl_atom, int n_excl,
                                         const double* ws, long long ws_numel, int* best_chain, double* energy, double* inter,
                                         double* intra, double* receptor, float* x_search, double* moved, double* moved_flex, int P,
                                         int K, int A, int L, int F, int T, int S, void* stream) {
    const int rc = check_tables(x, mov_idx, type, fixed_mask, active, rot, rot_mask, pair_start, pair_atom, n_pair, excl_start, excl_atom,
                                n_excl, P, A, L, F, T, S);
    if (rc == PD_ERR_ARG) return rc;
    if (!ws || !best_chain || !energy || !x_search || !moved || K < 1) return PD_ERR_ARG;
    if (!aligned(ws, 8) || !aligned(best_chain, 4) || !aligned(energy, 8) || !aligned(inter, 8) || !aligned(intra, 8) ||
        !aligned(receptor, 8) || !aligned(x_search, 4) || !aligned(moved, 8) || !aligned(moved_flex, 8))
        return PD_ERR_ARG;
    if (rc != PD_OK) return rc;
    if (K > FS_MAX_K || (long long)P * K > FS_MAX_BLOCKS) return PD_ERR_UNSUPPORTED;
    if (ws_numel < pd_vina_flex_search_workspace_numel(P, K, L + F, T + S)) return PD_ERR_ARG;
    const FlexTab t = {mov_idx, type, fixed_mask, active, rot, rot_mask, pair_start, pair_atom, excl_start, excl_atom, A, L, L + F, T + S};
    const FlexSelectOut o = {best_chain, energy, inter, intra, receptor, x_search, moved, moved_flex};
    hipLaunchKernelGGL(vina_flex_search_select_kernel, dim3(P), dim3(NT), 6 * (size_t)(L + F) * sizeof(double), (hipStream_t)stream, t, x,
                       ws, K, o);
    return pd_check_launch();
}
