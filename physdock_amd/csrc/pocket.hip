// The empty space around the ligand of P poses of one system: how large is the pocket the model drew, how much of it does the ligand
// fill, which ligand atoms stick out into the solvent, and which residues line the site - without a ground truth.  The grid method
// of LIGSITE (Hendlich, Rippmann & Barnickel 1997) and POVME, heavy atoms only, recomputed for every pose because every pose carries
// its own receptor.  (physdock_amd/pocket.py builds the tables once per system; tests/pocket_ref.py is the written definition.)
// Caveat: the spacing, the probe, the lining distance, the reach and the enclosure threshold are this package's own defaults and
// have NOT BEEN VALIDATED on real complexes; volumes depend on them and on the lattice position - compare poses of one system.
//
// One system, over the A atoms of a pose: cls [A] (0 ignored, 1 receptor, 2 ligand: the byte of pd_buried_surface), radius [A] (A,
// fp32), lig_idx [L], the receptor atoms by residue res_start [R + 1] / res_atom [N].  h (fp32 spacing), n points per axis (8 .. 48),
// probe, lining (fp32), steps [7] and min_enclosed.
//   centre     given (fp32), or the float64 mean of the active ligand atoms (cls 2) summed in lig_idx order, rounded once to fp32;
//              with snap each coordinate c becomes fl32(h * rint(c / h)) in float64.  It is an output (centre_used).
//   lattice    o = centre - (h (n - 1)) / 2 in float64; point (i, j, k) is g = o + (i, j, k) h, linear index (i n + j) n + k
//   solid(g)   some receptor atom j has d(g, x_j) < radius_j + probe          (all predicates in float64 from the fp32 inputs:
//   inside(g)  some active ligand atom i has d(g, x_i) < radius_i              d = sqrt((dx dx + dy dy) + dz dz), no fused
//   near(g,j)  d(g, x_j) < radius_j + lining, j a receptor atom                multiply-add)
//   buried(g)  of the seven directions (1,0,0) (0,1,0) (0,0,1) (1,1,1) (1,1,-1) (1,-1,1) (-1,1,1) the number in which a solid
//              point lies within steps[d] lattice steps of g in the + sense AND in the - sense (leaving the lattice is no hit)
//   pocket     not solid and buried >= min_enclosed; pocket points form 6-connected components; a pocket point with inside is
//              occupied; the site is the union of the components that hold an occupied point
// Outputs per pose (include/physdock_hip.h lists them): classes, buried, counts [8], truncated, values [6], atom_class, atom_buried,
// lining_points [R], lining_residues, ok.  A pose with a non-finite coordinate in an atom of class != 0 or a non-finite centre has
// ok = 0, counts 0, floats NaN, bytes 255, truncated 0.
//
// The fp32 filter.  A predicate d < T is decided in fp32 only outside a guard band around T; inside it the pair is evaluated again
// in float64 in the order above, so the result IS the float64 predicate.  With u = 2^-24, E = h (n - 1) the lattice edge and all
// coordinates taken relative to o: an atom's relative coordinate is rounded once from float64 (error <= u |r|), a point's is
// fl(i h) (<= u |g|, |g| <= E), their difference adds u |d|; with |r| <= |g| + |d| the difference vector is off by at most
// sqrt(3) 2 u (E + d).  fmaf(dz, dz, fmaf(dy, dy, dx * dx)) carries three roundings: 1.5 u d on the distance.  T = fl(radius +
// margin) (u T), T -+ B (u T) and its square (u T / 2).  Near d = T the sum is below 3.5 u (E + T) + 4.5 u T < 8 u (E + T); the band
// is B = 16 u (E + T) = 2^-20 (E + T), twice that: 1.1e-5 A at n = 9, h = 1 and 4.8e-5 A at n = 48.  Further from T than B the error
// grows with 5 u per unit of distance only, so the fp32 decision stays right.  The launcher refuses E > 4096 A.
//
// pocket_setup_kernel     one block per pose: ok and the centre.
// pocket_classify_kernel  one block of 256 threads per (8 row-words of 32 points, pose): a thread owns one point.  Atoms stream
//                         through LDS in runs of 256; a run keeps the atoms within reach of the block's bounding sphere (a superset,
//                         (rb + T) (1 + 2^-13) + 0.01 A) by wave ballot and popcount.  Wave ballots give the solid and inside bit words.
// pocket_pose_kernel      one block of 1024 threads per pose: the solid bits in LDS, the 14 walks on bits, lock-free union-find
//                         (every root is the smallest index of its tree: one pass of unions, one of finds - a winding tunnel costs
//                         no sweeps), classes, counts, the per-atom values.
// pocket_lining_kernel    one wave per residue: the site points in the lattice box of its atoms.
// "Any" tests and integer sums only (integer atomics: minima in the union-find, one count); every float is one quotient or product
// of exact integers: results are bit-identical from run to run, whatever P is and wherever a pose sits.  No allocation.
#include "common.h"
#include "geom3.h"
#include "physdock_hip.h"

namespace {

constexpr int PK_MAX_L = 1024, PK_MAX_R = 4096, PK_MAX_P = 65535, PK_MAX_A = 1 << 22;
constexpr int PK_MAX_WORDS = PD_POCKET_MAX_N * PD_POCKET_MAX_N * 2;      // bit words of one mask at n = 48
constexpr int PK_POSE_THREADS = 1024, PK_POSE_WAVES = PK_POSE_THREADS / 64;
constexpr int PK_SUMS = 11;
constexpr float PK_BAND = 9.5367431640625e-07f;                          // 2^-20
constexpr float PK_REACH_REL = 1.0001220703125f, PK_REACH_ABS = 0.01f;   // 1 + 2^-13
constexpr float PK_MAX_EDGE = 4096.f;
static_assert(PD_POCKET_MIN_N == 8 && PD_POCKET_MAX_N == 48 && PD_POCKET_COUNTS == 8 && PD_POCKET_VALUES == 6, "the numbers the header documents");

__constant__ int PK_DIR[7][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 1}, {1, 1, -1}, {1, -1, 1}, {-1, 1, 1}};

struct PkSteps { int s[7]; };
struct PkLattice { double ox, oy, oz, h; };

__device__ __forceinline__ PkLattice pk_lattice(const float* c, float h, int n) {
    const double hd = (double)h, half = (hd * (double)(n - 1)) / 2.0;
    return {(double)c[0] - half, (double)c[1] - half, (double)c[2] - half, hd};
}
__device__ __forceinline__ float pk_dist2(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}
// the float64 predicate of the written definition: d(g, x_a) < T
__device__ bool pk_within(double gx, double gy, double gz, const float* xa, double T) {
#pragma clang fp contract(off)
    const double dx = gx - (double)xa[0], dy = gy - (double)xa[1], dz = gz - (double)xa[2];
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    return sqrt(d2) < T;
}
// the fp32 filter of one pair: s the fp32 squared distance, T the fp32 threshold, E the lattice edge; 1 in, 0 out, -1 inside the band
__device__ __forceinline__ int pk_filter(float s, float T, float E) {
    const float B = PK_BAND * (E + T), lo = T - B, hi = T + B;
    if (!(s < hi * hi)) return 0;
    return (lo > 0.f && s < lo * lo) ? 1 : -1;
}
__device__ __forceinline__ int pk_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void pk_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void pk_sync() {
    __threadfence();
    __syncthreads();
}
// union-find over the labels of the pocket points: a parent is never larger than its child, so a root is the smallest index of its tree
__device__ __forceinline__ int pk_find(const int* lab, int a) {
    for (int v; (v = pk_load(lab + a)) != a;) a = v;
    return a;
}
__device__ __forceinline__ void pk_union(int* lab, int a, int b) {
    for (;;) {
        a = pk_find(lab, a);
        b = pk_find(lab, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(lab + a, b);                       // a > b: a root takes the smaller root as its parent
        if (old == a) return;
        a = old;                                                     // a had been linked meanwhile: its former parent joins b
    }
}

__global__ __launch_bounds__(256) void pocket_setup_kernel(const float* __restrict__ x, const unsigned char* __restrict__ cls,
                                                          const int* __restrict__ lig_idx, const float* __restrict__ centre,
                                                          int centre_stride, int snap, float h, float* __restrict__ centre_used,
                                                          unsigned char* __restrict__ ok, int A, int L) {
    const int tid = threadIdx.x, p = blockIdx.x;
    const float* xp = x + (long long)p * A * 3;
    int good = 1;
    for (int a = tid; a < A; a += 256)
        if (cls[a] != 0 && !finite3(xp[3 * a], xp[3 * a + 1], xp[3 * a + 2])) good = 0;
    good = __syncthreads_and(good);
    if (tid != 0) return;
    double c[3];
    if (centre) {
        for (int d = 0; d < 3; ++d) c[d] = (double)centre[(long long)p * centre_stride + d];
    } else {
        double s[3] = {0.0, 0.0, 0.0};
        int cnt = 0;
        for (int q = 0; q < L; ++q) {                                // sequential, in lig_idx order
            const int a = lig_idx[q];
            if (cls[a] != 2) continue;
            s[0] += (double)xp[3 * a], s[1] += (double)xp[3 * a + 1], s[2] += (double)xp[3 * a + 2];
            ++cnt;
        }
        for (int d = 0; d < 3; ++d) c[d] = (double)(float)(s[d] / (double)cnt);      // no active atom: 0 / 0, a NaN centre
    }
    float out[3];
    for (int d = 0; d < 3; ++d) out[d] = snap ? (float)((double)h * rint(c[d] / (double)h)) : (float)c[d];
    const bool fine = good && finite3(out[0], out[1], out[2]);
    ok[p] = fine ? 1 : 0;
    for (int d = 0; d < 3; ++d) centre_used[3 * (long long)p + d] = fine ? out[d] : __int_as_float(0x7fc00000);
}

__global__ __launch_bounds__(256) void pocket_classify_kernel(const float* __restrict__ x, const unsigned char* __restrict__ cls,
                                                             const float* __restrict__ radius, const float* __restrict__ centre_used,
                                                             const unsigned char* __restrict__ ok, float h, float probe, int n, int A,
                                                             unsigned* __restrict__ solid_bits, unsigned* __restrict__ inside_bits) {
    __shared__ float ex[256], ey[256], ez[256], et[256];
    __shared__ int ea[256];                                          // the atom, its class in bit 30
    __shared__ int wcnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = blockIdx.y;
    if (!ok[p]) return;                                              // uniform over the block
    const float* xp = x + (long long)p * A * 3;
    const PkLattice lat = pk_lattice(centre_used + 3 * (long long)p, h, n);
    const int W = (n + 31) >> 5, nunits = n * n * W;
    const float E = h * (float)(n - 1);
    // the point of this thread
    const int unit = blockIdx.x * 8 + (tid >> 5), row = unit / W;
    const int pi = row / n, pj = row - pi * n, pk = (unit - row * W) * 32 + (tid & 31);
    const bool valid = unit < nunits && pk < n;
    const float gx = (float)pi * h, gy = (float)pj * h, gz = (float)pk * h;
    // the block's points lie in a box of the lattice: its centre and half diagonal, relative to o
    const int u0 = blockIdx.x * 8, u1 = min(u0 + 7, nunits - 1), r0 = u0 / W, r1 = u1 / W;
    const int i0 = r0 / n, i1 = r1 / n, j0 = i0 == i1 ? r0 - i0 * n : 0, j1 = i0 == i1 ? r1 - i1 * n : n - 1;
    const float bx = 0.5f * (float)(i0 + i1) * h, by = 0.5f * (float)(j0 + j1) * h, bz = 0.5f * E;
    const float di = (float)(i1 - i0), dj = (float)(j1 - j0), dk = (float)(n - 1);
    const float rb = 0.5f * h * sqrtf(di * di + dj * dj + dk * dk);
    bool solid = false, inside = false;
    for (int a0 = 0; a0 < A; a0 += 256) {
        const int a = a0 + tid;
        const int c = a < A ? cls[a] : 0;
        bool keep = false;
        float rx = 0.f, ry = 0.f, rz = 0.f, T = 0.f;
        if (c != 0) {
            rx = (float)((double)xp[3 * a] - lat.ox), ry = (float)((double)xp[3 * a + 1] - lat.oy), rz = (float)((double)xp[3 * a + 2] - lat.oz);
            T = c == 1 ? radius[a] + probe : radius[a];
            const float reach = fmaf(rb + T, PK_REACH_REL, PK_REACH_ABS);
            keep = pk_dist2(rx, ry, rz, bx, by, bz) < reach * reach;
        }
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) wcnt[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int v = wcnt[w];
            before += w < wave ? v : 0;
            total += v;
        }
        if (keep) {
            const int e = before + __popcll(mask & ((1ull << lane) - 1ull));          // e < total <= 256
            ex[e] = rx, ey[e] = ry, ez[e] = rz, et[e] = T;
            ea[e] = a | (c == 1 ? 1 << 30 : 0);
        }
        __syncthreads();                                             // the list is complete
        if (valid) {
            for (int e = 0; e < total; ++e) {
                const float T_e = et[e];
                const int f = pk_filter(pk_dist2(gx, gy, gz, ex[e], ey[e], ez[e]), T_e, E);
                if (f == 0) continue;
                const int ae = ea[e], atom = ae & ~(1 << 30);
                const bool rec = (ae >> 30) != 0;
                if (rec ? solid : inside) continue;
                bool hit = f > 0;
                if (f < 0) {                                         // inside the band: the float64 predicate itself
                    const double T64 = rec ? (double)radius[atom] + (double)probe : (double)radius[atom];
                    hit = pk_within(lat.ox + (double)pi * lat.h, lat.oy + (double)pj * lat.h, lat.oz + (double)pk * lat.h, xp + 3 * atom, T64);
                }
                if (hit) {
                    if (rec) solid = true;
                    else inside = true;
                }
            }
        }
        __syncthreads();                                             // the list may be written again
    }
    const unsigned long long ms = __ballot(valid && solid), mi = __ballot(valid && inside);
    if ((lane & 31) == 0 && unit < nunits) {
        const long long w = (long long)p * nunits + unit;
        solid_bits[w] = lane ? (unsigned)(ms >> 32) : (unsigned)ms;
        inside_bits[w] = lane ? (unsigned)(mi >> 32) : (unsigned)mi;
    }
}

__device__ __forceinline__ bool pk_bit(const unsigned* bits, int n, int W, int i, int j, int k) {
    return (bits[(i * n + j) * W + (k >> 5)] >> (k & 31)) & 1u;
}
// does a walk from (i, j, k) in steps of (dx, dy, dz) meet a solid point within S steps?  Leaving the lattice is no hit.
__device__ __forceinline__ bool pk_walk(const unsigned* sb, int n, int W, int i, int j, int k, int dx, int dy, int dz, int S) {
    for (int s = 1; s <= S; ++s) {
        i += dx, j += dy, k += dz;
        if ((unsigned)i >= (unsigned)n || (unsigned)j >= (unsigned)n || (unsigned)k >= (unsigned)n) return false;
        if (pk_bit(sb, n, W, i, j, k)) return true;
    }
    return false;
}

__global__ __launch_bounds__(PK_POSE_THREADS) void pocket_pose_kernel(
    const float* __restrict__ x, const unsigned char* __restrict__ cls, const int* __restrict__ lig_idx,
    const float* __restrict__ centre_used, const unsigned char* __restrict__ ok, float h, int n, PkSteps steps, int min_enclosed,
    int* __restrict__ labels, int* __restrict__ marks, const unsigned* __restrict__ solid_bits, const unsigned* __restrict__ inside_bits,
    unsigned char* __restrict__ classes, unsigned char* __restrict__ buried, int* __restrict__ counts, unsigned char* __restrict__ truncated,
    float* __restrict__ values, unsigned char* __restrict__ atom_class, unsigned char* __restrict__ atom_buried,
    int* __restrict__ lining_residues, int P, int A, int L) {
    __shared__ unsigned sb[PK_MAX_WORDS];
    __shared__ int red[PK_POSE_WAVES][PK_SUMS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = blockIdx.x;
    const int W = (n + 31) >> 5, nw = n * n * W, n2 = n * n, n3 = n2 * n;
    unsigned char* cl = classes + (long long)p * n3;
    unsigned char* bu = buried + (long long)p * n3;
    if (!ok[p]) {                                                    // uniform over the block
        for (int g = tid; g < n3; g += PK_POSE_THREADS) cl[g] = 255, bu[g] = 255;
        for (int s = tid; s < L; s += PK_POSE_THREADS) atom_class[(long long)p * L + s] = 255, atom_buried[(long long)p * L + s] = 255;
        if (tid < PD_POCKET_COUNTS) counts[(long long)p * PD_POCKET_COUNTS + tid] = 0;
        if (tid < PD_POCKET_VALUES) values[(long long)tid * P + p] = __int_as_float(0x7fc00000);
        if (tid == 0) truncated[p] = 0, lining_residues[p] = 0;
        return;
    }
    int* lab = labels + (long long)p * n3;
    int* mk = marks + (long long)p * n3;
    const unsigned* ib = inside_bits + (long long)p * nw;
    for (int w = tid; w < nw; w += PK_POSE_THREADS) sb[w] = solid_bits[(long long)p * nw + w];
    __syncthreads();
    // enclosure: 14 walks on the solid bits
    for (int g = tid; g < n3; g += PK_POSE_THREADS) {
        const int i = g / n2, j = (g - i * n2) / n, k = g - i * n2 - j * n;
        const bool solid = pk_bit(sb, n, W, i, j, k);
        int b = 0;
        if (!solid) {
#pragma unroll
            for (int d = 0; d < 7; ++d) {
                const int dx = PK_DIR[d][0], dy = PK_DIR[d][1], dz = PK_DIR[d][2], S = steps.s[d];
                if (pk_walk(sb, n, W, i, j, k, dx, dy, dz, S) && pk_walk(sb, n, W, i, j, k, -dx, -dy, -dz, S)) ++b;
            }
        }
        bu[g] = (unsigned char)b;
        pk_store(lab + g, !solid && b >= min_enclosed ? g : -1);
    }
    pk_sync();
    // components: a pocket point joins its pocket neighbours at -k, -j, -i
    for (int g = tid; g < n3; g += PK_POSE_THREADS) {
        if (pk_load(lab + g) < 0) continue;
        const int i = g / n2, j = (g - i * n2) / n, k = g - i * n2 - j * n;
        if (k > 0 && pk_load(lab + g - 1) >= 0) pk_union(lab, g, g - 1);
        if (j > 0 && pk_load(lab + g - n) >= 0) pk_union(lab, g, g - n);
        if (i > 0 && pk_load(lab + g - n2) >= 0) pk_union(lab, g, g - n2);
    }
    pk_sync();
    for (int g = tid; g < n3; g += PK_POSE_THREADS) {
        if (pk_load(lab + g) < 0) continue;
        const int r = pk_find(lab, g);
        pk_store(lab + g, r);                                        // any value a concurrent find reads here is an ancestor of g
        if (r == g) pk_store(mk + g, 0);
    }
    pk_sync();
    for (int g = tid; g < n3; g += PK_POSE_THREADS) {
        const int r = pk_load(lab + g);
        if (r < 0) continue;
        const int i = g / n2, j = (g - i * n2) / n, k = g - i * n2 - j * n;
        if (pk_bit(ib, n, W, i, j, k)) pk_store(mk + r, 1);          // an occupied point: its component belongs to the site
    }
    pk_sync();
    // classes and counts
    int sum[PK_SUMS];
#pragma unroll
    for (int q = 0; q < PK_SUMS; ++q) sum[q] = 0;
    for (int g = tid; g < n3; g += PK_POSE_THREADS) {
        const int i = g / n2, j = (g - i * n2) / n, k = g - i * n2 - j * n;
        const bool solid = pk_bit(sb, n, W, i, j, k), in = pk_bit(ib, n, W, i, j, k);
        const int r = pk_load(lab + g);
        const bool pocket = r >= 0, site = pocket && pk_load(mk + r) != 0, root = pocket && r == g;
        const bool face = i == 0 || j == 0 || k == 0 || i == n - 1 || j == n - 1 || k == n - 1;
        cl[g] = solid ? 0 : (!pocket ? 1 : (!site ? 2 : (in ? 4 : 3)));
        sum[0] += solid, sum[1] += !solid, sum[2] += pocket, sum[3] += site, sum[4] += site && in, sum[5] += !solid && in;
        sum[6] += root, sum[7] += root && site, sum[8] += site && face;
    }
    pk_sync();
    // the lattice point nearest each ligand atom
    const float* xp = x + (long long)p * A * 3;
    const PkLattice lat = pk_lattice(centre_used + 3 * (long long)p, h, n);
    for (int s = tid; s < L; s += PK_POSE_THREADS) {
        const int a = lig_idx[s];
        unsigned char ac = 255, ab = 255;
        if (cls[a] == 2) {
            const double qi = rint(((double)xp[3 * a] - lat.ox) / lat.h), qj = rint(((double)xp[3 * a + 1] - lat.oy) / lat.h),
                         qk = rint(((double)xp[3 * a + 2] - lat.oz) / lat.h), top = (double)(n - 1);
            if (qi >= 0.0 && qi <= top && qj >= 0.0 && qj <= top && qk >= 0.0 && qk <= top) {
                const int g = ((int)qi * n + (int)qj) * n + (int)qk;
                ac = cl[g], ab = bu[g];
                sum[9] += ab, sum[10] += 1;
            }
        }
        atom_class[(long long)p * L + s] = ac;
        atom_buried[(long long)p * L + s] = ab;
    }
#pragma unroll
    for (int q = 0; q < PK_SUMS; ++q) {
        const int v = wave_sum(sum[q]);
        if (lane == 0) red[wave][q] = v;
    }
    __syncthreads();
    if (tid == 0) {
        int t[PK_SUMS];
        for (int q = 0; q < PK_SUMS; ++q) {
            t[q] = 0;
            for (int w = 0; w < PK_POSE_WAVES; ++w) t[q] += red[w][q];
        }
        for (int q = 0; q < PD_POCKET_COUNTS; ++q) counts[(long long)p * PD_POCKET_COUNTS + q] = t[q];
        truncated[p] = t[8] > 0 ? 1 : 0;
        lining_residues[p] = 0;                                      // pocket_lining_kernel counts into it
        const double h3 = (lat.h * lat.h) * lat.h;
        const int n_pocket = t[2], n_site = t[3], n_occ = t[4], n_lig = t[5];
        values[0 * (long long)P + p] = (float)((double)n_site * h3);
        values[1 * (long long)P + p] = (float)((double)(n_site - n_occ) * h3);
        values[2 * (long long)P + p] = (float)((double)n_pocket * h3);
        values[3 * (long long)P + p] = n_site > 0 ? (float)((double)n_occ / (double)n_site) : 0.f;
        values[4 * (long long)P + p] = n_lig > 0 ? (float)((double)n_occ / (double)n_lig) : 0.f;
        values[5 * (long long)P + p] = t[10] > 0 ? (float)((double)t[9] / (double)(7 * t[10])) : 0.f;
    }
}

__global__ __launch_bounds__(256) void pocket_lining_kernel(const float* __restrict__ x, const float* __restrict__ radius,
                                                           const int* __restrict__ res_start, const int* __restrict__ res_atom,
                                                           const float* __restrict__ centre_used, const unsigned char* __restrict__ ok,
                                                           float h, int n, float lining, const unsigned char* __restrict__ classes,
                                                           int* __restrict__ lining_points, int* __restrict__ lining_residues, int A,
                                                           int R) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = blockIdx.x;
    const bool fine = ok[p] != 0;                                    // uniform over the block
    const float* xp = x + (long long)p * A * 3;
    const int n2 = n * n, n3 = n2 * n;
    const unsigned char* cl = classes + (long long)p * n3;
    const float E = h * (float)(n - 1);
    PkLattice lat = {0.0, 0.0, 0.0, (double)h};
    if (fine) lat = pk_lattice(centre_used + 3 * (long long)p, h, n);
    for (int r = blockIdx.y * 4 + wave; r < R; r += gridDim.y * 4) {                 // uniform over the wave
        const int start = res_start[r], end = res_start[r + 1];
        int count = 0;
        if (fine && end > start) {
            // the lattice box that holds every point within reach of an atom of the residue, one spacing to spare
            double lo[3] = {(double)n, (double)n, (double)n}, hi[3] = {-1.0, -1.0, -1.0};
            for (int q = start + lane; q < end; q += 64) {
                const int a = res_atom[q];
                const double t = ((double)radius[a] + (double)lining) + lat.h;
                const double c[3] = {(double)xp[3 * a] - lat.ox, (double)xp[3 * a + 1] - lat.oy, (double)xp[3 * a + 2] - lat.oz};
                double l[3], u[3];
                bool some = true;
                for (int d = 0; d < 3; ++d) {
                    l[d] = fmin(fmax(floor((c[d] - t) / lat.h), 0.0), (double)n);
                    u[d] = fmax(fmin(ceil((c[d] + t) / lat.h), (double)(n - 1)), -1.0);
                    some = some && l[d] <= u[d];
                }
                if (some)
                    for (int d = 0; d < 3; ++d) lo[d] = fmin(lo[d], l[d]), hi[d] = fmax(hi[d], u[d]);
            }
            int b0[3], ext[3];
            for (int d = 0; d < 3; ++d) {
                b0[d] = (int)wave_min(lo[d]);
                ext[d] = max((int)wave_max(hi[d]) - b0[d] + 1, 0);
            }
            const int box = ext[0] * ext[1] * ext[2];                // at most n^3
            for (int q = lane; q < box; q += 64) {
                const int qi = q / (ext[1] * ext[2]), qj = (q - qi * ext[1] * ext[2]) / ext[2], qk = q - qi * ext[1] * ext[2] - qj * ext[2];
                const int i = b0[0] + qi, j = b0[1] + qj, k = b0[2] + qk;
                const unsigned char c = cl[(i * n + j) * n + k];
                if (c != 3 && c != 4) continue;                      // not a site point
                const float gx = (float)i * h, gy = (float)j * h, gz = (float)k * h;
                bool near = false;
                for (int e = start; e < end && !near; ++e) {
                    const int a = res_atom[e];
                    const float T = radius[a] + lining;
                    const float rx = (float)((double)xp[3 * a] - lat.ox), ry = (float)((double)xp[3 * a + 1] - lat.oy),
                                rz = (float)((double)xp[3 * a + 2] - lat.oz);
                    const int f = pk_filter(pk_dist2(gx, gy, gz, rx, ry, rz), T, E);
                    if (f > 0) near = true;
                    else if (f < 0)
                        near = pk_within(lat.ox + (double)i * lat.h, lat.oy + (double)j * lat.h, lat.oz + (double)k * lat.h, xp + 3 * a,
                                         (double)radius[a] + (double)lining);
                }
                count += near ? 1 : 0;
            }
            count = wave_sum(count);
        }
        if (lane == 0) {
            lining_points[(long long)p * R + r] = count;
            if (count > 0) atomicAdd(lining_residues + p, 1);
        }
    }
}

}  // namespace

PD_EXPORT long long pd_pocket_grid_workspace_numel(int P, int n, int A) {
    if (P <= 0 || A <= 0) return PD_ERR_ARG;
    if (n < PD_POCKET_MIN_N || n > PD_POCKET_MAX_N || P > PK_MAX_P || A > PK_MAX_A) return PD_ERR_UNSUPPORTED;
    const long long W = (n + 31) >> 5;
    return (long long)P * (2ll * n * n * n + 2ll * n * n * W);
}

PD_EXPORT int pd_pocket_grid(const float* x, const unsigned char* cls, const float* radius, const int* lig_idx, const int* res_start,
                             const int* res_atom, const float* centre, int centre_stride, int snap, float h, int n, float probe,
                             float lining, const int* steps, int min_enclosed, int* ws, long long ws_numel, float* centre_used,
                             unsigned char* ok, unsigned char* classes, unsigned char* buried, int* counts, unsigned char* truncated,
                             float* values, unsigned char* atom_class, unsigned char* atom_buried, int* lining_points,
                             int* lining_residues, int P, int A, int L, int R, int N, void* stream) {
    if (!x || !cls || !radius || !lig_idx || !res_start || !steps || !ws || !centre_used || !ok || !classes || !buried || !counts ||
        !truncated || !values || !atom_class || !atom_buried || !lining_points || !lining_residues)
        return PD_ERR_ARG;
    if (P <= 0 || A <= 0 || L <= 0 || R <= 0 || N < 0 || N > A) return PD_ERR_ARG;
    if (N > 0 && !res_atom) return PD_ERR_ARG;
    if (centre && centre_stride != 0 && centre_stride != 3) return PD_ERR_ARG;
    if (!(h > 0.f) || !(h <= 3.0e38f) || !(probe >= 0.f) || !(probe <= 3.0e38f) || !(lining >= 0.f) || !(lining <= 3.0e38f))
        return PD_ERR_ARG;                                                                        // negative, NaN or infinite
    if (min_enclosed < 0 || min_enclosed > 7) return PD_ERR_ARG;
    PkSteps st;
    for (int d = 0; d < 7; ++d) {
        if (steps[d] < 0) return PD_ERR_ARG;
        st.s[d] = steps[d];
    }
    if (pd_misaligned(x, 4) || pd_misaligned(radius, 4) || pd_misaligned(lig_idx, 4) || pd_misaligned(res_start, 4) ||
        pd_misaligned(res_atom, 4) || pd_misaligned(centre, 4) || pd_misaligned(ws, 4) || pd_misaligned(centre_used, 4) ||
        pd_misaligned(counts, 4) || pd_misaligned(values, 4) || pd_misaligned(lining_points, 4) || pd_misaligned(lining_residues, 4))
        return PD_ERR_ARG;
    if (n < PD_POCKET_MIN_N || n > PD_POCKET_MAX_N || L > PK_MAX_L || R > PK_MAX_R || P > PK_MAX_P || A > PK_MAX_A)
        return PD_ERR_UNSUPPORTED;
    if (h * (float)(n - 1) > PK_MAX_EDGE) return PD_ERR_UNSUPPORTED;
    if (ws_numel < pd_pocket_grid_workspace_numel(P, n, A)) return PD_ERR_ARG;
    for (int d = 0; d < 7; ++d) st.s[d] = st.s[d] < n ? st.s[d] : n;                              // a longer walk has left the lattice
    const int W = (n + 31) >> 5, nw = n * n * W;
    const long long n3 = (long long)n * n * n;
    int* labels = ws;
    int* marks = ws + (long long)P * n3;
    unsigned* solid_bits = (unsigned*)(ws + 2ll * P * n3);
    unsigned* inside_bits = solid_bits + (long long)P * nw;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pocket_setup_kernel, dim3(P), dim3(256), 0, s, x, cls, lig_idx, centre, centre_stride, snap, h, centre_used, ok, A,
                       L);
    hipLaunchKernelGGL(pocket_classify_kernel, dim3((nw + 7) / 8, P), dim3(256), 0, s, x, cls, radius, (const float*)centre_used,
                       (const unsigned char*)ok, h, probe, n, A, solid_bits, inside_bits);
    hipLaunchKernelGGL(pocket_pose_kernel, dim3(P), dim3(PK_POSE_THREADS), 0, s, x, cls, lig_idx, (const float*)centre_used,
                       (const unsigned char*)ok, h, n, st, min_enclosed, labels, marks, (const unsigned*)solid_bits,
                       (const unsigned*)inside_bits, classes, buried, counts, truncated, values, atom_class, atom_buried, lining_residues,
                       P, A, L);
    const int ry = (R + 3) / 4 < 64 ? (R + 3) / 4 : 64;
    hipLaunchKernelGGL(pocket_lining_kernel, dim3(P, ry), dim3(256), 0, s, x, radius, res_start, res_atom, (const float*)centre_used,
                       (const unsigned char*)ok, h, n, lining, (const unsigned char*)classes, lining_points, lining_residues, A, R);
    return pd_check_launch();
}
