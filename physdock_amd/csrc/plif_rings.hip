// Ring interactions of P poses of one ligand in its receptor: pi-stacking, pi-cation and halogen bonds per residue - the kinds the
// fingerprint of plif.hip leaves out because they need ring centroids and normals.  (physdock_amd/ring_interactions.py builds the
// tables once per system; the same definition stands in its docstring and, as float64 numpy, in tests/plif_rings_ref.py.)
//
// Tables.  lig_idx, lig_active, type, charge, res_start and res_atom are those of pd_plif_fingerprint: the receptor's CATION atoms
// (charge bit 0) and ACCEPTOR atoms (type bit 6) are the entries of res_atom that carry the bit.  Rings as a CSR over pose atoms:
// ring g is ring_atom[ring_start[g] .. ring_start[g + 1]) in cyclic order, 3 .. 8 atoms; the ligand's G_l rings first
// (ring_residue = -1), then the receptor's G_r rings IN ASCENDING ORDER OF ring_residue, the residue id a ring belongs to.
// halogen [H][2]: ligand-local indices (X, C) of a Cl, Br or I and the carbon it is bonded to.
//
// Ring frame of a pose, in double from the fp32 coordinates:
//   centroid  c = (a_0 + ... + a_{k-1}) / k           (summed in list order, one division per coordinate)
//   normal    N = sum_i (a_i - c) x (a_{i+1} - c), indices mod k;  n = N / |N|
// A ring with |N| zero or not finite, with a coordinate that is not finite, with fewer than 3 or more than 8 atoms or with an atom
// index outside 0 .. A - 1 is degenerate: it takes part in nothing and reports n = 0.  The sign of n is never looked at, only
// |n . m| and squares: no byte changes when a ring's list is rotated or reversed.
//
// Five kinds; bit k of a byte stands for kind k.  thresholds: EIGHT doubles ON THE HOST - five distances (A), then three cosines:
//   bit  kind          between                                  condition
//   0    pi_parallel   ligand ring g, receptor ring h           d = |c_g - c_h| < t[0] (5.5); min(off_gh, off_hg) < t[1] (2.0);
//                                                               |n_g . n_h| > t[5] (cos 30)
//   1    pi_tshaped    the same                                 the same distance and offset; |n_g . n_h| < t[6] (cos 60)
//   2    pi_cation     ligand ring g, receptor CATION atom j    |x_j - c_g| < t[2] (6.0); offset of x_j on the plane of g < t[3] (2.0)
//   3    cation_pi     active ligand CATION atom i, rec. ring h the same with the roles swapped
//   4    halogen_bond  active ligand halogen X with carbon C,   |x_X - x_j| < t[4] (4.0); cos(C - X ... j) < t[7] (cos 135)
//                      receptor ACCEPTOR atom j
// off_gh = sqrt(max(0, d^2 - ((c_h - c_g) . n_g)^2)): the distance from c_g to the projection of c_h onto the plane of g; the offset
// of a point is the same with the point in place of c_h.  Every condition is a comparison of doubles and is false for a NaN: no NaN
// reaches a byte.  Bits 5 - 7 are always 0.  No trigonometric function is called.
//
//   bits[p][s]               OR over the residue's rings (bits 0, 1, 3), cations (bit 2) and acceptors (bit 4)
//   ligand_bits[p][i]        OR per ligand atom: the bytes of the rings it is in, bit 3 for a cation, bit 4 for a halogen X; an
//                            inactive atom stores 0
//   ring_bits[p][g]          OR per ligand ring (bits 0, 1, 2)
//   centroid, normal [p][g]  the frames, ligand rings first
//   min_centroid_dist[p][s]  the exact minimum in double of d over (ligand ring, ring of residue s), both not degenerate, rounded
//                            once to fp32; +inf when there is no such pair
//   counts[p][k]             the number of residues whose byte has bit k
//
// Four launches; every pair is visited twice, once per side.  plif_rings_frame_kernel: one thread per (ring, pose), FRAME_BLOCK
// rings per block.  plif_rings_receptor_kernel: one thread per (receptor entity, pose) - the G_r rings, then the N entries of
// res_atom -, RECEPTOR_BLOCK per block; the ligand's ring frames, atoms and halogens are staged in LDS (19 KB) and walked in
// ascending order; a byte per entity and a minimum per ring go to the workspace.  plif_rings_ligand_kernel: one wave per (ligand
// entity, pose) - the G_l rings, the L atoms (only an active cation does work), the H halogens - striding the receptor's rings or
// list entries, OR butterfly.  plif_rings_fold_kernel: one wave per pose folds the workspace by residue (a residue's rings by
// binary search in ring_residue) and by ligand atom and counts the kinds.  No atomics, no scratch memory; only OR, exact minima and
// integer sums are reduced, so the order does not matter; every value depends on its own pose alone and on no launch dimension:
// results are bit-identical from run to run, whatever P is and wherever a pose sits.  No allocation, no synchronisation.
#include "common.h"
#include "geom3.h"
#include "physdock_hip.h"

namespace {

constexpr int RINGS_MAX_L = 1024;
constexpr int RINGS_MAX_A = 1 << 22;
constexpr int RINGS_MAX_P = 65535;
constexpr int RINGS_MAX_GL = 64;
constexpr int RINGS_MAX_GR = 4096;
constexpr int RINGS_MAX_H = 64;
constexpr int RINGS_MAX_SIZE = 8;
constexpr int FRAME_BLOCK = 64;
constexpr int RECEPTOR_BLOCK = 256;
constexpr int LIGAND_BLOCK = 64;              // one wave: the OR butterfly needs no LDS
constexpr int FOLD_BLOCK = 64;
constexpr unsigned CATION_BIT = 1u, ACCEPTOR_BIT = 64u;
static_assert(PD_PLIF_RING_KINDS == 5 && PD_PLIF_RING_THRESHOLDS == 8, "the counts the header documents");

struct RingThresholds {
    double stack_dist, stack_offset, pication_dist, pication_offset, halogen_dist, cos_parallel, cos_t, cos_halogen;
};

// a degenerate ring reports the normal 0
__device__ __forceinline__ bool ring_ok(Vec3 n) { return dot(n, n) > 0.5; }

// bits 0 and 1 of two rings that are not degenerate; d: their centroid distance
__device__ __forceinline__ unsigned ring_ring(Vec3 cg, Vec3 ng, Vec3 ch, Vec3 nh, const RingThresholds& t, double& d) {
    const Vec3 v = sub(ch, cg);
    const double d2 = dot(v, v), pg = dot(v, ng), ph = dot(v, nh);
    d = sqrt(d2);
    const double off = fmin(sqrt(fmax(0.0, d2 - pg * pg)), sqrt(fmax(0.0, d2 - ph * ph)));
    const double c = fabs(dot(ng, nh));
    if (!(d < t.stack_dist && off < t.stack_offset)) return 0u;
    return (c > t.cos_parallel ? 1u : 0u) | (c < t.cos_t ? 2u : 0u);
}
// a ring that is not degenerate and a point: within pication_dist of the centroid and pication_offset of the axis?
__device__ __forceinline__ bool ring_point(Vec3 c, Vec3 n, Vec3 x, const RingThresholds& t) {
    const Vec3 v = sub(x, c);
    const double d2 = dot(v, v), p = dot(v, n);
    return sqrt(d2) < t.pication_dist && sqrt(fmax(0.0, d2 - p * p)) < t.pication_offset;
}
// halogen X with its carbon C and an acceptor at j
__device__ __forceinline__ bool halogen_bond(Vec3 X, Vec3 Cc, Vec3 j, const RingThresholds& t) {
    const Vec3 u = sub(Cc, X), w = sub(j, X);
    const double d2 = dot(w, w);
    return sqrt(d2) < t.halogen_dist && dot(u, w) / sqrt(dot(u, u) * d2) < t.cos_halogen;
}

__global__ __launch_bounds__(FRAME_BLOCK) void plif_rings_frame_kernel(const float* __restrict__ x, const int* __restrict__ ring_start,
                                                                      const int* __restrict__ ring_atom, double* __restrict__ centroid,
                                                                      double* __restrict__ normal, int A, int G) {
    const int g = blockIdx.x * FRAME_BLOCK + threadIdx.x, p = blockIdx.y;
    if (g >= G) return;
    const float* xp = x + (long long)p * A * 3;
    const int b = ring_start[g], k = ring_start[g + 1] - b;
    double* co = centroid + ((long long)p * G + g) * 3;
    double* no = normal + ((long long)p * G + g) * 3;
    bool ok = k >= 3 && k <= RINGS_MAX_SIZE;
    for (int i = 0; ok && i < k; ++i) {
        const int a = ring_atom[b + i];
        ok = a >= 0 && a < A;
    }
    Vec3 c = {0.0, 0.0, 0.0}, N = {0.0, 0.0, 0.0};
    if (ok) {
        bool finite = true;
        for (int i = 0; i < k; ++i) {
            const Vec3 a = load3(xp + 3 * ring_atom[b + i]);
            finite = finite && isfinite(a.x) && isfinite(a.y) && isfinite(a.z);
            c = i == 0 ? a : Vec3{c.x + a.x, c.y + a.y, c.z + a.z};
        }
        c = {c.x / k, c.y / k, c.z / k};
        Vec3 r = sub(load3(xp + 3 * ring_atom[b]), c);
        for (int i = 0; i < k; ++i) {
            const Vec3 s = sub(load3(xp + 3 * ring_atom[b + (i + 1 == k ? 0 : i + 1)]), c);
            N = {N.x + (r.y * s.z - r.z * s.y), N.y + (r.z * s.x - r.x * s.z), N.z + (r.x * s.y - r.y * s.x)};
            r = s;
        }
        const double len = sqrt(dot(N, N));
        ok = finite && isfinite(len) && len > 0.0;
        if (ok) N = {N.x / len, N.y / len, N.z / len};
    }
    co[0] = c.x; co[1] = c.y; co[2] = c.z;
    no[0] = ok ? N.x : 0.0; no[1] = ok ? N.y : 0.0; no[2] = ok ? N.z : 0.0;
}

__global__ __launch_bounds__(RECEPTOR_BLOCK) void plif_rings_receptor_kernel(
    const float* __restrict__ x, const int* __restrict__ lig_idx, const unsigned char* __restrict__ type,
    const unsigned char* __restrict__ charge, const unsigned char* __restrict__ lig_active, const int* __restrict__ res_atom,
    const int* __restrict__ halogen, const double* __restrict__ centroid, const double* __restrict__ normal, RingThresholds thr,
    unsigned char* __restrict__ ws_ring_bits, double* __restrict__ ws_ring_min, unsigned char* __restrict__ ws_atom_bits, int A, int L, int N,
    int G_l, int G_r, int H) {
    __shared__ double lc[RINGS_MAX_GL * 3], ln[RINGS_MAX_GL * 3];   // the ligand's ring frames
    __shared__ float lx[RINGS_MAX_L * 3];                           // the ligand's atoms
    __shared__ float hx[RINGS_MAX_H * 6];                           // halogen X, then its carbon
    __shared__ unsigned char lcat[RINGS_MAX_L], hok[RINGS_MAX_H];   // 1: an active cation / a halogen that takes part
    const int tid = threadIdx.x, p = blockIdx.y, e = blockIdx.x * RECEPTOR_BLOCK + tid, G = G_l + G_r;
    const float* xp = x + (long long)p * A * 3;
    const double* cp = centroid + (long long)p * G * 3;
    const double* np = normal + (long long)p * G * 3;
    for (int i = tid; i < G_l * 3; i += RECEPTOR_BLOCK) {
        lc[i] = cp[i];
        ln[i] = np[i];
    }
    for (int i = tid; i < L; i += RECEPTOR_BLOCK) {
        const int a = lig_idx[i];
        lx[3 * i] = xp[3 * a];
        lx[3 * i + 1] = xp[3 * a + 1];
        lx[3 * i + 2] = xp[3 * a + 2];
        lcat[i] = (lig_active[i] && (charge[a] & CATION_BIT)) ? 1 : 0;
    }
    for (int h = tid; h < H; h += RECEPTOR_BLOCK) {
        const int X = halogen[2 * h], Cc = halogen[2 * h + 1];
        const bool ok = X >= 0 && X < L && Cc >= 0 && Cc < L && lig_active[X];
        const int ax = ok ? lig_idx[X] : 0, ac = ok ? lig_idx[Cc] : 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            hx[6 * h + k] = xp[3 * ax + k];
            hx[6 * h + 3 + k] = xp[3 * ac + k];
        }
        hok[h] = ok ? 1 : 0;
    }
    __syncthreads();
    if (e >= G_r + N) return;
    if (e < G_r) {                                                   // a receptor ring: stacks with the ligand's rings, cation_pi
        const Vec3 ch = load3(cp + 3 * (G_l + e)), nh = load3(np + 3 * (G_l + e));
        unsigned b = 0;
        double m = INFINITY;
        if (ring_ok(nh)) {
            for (int g = 0; g < G_l; ++g) {                          // every thread reads the same LDS words: a broadcast
                const Vec3 ng = load3(ln + 3 * g);
                if (!ring_ok(ng)) continue;
                double d;
                b |= ring_ring(load3(lc + 3 * g), ng, ch, nh, thr, d);
                m = fmin(m, d);
            }
            for (int i = 0; i < L; ++i)
                if (lcat[i] && ring_point(ch, nh, load3(lx + 3 * i), thr)) b |= 8u;
        }
        ws_ring_bits[(long long)p * G_r + e] = (unsigned char)b;
        ws_ring_min[(long long)p * G_r + e] = m;
        return;
    }
    const int n = e - G_r, j = res_atom[n];                          // an entry of the receptor list: pi_cation, halogen_bond
    const Vec3 xj = load3(xp + 3 * j);
    unsigned b = 0;
    if (charge[j] & CATION_BIT)
        for (int g = 0; g < G_l; ++g) {
            const Vec3 ng = load3(ln + 3 * g);
            if (ring_ok(ng) && ring_point(load3(lc + 3 * g), ng, xj, thr)) b |= 4u;
        }
    if (type[j] & ACCEPTOR_BIT)
        for (int h = 0; h < H; ++h)
            if (hok[h] && halogen_bond(load3(hx + 6 * h), load3(hx + 6 * h + 3), xj, thr)) b |= 16u;
    ws_atom_bits[(long long)p * N + n] = (unsigned char)b;
}

__global__ __launch_bounds__(LIGAND_BLOCK) void plif_rings_ligand_kernel(
    const float* __restrict__ x, const int* __restrict__ lig_idx, const unsigned char* __restrict__ type,
    const unsigned char* __restrict__ charge, const unsigned char* __restrict__ lig_active, const int* __restrict__ res_atom,
    const int* __restrict__ halogen, const double* __restrict__ centroid, const double* __restrict__ normal, RingThresholds thr,
    unsigned char* __restrict__ ring_bits, unsigned char* __restrict__ ws_cation_bits, unsigned char* __restrict__ ws_halogen_bits, int A,
    int L, int N, int G_l, int G_r, int H) {
    const int tid = threadIdx.x, e = blockIdx.x, p = blockIdx.y, G = G_l + G_r;
    const float* xp = x + (long long)p * A * 3;
    const double* cp = centroid + (long long)p * G * 3;
    const double* np = normal + (long long)p * G * 3;
    int b = 0;
    if (e < G_l) {                                                   // a ligand ring (every branch here is uniform over the block)
        const Vec3 cg = load3(cp + 3 * e), ng = load3(np + 3 * e);
        if (ring_ok(ng)) {
            for (int h = tid; h < G_r; h += LIGAND_BLOCK) {
                const Vec3 nh = load3(np + 3 * (G_l + h));
                if (!ring_ok(nh)) continue;
                double d;
                b |= (int)ring_ring(cg, ng, load3(cp + 3 * (G_l + h)), nh, thr, d);
            }
            for (int n = tid; n < N; n += LIGAND_BLOCK) {
                const int j = res_atom[n];
                if ((charge[j] & CATION_BIT) && ring_point(cg, ng, load3(xp + 3 * j), thr)) b |= 4;
            }
        }
        b = wave_or(b);
        if (tid == 0) ring_bits[(long long)p * G_l + e] = (unsigned char)b;
    } else if (e < G_l + L) {                                        // a ligand atom: cation_pi
        const int i = e - G_l, a = lig_idx[i];
        if (lig_active[i] && (charge[a] & CATION_BIT)) {
            const Vec3 xi = load3(xp + 3 * a);
            for (int h = tid; h < G_r; h += LIGAND_BLOCK) {
                const Vec3 nh = load3(np + 3 * (G_l + h));
                if (ring_ok(nh) && ring_point(load3(cp + 3 * (G_l + h)), nh, xi, thr)) b |= 8;
            }
        }
        b = wave_or(b);
        if (tid == 0) ws_cation_bits[(long long)p * L + i] = (unsigned char)b;
    } else {                                                         // a halogen
        const int h = e - G_l - L, X = halogen[2 * h], Cc = halogen[2 * h + 1];
        if (X >= 0 && X < L && Cc >= 0 && Cc < L && lig_active[X]) {
            const Vec3 xx = load3(xp + 3 * lig_idx[X]), xc = load3(xp + 3 * lig_idx[Cc]);
            for (int n = tid; n < N; n += LIGAND_BLOCK) {
                const int j = res_atom[n];
                if ((type[j] & ACCEPTOR_BIT) && halogen_bond(xx, xc, load3(xp + 3 * j), thr)) b |= 16;
            }
        }
        b = wave_or(b);
        if (tid == 0) ws_halogen_bits[(long long)p * H + h] = (unsigned char)b;
    }
}

__global__ __launch_bounds__(FOLD_BLOCK) void plif_rings_fold_kernel(
    const int* __restrict__ lig_idx, const unsigned char* __restrict__ lig_active, const int* __restrict__ res_start,
    const int* __restrict__ ring_start, const int* __restrict__ ring_atom, const int* __restrict__ ring_residue,
    const int* __restrict__ halogen, const unsigned char* __restrict__ ws_ring_bits, const double* __restrict__ ws_ring_min,
    const unsigned char* __restrict__ ws_atom_bits, const unsigned char* __restrict__ ws_cation_bits,
    const unsigned char* __restrict__ ws_halogen_bits, const unsigned char* __restrict__ ring_bits, unsigned char* __restrict__ bits,
    unsigned char* __restrict__ ligand_bits, float* __restrict__ min_centroid_dist, int* __restrict__ counts, int L, int R, int N, int G_l,
    int G_r, int H) {
    const int tid = threadIdx.x, p = blockIdx.x;
    const unsigned char* wa = ws_atom_bits + (long long)p * N;
    const unsigned char* wr = ws_ring_bits + (long long)p * G_r;
    const double* wm = ws_ring_min + (long long)p * G_r;
    const int* rr = ring_residue + G_l;                              // the receptor's rings, ascending in the residue
    int cnt[PD_PLIF_RING_KINDS] = {0, 0, 0, 0, 0};
    for (int s = tid; s < R; s += FOLD_BLOCK) {
        unsigned b = 0;
        double m = INFINITY;
        for (int n = res_start[s], end = res_start[s + 1]; n < end; ++n) b |= wa[n];
        int lo = 0, hi = G_r;                                        // the first ring whose residue is not below s
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (rr[mid] < s) lo = mid + 1; else hi = mid;
        }
        for (int h = lo; h < G_r && rr[h] == s; ++h) {
            b |= wr[h];
            m = fmin(m, wm[h]);
        }
        bits[(long long)p * R + s] = (unsigned char)b;
        min_centroid_dist[(long long)p * R + s] = (float)m;
#pragma unroll
        for (int k = 0; k < PD_PLIF_RING_KINDS; ++k) cnt[k] += (int)((b >> k) & 1u);
    }
#pragma unroll
    for (int k = 0; k < PD_PLIF_RING_KINDS; ++k) {
        const int s = wave_sum(cnt[k]);
        if (tid == k) counts[p * PD_PLIF_RING_KINDS + k] = s;
    }
    for (int i = tid; i < L; i += FOLD_BLOCK) {
        unsigned b = 0;
        if (lig_active[i]) {
            const int a = lig_idx[i];
            b = ws_cation_bits[(long long)p * L + i];
            for (int g = 0; g < G_l; ++g)
                for (int q = ring_start[g], end = ring_start[g + 1]; q < end; ++q)
                    if (ring_atom[q] == a) b |= ring_bits[(long long)p * G_l + g];
            for (int h = 0; h < H; ++h)
                if (halogen[2 * h] == i) b |= ws_halogen_bits[(long long)p * H + h];
        }
        ligand_bits[(long long)p * L + i] = (unsigned char)b;
    }
}

inline bool misaligned4(const void* a) { return ((uintptr_t)a & 3) != 0; }
inline bool misaligned8(const void* a) { return ((uintptr_t)a & 7) != 0; }

// the workspace: ws_ring_min double [P][G_r], then the bytes ws_ring_bits [P][G_r], ws_atom_bits [P][N], ws_cation_bits [P][L],
// ws_halogen_bits [P][H]; rounded up to a multiple of 8
inline long long workspace_bytes_of(long long P, long long L, long long N, long long G_r, long long H) {
    return (P * (9 * G_r + N + L + H) + 7) / 8 * 8;
}

}  // namespace

PD_EXPORT int pd_plif_rings_workspace(int P, int L, int N, int G_l, int G_r, int H) {
    if (P <= 0 || L <= 0 || N < 0 || G_l < 0 || G_r < 0 || H < 0) return PD_ERR_ARG;
    const long long bytes = workspace_bytes_of(P, L, N, G_r, H);
    return bytes > 0x7fffffffLL ? PD_ERR_UNSUPPORTED : (int)bytes;
}

PD_EXPORT int pd_plif_rings(const float* x, const int* lig_idx, const unsigned char* type, const unsigned char* charge,
                            const unsigned char* lig_active, const int* res_start, const int* res_atom, const int* ring_start,
                            const int* ring_atom, const int* ring_residue, int G_l, int G_r, const int* halogen, int H,
                            const double* thresholds, void* workspace, size_t workspace_bytes, unsigned char* bits,
                            unsigned char* ligand_bits, unsigned char* ring_bits, double* centroid, double* normal,
                            float* min_centroid_dist, int* counts, int P, int A, int L, int R, int N, void* stream) {
    if (!x || !lig_idx || !type || !charge || !lig_active || !res_start || !thresholds || !workspace || !bits || !ligand_bits ||
        !min_centroid_dist || !counts)
        return PD_ERR_ARG;
    if (P <= 0 || A <= 0 || L <= 0 || R <= 0 || N < 0 || N > A || G_l < 0 || G_r < 0 || H < 0) return PD_ERR_ARG;
    const long long G = (long long)G_l + G_r;
    if (N > 0 && !res_atom) return PD_ERR_ARG;
    if (G > 0 && (!ring_start || !ring_atom || !ring_residue || !centroid || !normal)) return PD_ERR_ARG;
    if (G_l > 0 && !ring_bits) return PD_ERR_ARG;
    if (H > 0 && !halogen) return PD_ERR_ARG;
    if (misaligned4(x) || misaligned4(lig_idx) || misaligned4(res_start) || misaligned4(res_atom) || misaligned4(ring_start) ||
        misaligned4(ring_atom) || misaligned4(ring_residue) || misaligned4(halogen) || misaligned4(min_centroid_dist) ||
        misaligned4(counts) || misaligned8(thresholds) || misaligned8(workspace) || misaligned8(centroid) || misaligned8(normal))
        return PD_ERR_ARG;
    for (int k = 0; k < 5; ++k)
        if (!(thresholds[k] >= 0.0) || !(thresholds[k] <= 1.0e300)) return PD_ERR_ARG;          // negative, NaN or infinite
    for (int k = 5; k < PD_PLIF_RING_THRESHOLDS; ++k)
        if (!(thresholds[k] >= -1.0) || !(thresholds[k] <= 1.0)) return PD_ERR_ARG;
    if (L > RINGS_MAX_L || A > RINGS_MAX_A || P > RINGS_MAX_P || R > A || G_l > RINGS_MAX_GL || G_r > RINGS_MAX_GR || H > RINGS_MAX_H)
        return PD_ERR_UNSUPPORTED;
    const long long need = workspace_bytes_of(P, L, N, G_r, H);
    if (need > 0x7fffffffLL) return PD_ERR_UNSUPPORTED;
    if ((long long)workspace_bytes < need) return PD_ERR_ARG;
    const RingThresholds thr = {thresholds[0], thresholds[1], thresholds[2], thresholds[3],
                                thresholds[4], thresholds[5], thresholds[6], thresholds[7]};
    double* ws_ring_min = (double*)workspace;
    unsigned char* ws_ring_bits = (unsigned char*)workspace + 8LL * P * G_r;
    unsigned char* ws_atom_bits = ws_ring_bits + (long long)P * G_r;
    unsigned char* ws_cation_bits = ws_atom_bits + (long long)P * N;
    unsigned char* ws_halogen_bits = ws_cation_bits + (long long)P * L;
    hipStream_t s = (hipStream_t)stream;
    if (G > 0)
        hipLaunchKernelGGL(plif_rings_frame_kernel, dim3(((int)G + FRAME_BLOCK - 1) / FRAME_BLOCK, P), dim3(FRAME_BLOCK), 0, s, x, ring_start,
                           ring_atom, centroid, normal, A, (int)G);
    if (G_r + N > 0)
        hipLaunchKernelGGL(plif_rings_receptor_kernel, dim3((G_r + N + RECEPTOR_BLOCK - 1) / RECEPTOR_BLOCK, P), dim3(RECEPTOR_BLOCK), 0, s, x,
                           lig_idx, type, charge, lig_active, res_atom, halogen, (const double*)centroid, (const double*)normal, thr,
                           ws_ring_bits, ws_ring_min, ws_atom_bits, A, L, N, G_l, G_r, H);
    hipLaunchKernelGGL(plif_rings_ligand_kernel, dim3(G_l + L + H, P), dim3(LIGAND_BLOCK), 0, s, x, lig_idx, type, charge, lig_active, res_atom,
                       halogen, (const double*)centroid, (const double*)normal, thr, ring_bits, ws_cation_bits, ws_halogen_bits, A, L, N, G_l,
                       G_r, H);
    hipLaunchKernelGGL(plif_rings_fold_kernel, dim3(P), dim3(FOLD_BLOCK), 0, s, lig_idx, lig_active, res_start, ring_start, ring_atom,
                       ring_residue, halogen, (const unsigned char*)ws_ring_bits, (const double*)ws_ring_min,
                       (const unsigned char*)ws_atom_bits, (const unsigned char*)ws_cation_bits, (const unsigned char*)ws_halogen_bits,
                       (const unsigned char*)ring_bits, bits, ligand_bits, min_centroid_dist, counts, L, R, N, G_l, G_r, H);
    return pd_check_launch();
}
