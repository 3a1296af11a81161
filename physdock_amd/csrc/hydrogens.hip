// Riding hydrogens of P poses of one ligand in its receptor, and the hydrogen bonds they make with the D - H ... A angle - the layer
// the heavy-atom model leaves out.  (physdock_amd/hydrogens.py builds the tables once per system; the same definition stands in its
// docstring and, as float64 numpy, in tests/hydrogens_ref.py.)
//
// Hydrogen table, H rows.  parent [H]: the pose atom the hydrogen rides on.  ref [H][3]: pose atoms n1, n2, n3, -1 where unused.
// mode [H]: PD_H_TRI 0, PD_H_BISECT 1, PD_H_NERF 2, PD_H_LINEAR 3.  length [H] (A), a [H], b [H] (radians) in fp32.  side [H]: 0
// receptor, 1 ligand.  With p the parent's position, u_i = (n_i - p) / |n_i - p| and unit(v) = v / |v|, ALL IN DOUBLE from the fp32
// coordinates and table values, the result rounded once to fp32:
//   TRI     H = p + length unit(-(u1 + u2 + u3))
//   BISECT  bis = unit(-(u1 + u2)), w = unit(u1 x u2);  H = p + length (cos a bis + sin a w)
//   NERF    bc = unit(p - n1), n = unit((n1 - n2) x bc), m = n x bc;  H = p + length (-cos a bc + sin a (cos b m + sin b n))
//           a is the angle n1 - p - H, b the dihedral n2 - n1 - p - H (0 = cis to n2)
//   LINEAR  H = p + length unit(p - n1)
// A hydrogen is NOT PLACED - x_h NaN, placed 0, part of nothing - when a vector about to be normalised is shorter than 1e-6, when a
// coordinate it reads is not finite, when a ref its mode needs is -1 (or outside 0 .. A - 1), or when its mode is none of the four.
//
// Rotor groups.  group_h [G][3]: the rows of one OH / SH (one row, then -1 -1; 12 candidates) or one NH3+ (three rows; 4
// candidates): NERF rows that share parent, n1 and n2.  Candidate k adds k * 30 degrees to every b of the group.  The group's
// acceptors are the entries A of the OTHER molecule's acceptor list with finite coordinates and |A - p| <= d_da; the score of k is
// the smallest |A - H| over the group's hydrogens and those acceptors; the smallest score wins, on a tie the smallest k, without an
// acceptor k = 0.  Only heavy atoms are looked at: no rotor sees another.  A group with a row that is not placed, or with orient ==
// 0, keeps the default angles and reports 0.
//   acc [NA_r + NA_l]: the receptor's acceptor atoms SORTED BY RESIDUE, then the ligand's (pose atoms).
//
// Hydrogen bond (the published conditions of PLIP): a placed hydrogen h whose parent D is N, O or S - the list polar [HP_l + HP_r],
// the ligand's such rows first, then the receptor's SORTED BY THE RESIDUE OF THE PARENT - and an acceptor A of the other molecule
// with |D - A| <= t[0] (4.1) and (D - H) . (A - H) <= t[1] |D - H| |A - H| (t[1] = cos 100 deg), on the fp32 x_h AS STORED, in double.
// A NaN fails every comparison.  Bit 0 hbond_donor: the ligand donates.  Bit 1 hbond_acceptor: the ligand accepts.
//   bits[p][s]         bit 0: a ligand hydrogen bonds to an acceptor of residue s (racc_start [R + 1] is the CSR of the receptor's
//                      part of acc); bit 1: a hydrogen of residue s (rh_start [R + 1], the CSR of the receptor's part of polar) bonds
//                      to a ligand acceptor
//   ligand_bits[p][i]  bit 0: a hydrogen on ligand atom i donates; bit 1: ligand atom i (lig_acc_slot [L]: its place in the ligand's
//                      part of acc, or -1) accepts
//   h_bits[p][h]       the bit of the hydrogen's side when it bonds to anything (polar_slot [H]: its place in polar, or -1)
//   counts[p][k]       the number of (hydrogen, acceptor) pairs of kind k
//
// pd_place_hydrogens, two launches.  hydrogens_place_kernel: one thread per (row, pose), PLACE_BLOCK rows per block, every row at its
// default angles.  hydrogens_rotor_kernel: one wave per (group, pose); lanes 0 .. 11 compute the 12 candidate positions into LDS, the
// lanes stride the other molecule's acceptors, each keeps its 12 minima of |A - H|^2 in registers, a min butterfly folds them, every
// lane selects the same k and lane 0 rewrites the group's rows.  pd_hydrogen_bonds, two launches.  hydrogens_hbond_kernel: one wave per
// (polar row, pose) strides the other side's acceptors, writes one workspace byte per (row, acceptor) and, after a sum butterfly, the
// row's pair count.  hydrogens_fold_kernel: one wave per pose folds the workspace by residue, ligand atom and row.  No atomics, no
// scratch memory; only OR, exact minima and integer sums are reduced, so no order matters; every value depends on its own pose alone
// and on no launch dimension: results are bit-identical from run to run, whatever P is and wherever a pose sits.  No allocation, no
// synchronisation.
#include "common.h"
#include "geom3.h"
#include "physdock_hip.h"

namespace {

constexpr int HYD_MAX_H = 65535;
constexpr int HYD_MAX_A = 1 << 22;
constexpr int HYD_MAX_P = 65535;
constexpr int HYD_MAX_L = 1024;
constexpr int PLACE_BLOCK = 128;
constexpr int ROTOR_BLOCK = 64;               // one wave: the butterflies need no LDS
constexpr int HBOND_BLOCK = 64;
constexpr int FOLD_BLOCK = 64;
constexpr int ROTOR_POSITIONS = 12;           // 12 candidates x 1 hydrogen, or 4 candidates x 3 hydrogens
constexpr double ROTOR_STEP = 0.52359877559829887;     // 30 degrees
constexpr double TINY = 1.0e-6;
static_assert(PD_HBOND_KINDS == 2 && PD_HBOND_THRESHOLDS == 2, "the counts the header documents");

// v / |v|; ok goes false when |v| is below TINY or not a number
__device__ __forceinline__ Vec3 unit(Vec3 v, bool& ok) {
    const double n = sqrt(dot(v, v));
    ok = ok && n >= TINY;
    return {v.x / n, v.y / n, v.z / n};
}
// atom i of a pose; false for an index outside 0 .. A - 1 and for a coordinate that is not finite
__device__ __forceinline__ bool load_atom(const float* xp, int A, int i, Vec3& v) {
    if (i < 0 || i >= A) return false;
    v = load3(xp + 3LL * i);
    return finite3(v);
}

// one row at the dihedral b (the table's b, or a rotor candidate's); false: not placed
__device__ __forceinline__ bool place_row(const float* xp, int A, int par, const int* r, int mode, double len, double a, double b, Vec3& h) {
    Vec3 p, n1, n2, n3, d;
    if (!load_atom(xp, A, par, p) || !load_atom(xp, A, r[0], n1)) return false;
    bool ok = true;
    if (mode == PD_H_LINEAR) {
        d = unit(sub(p, n1), ok);
    } else if (mode == PD_H_NERF) {
        if (!load_atom(xp, A, r[1], n2)) return false;
        const Vec3 bc = unit(sub(p, n1), ok);
        const Vec3 n = unit(cross(sub(n1, n2), bc), ok);
        const Vec3 m = cross(n, bc);
        const double ca = cos(a), sa = sin(a), cb = cos(b), sb = sin(b);
        d = {-ca * bc.x + sa * (cb * m.x + sb * n.x), -ca * bc.y + sa * (cb * m.y + sb * n.y), -ca * bc.z + sa * (cb * m.z + sb * n.z)};
    } else if (mode == PD_H_BISECT) {
        if (!load_atom(xp, A, r[1], n2)) return false;
        const Vec3 u1 = unit(sub(n1, p), ok), u2 = unit(sub(n2, p), ok);
        const Vec3 bis = unit(neg(add(u1, u2)), ok), w = unit(cross(u1, u2), ok);
        const double ca = cos(a), sa = sin(a);
        d = {ca * bis.x + sa * w.x, ca * bis.y + sa * w.y, ca * bis.z + sa * w.z};
    } else if (mode == PD_H_TRI) {
        if (!load_atom(xp, A, r[1], n2) || !load_atom(xp, A, r[2], n3)) return false;
        const Vec3 u1 = unit(sub(n1, p), ok), u2 = unit(sub(n2, p), ok), u3 = unit(sub(n3, p), ok);
        d = unit(neg(add(add(u1, u2), u3)), ok);
    } else {
        return false;
    }
    if (!ok) return false;
    h = {p.x + len * d.x, p.y + len * d.y, p.z + len * d.z};
    return true;
}

__global__ __launch_bounds__(PLACE_BLOCK) void hydrogens_place_kernel(const float* __restrict__ x, const int* __restrict__ parent,
                                                                      const int* __restrict__ ref, const unsigned char* __restrict__ mode,
                                                                      const float* __restrict__ length, const float* __restrict__ angle_a,
                                                                      const float* __restrict__ angle_b, float* __restrict__ x_h,
                                                                      unsigned char* __restrict__ placed, int A, int H) {
    const int h = blockIdx.x * PLACE_BLOCK + threadIdx.x, p = blockIdx.y;
    if (h >= H) return;
    const float* xp = x + (long long)p * A * 3;
    const int r[3] = {ref[3 * h], ref[3 * h + 1], ref[3 * h + 2]};
    Vec3 pos;
    const bool ok = place_row(xp, A, parent[h], r, mode[h], (double)length[h], (double)angle_a[h], (double)angle_b[h], pos);
    float* out = x_h + ((long long)p * H + h) * 3;
    const float nan = __builtin_nanf("");
    out[0] = ok ? (float)pos.x : nan;
    out[1] = ok ? (float)pos.y : nan;
    out[2] = ok ? (float)pos.z : nan;
    placed[(long long)p * H + h] = ok ? 1 : 0;
}

__global__ __launch_bounds__(ROTOR_BLOCK) void hydrogens_rotor_kernel(
    const float* __restrict__ x, const int* __restrict__ parent, const int* __restrict__ ref, const unsigned char* __restrict__ mode,
    const float* __restrict__ length, const float* __restrict__ angle_a, const float* __restrict__ angle_b,
    const unsigned char* __restrict__ side, const int* __restrict__ group_h, const int* __restrict__ acc, int NA_r, int NA_l, double d_da,
    int orient, float* __restrict__ x_h, const unsigned char* __restrict__ placed, int* __restrict__ rotor_choice, int A, int H, int G) {
    __shared__ double cand[ROTOR_POSITIONS * 3];
    const int lane = threadIdx.x, g = blockIdx.x, p = blockIdx.y;
    const float* xp = x + (long long)p * A * 3;
    const int h[3] = {group_h[3 * g], group_h[3 * g + 1], group_h[3 * g + 2]};
    const int nh = (h[1] >= 0 && h[2] >= 0) ? 3 : 1;
    bool valid = orient != 0;                                        // (every branch on `valid` is uniform over the wave)
    for (int i = 0; i < nh; ++i) valid = valid && h[i] >= 0 && h[i] < H && mode[h[i]] == PD_H_NERF && placed[(long long)p * H + h[i]] != 0;
    Vec3 pp = {0.0, 0.0, 0.0};
    valid = valid && load_atom(xp, A, parent[h[0] >= 0 && h[0] < H ? h[0] : 0], pp);
    if (!valid) {
        if (lane == 0) rotor_choice[(long long)p * G + g] = 0;
        return;
    }
    if (lane < ROTOR_POSITIONS) {                                    // position k * nh + i: candidate k, hydrogen i of the group
        const int k = lane / nh, hh = h[lane % nh];
        const int r[3] = {ref[3 * hh], ref[3 * hh + 1], ref[3 * hh + 2]};
        Vec3 c = {0.0, 0.0, 0.0};
        place_row(xp, A, parent[hh], r, PD_H_NERF, (double)length[hh], (double)angle_a[hh], (double)angle_b[hh] + (double)k * ROTOR_STEP, c);
        cand[3 * lane] = c.x;
        cand[3 * lane + 1] = c.y;
        cand[3 * lane + 2] = c.z;
    }
    __syncthreads();
    const bool lig = side[h[0]] != 0;
    const int n = lig ? NA_r : NA_l;
    const int* list = lig ? acc : acc + NA_r;
    double best[ROTOR_POSITIONS];
#pragma unroll
    for (int q = 0; q < ROTOR_POSITIONS; ++q) best[q] = INFINITY;
    for (int j = lane; j < n; j += ROTOR_BLOCK) {
        Vec3 xa;
        if (!load_atom(xp, A, list[j], xa)) continue;
        const Vec3 dp = sub(xa, pp);
        if (!(sqrt(dot(dp, dp)) <= d_da)) continue;
#pragma unroll
        for (int q = 0; q < ROTOR_POSITIONS; ++q) {
            const Vec3 e = sub(xa, Vec3{cand[3 * q], cand[3 * q + 1], cand[3 * q + 2]});
            best[q] = fmin(best[q], dot(e, e));
        }
    }
#pragma unroll
    for (int q = 0; q < ROTOR_POSITIONS; ++q) best[q] = wave_min(best[q]);
    double score[ROTOR_POSITIONS];                                   // |A - H| of candidate k; only the first 12 / nh count
    if (nh == 3) {
#pragma unroll
        for (int k = 0; k < ROTOR_POSITIONS; ++k)
            score[k] = k < 4 ? sqrt(fmin(fmin(best[3 * (k & 3)], best[3 * (k & 3) + 1]), best[3 * (k & 3) + 2])) : INFINITY;
    } else {
#pragma unroll
        for (int k = 0; k < ROTOR_POSITIONS; ++k) score[k] = sqrt(best[k]);
    }
    int kbest = 0;
    double sbest = score[0];
#pragma unroll
    for (int k = 1; k < ROTOR_POSITIONS; ++k)
        if (score[k] < sbest) {                                      // strictly: a tie keeps the smaller k
            sbest = score[k];
            kbest = k;
        }
    if (lane == 0) {
        rotor_choice[(long long)p * G + g] = kbest;
        for (int i = 0; i < nh; ++i) {
            float* out = x_h + ((long long)p * H + h[i]) * 3;
            const double* c = cand + 3 * (kbest * nh + i);
            out[0] = (float)c[0];
            out[1] = (float)c[1];
            out[2] = (float)c[2];
        }
    }
}

__global__ __launch_bounds__(HBOND_BLOCK) void hydrogens_hbond_kernel(
    const float* __restrict__ x, const float* __restrict__ x_h, const unsigned char* __restrict__ placed, const int* __restrict__ parent,
    const int* __restrict__ polar, int HP_l, const int* __restrict__ acc, int NA_r, int NA_l, double d_da, double cos_min,
    int* __restrict__ ws_count, unsigned char* __restrict__ ws_hit, int A, int H, int HP, long long W) {
    const int lane = threadIdx.x, q = blockIdx.x, p = blockIdx.y;
    const float* xp = x + (long long)p * A * 3;
    const bool lig = q < HP_l;
    const int n = lig ? NA_r : NA_l;
    const int* list = lig ? acc : acc + NA_r;
    unsigned char* row = ws_hit + (long long)p * W + (lig ? (long long)q * NA_r : (long long)HP_l * NA_r + (long long)(q - HP_l) * NA_l);
    const int h = polar[q];
    Vec3 D = {0.0, 0.0, 0.0}, Hp = {0.0, 0.0, 0.0};
    bool ok = h >= 0 && h < H && placed[(long long)p * H + h] != 0;  // (uniform over the wave)
    if (ok) {
        Hp = load3(x_h + ((long long)p * H + h) * 3);
        ok = load_atom(xp, A, parent[h], D) && finite3(Hp);
    }
    const Vec3 dh = sub(D, Hp);
    const double ndh = sqrt(dot(dh, dh));
    int cnt = 0;
    for (int j = lane; j < n; j += HBOND_BLOCK) {
        Vec3 xa;
        int hit = 0;
        if (ok && load_atom(xp, A, list[j], xa)) {
            const Vec3 da = sub(D, xa), ah = sub(xa, Hp);
            hit = (sqrt(dot(da, da)) <= d_da && dot(dh, ah) <= cos_min * ndh * sqrt(dot(ah, ah))) ? 1 : 0;
        }
        row[j] = (unsigned char)hit;
        cnt += hit;
    }
    cnt = wave_sum(cnt);
    if (lane == 0) ws_count[(long long)p * HP + q] = cnt;
}

__global__ __launch_bounds__(FOLD_BLOCK) void hydrogens_fold_kernel(
    const int* __restrict__ parent, const int* __restrict__ polar, const int* __restrict__ polar_slot, const int* __restrict__ racc_start,
    const int* __restrict__ rh_start, const int* __restrict__ lig_idx, const int* __restrict__ lig_acc_slot,
    const int* __restrict__ ws_count, const unsigned char* __restrict__ ws_hit, unsigned char* __restrict__ bits,
    unsigned char* __restrict__ ligand_bits, unsigned char* __restrict__ h_bits, int* __restrict__ counts, int H, int L, int R, int HP_l,
    int HP_r, int NA_r, int NA_l, long long W) {
    const int tid = threadIdx.x, p = blockIdx.x, HP = HP_l + HP_r;
    const int* cnt = ws_count + (long long)p * HP;
    const unsigned char* hit_l = ws_hit + (long long)p * W;            // [HP_l][NA_r]: ligand hydrogen, receptor acceptor
    const unsigned char* hit_r = hit_l + (long long)HP_l * NA_r;       // [HP_r][NA_l]: receptor hydrogen, ligand acceptor
    for (int s = tid; s < R; s += FOLD_BLOCK) {
        unsigned b = 0;
        const int a0 = max(racc_start[s], 0), a1 = min(racc_start[s + 1], NA_r);
        for (int q = 0; q < HP_l; ++q)
            for (int j = a0; j < a1; ++j) b |= hit_l[(long long)q * NA_r + j];
        const int h0 = max(rh_start[s], 0), h1 = min(rh_start[s + 1], HP_r);
        for (int q = h0; q < h1; ++q) b |= cnt[HP_l + q] > 0 ? 2u : 0u;
        bits[(long long)p * R + s] = (unsigned char)b;
    }
    for (int i = tid; i < L; i += FOLD_BLOCK) {
        unsigned b = 0;
        const int a = lig_idx[i], slot = lig_acc_slot[i];
        for (int q = 0; q < HP_l; ++q) {
            const int h = polar[q];
            if (h >= 0 && h < H && parent[h] == a && cnt[q] > 0) b |= 1u;
        }
        if (slot >= 0 && slot < NA_l)
            for (int q = 0; q < HP_r; ++q) b |= hit_r[(long long)q * NA_l + slot] ? 2u : 0u;
        ligand_bits[(long long)p * L + i] = (unsigned char)b;
    }
    for (int h = tid; h < H; h += FOLD_BLOCK) {
        const int q = polar_slot[h];
        h_bits[(long long)p * H + h] = (unsigned char)((q >= 0 && q < HP && cnt[q] > 0) ? (q < HP_l ? 1u : 2u) : 0u);
    }
    int c0 = 0, c1 = 0;
    for (int q = tid; q < HP_l; q += FOLD_BLOCK) c0 += cnt[q];
    for (int q = tid; q < HP_r; q += FOLD_BLOCK) c1 += cnt[HP_l + q];
    c0 = wave_sum(c0);
    c1 = wave_sum(c1);
    if (tid == 0) counts[2 * p] = c0;
    if (tid == 1) counts[2 * p + 1] = c1;
}

inline bool misaligned4(const void* a) { return ((uintptr_t)a & 3) != 0; }
inline bool misaligned8(const void* a) { return ((uintptr_t)a & 7) != 0; }

// the workspace: ws_count int [P][HP_l + HP_r], then the bytes ws_hit [P][HP_l * NA_r + HP_r * NA_l]; rounded up to a multiple of 8
inline long long hit_row_bytes(long long HP_l, long long HP_r, long long NA_r, long long NA_l) { return HP_l * NA_r + HP_r * NA_l; }
inline long long workspace_bytes_of(long long P, long long HP_l, long long HP_r, long long NA_r, long long NA_l) {
    return (P * (4 * (HP_l + HP_r) + hit_row_bytes(HP_l, HP_r, NA_r, NA_l)) + 7) / 8 * 8;
}
inline bool sizes_bad(int HP_l, int HP_r, int NA_r, int NA_l) { return HP_l < 0 || HP_r < 0 || NA_r < 0 || NA_l < 0; }
inline bool sizes_large(int HP_l, int HP_r, int NA_r, int NA_l) {
    return (long long)HP_l + HP_r > HYD_MAX_H || NA_r > HYD_MAX_A || NA_l > HYD_MAX_L;
}

}  // namespace

PD_EXPORT int pd_place_hydrogens(const float* x, const int* parent, const int* ref, const unsigned char* mode, const float* length,
                                 const float* angle_a, const float* angle_b, const unsigned char* side, const int* group_h, int G,
                                 const int* acc, int NA_r, int NA_l, double d_da, int orient, float* x_h, unsigned char* placed,
                                 int* rotor_choice, int P, int A, int H, void* stream) {
    if (!x || !parent || !ref || !mode || !length || !angle_a || !angle_b || !side || !x_h || !placed) return PD_ERR_ARG;
    if (P <= 0 || A <= 0 || H <= 0 || G < 0 || NA_r < 0 || NA_l < 0 || (long long)NA_r + NA_l > A) return PD_ERR_ARG;
    if (G > 0 && (!group_h || !rotor_choice)) return PD_ERR_ARG;
    if (NA_r + NA_l > 0 && !acc) return PD_ERR_ARG;
    if (misaligned4(x) || misaligned4(parent) || misaligned4(ref) || misaligned4(length) || misaligned4(angle_a) || misaligned4(angle_b) ||
        misaligned4(group_h) || misaligned4(acc) || misaligned4(x_h) || misaligned4(rotor_choice))
        return PD_ERR_ARG;
    if (!(d_da >= 0.0) || !(d_da <= 1.0e300)) return PD_ERR_ARG;    // negative, NaN or infinite
    if (H > HYD_MAX_H || A > HYD_MAX_A || P > HYD_MAX_P) return PD_ERR_UNSUPPORTED;
    if (G > H) return PD_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(hydrogens_place_kernel, dim3((H + PLACE_BLOCK - 1) / PLACE_BLOCK, P), dim3(PLACE_BLOCK), 0, s, x, parent, ref, mode,
                       length, angle_a, angle_b, x_h, placed, A, H);
    if (G > 0)
        hipLaunchKernelGGL(hydrogens_rotor_kernel, dim3(G, P), dim3(ROTOR_BLOCK), 0, s, x, parent, ref, mode, length, angle_a, angle_b, side,
                           group_h, acc, NA_r, NA_l, d_da, orient, x_h, (const unsigned char*)placed, rotor_choice, A, H, G);
    return pd_check_launch();
}

PD_EXPORT int pd_hydrogen_bonds_workspace(int P, int HP_l, int HP_r, int NA_r, int NA_l) {
    if (P <= 0 || sizes_bad(HP_l, HP_r, NA_r, NA_l)) return PD_ERR_ARG;
    const long long bytes = workspace_bytes_of(P, HP_l, HP_r, NA_r, NA_l);
    return bytes > 0x7fffffffLL ? PD_ERR_UNSUPPORTED : (int)(bytes > 8 ? bytes : 8);
}

PD_EXPORT int pd_hydrogen_bonds(const float* x, const float* x_h, const unsigned char* placed, const int* parent, const int* polar,
                                int HP_l, int HP_r, const int* polar_slot, const int* acc, int NA_r, int NA_l, const int* racc_start,
                                const int* rh_start, const int* lig_idx, const int* lig_acc_slot, const double* thresholds,
                                void* workspace, size_t workspace_bytes, unsigned char* bits, unsigned char* ligand_bits,
                                unsigned char* h_bits, int* counts, int P, int A, int H, int L, int R, void* stream) {
    if (!x || !x_h || !placed || !parent || !polar_slot || !racc_start || !rh_start || !lig_idx || !lig_acc_slot || !thresholds ||
        !workspace || !bits || !ligand_bits || !h_bits || !counts)
        return PD_ERR_ARG;
    if (P <= 0 || A <= 0 || H <= 0 || L <= 0 || R <= 0 || sizes_bad(HP_l, HP_r, NA_r, NA_l) || (long long)NA_r + NA_l > A) return PD_ERR_ARG;
    if (HP_l + HP_r > 0 && !polar) return PD_ERR_ARG;
    if (NA_r + NA_l > 0 && !acc) return PD_ERR_ARG;
    if (misaligned4(x) || misaligned4(x_h) || misaligned4(parent) || misaligned4(polar) || misaligned4(polar_slot) || misaligned4(acc) ||
        misaligned4(racc_start) || misaligned4(rh_start) || misaligned4(lig_idx) || misaligned4(lig_acc_slot) || misaligned4(counts) ||
        misaligned8(thresholds) || misaligned8(workspace))
        return PD_ERR_ARG;
    if (!(thresholds[0] >= 0.0) || !(thresholds[0] <= 1.0e300) || !(thresholds[1] >= -1.0) || !(thresholds[1] <= 1.0)) return PD_ERR_ARG;
    if (H > HYD_MAX_H || (long long)HP_l + HP_r > H || L > HYD_MAX_L || A > HYD_MAX_A || P > HYD_MAX_P || R > A ||
        sizes_large(HP_l, HP_r, NA_r, NA_l))
        return PD_ERR_UNSUPPORTED;
    const long long need = workspace_bytes_of(P, HP_l, HP_r, NA_r, NA_l);
    if (need > 0x7fffffffLL) return PD_ERR_UNSUPPORTED;
    if ((long long)workspace_bytes < need) return PD_ERR_ARG;
    const int HP = HP_l + HP_r;
    const long long W = hit_row_bytes(HP_l, HP_r, NA_r, NA_l);
    int* ws_count = (int*)workspace;
    unsigned char* ws_hit = (unsigned char*)workspace + 4LL * P * HP;
    hipStream_t s = (hipStream_t)stream;
    if (HP > 0)
        hipLaunchKernelGGL(hydrogens_hbond_kernel, dim3(HP, P), dim3(HBOND_BLOCK), 0, s, x, x_h, placed, parent, polar, HP_l, acc, NA_r, NA_l,
                           thresholds[0], thresholds[1], ws_count, ws_hit, A, H, HP, W);
    hipLaunchKernelGGL(hydrogens_fold_kernel, dim3(P), dim3(FOLD_BLOCK), 0, s, parent, polar, polar_slot, racc_start, rh_start, lig_idx,
                       lig_acc_slot, (const int*)ws_count, (const unsigned char*)ws_hit, bits, ligand_bits, h_bits, counts, H, L, R, HP_l, HP_r,
                       NA_r, NA_l, W);
    return pd_check_launch();
}
