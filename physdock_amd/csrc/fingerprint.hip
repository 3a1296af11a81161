// Circular (Morgan / ECFP-like) fingerprints of ligand graphs and what a screening run asks of them: Tanimoto similarity of two sets
// of fingerprints, the k nearest rows, and a MaxMin diverse subset.  The reference keys its ligands by the MD5 of their SMILES string
// (screening.py:100-103) and compares nothing; this is the package's own definition after Rogers & Hahn 2010, written down in
// tests/fingerprint_ref.py and physdock_amd/fingerprints.py - not RDKit's bytes.  Integers from end to end; the one float operation is
// the IEEE fp32 quotient of two exact integers when a similarity is written.
//
// morgan_kernel, one block of 256 threads per ligand, L <= 128 atoms, at most 512 bonds, the tables of pd_ligand_features.  In LDS: the
// bond list, the adjacency as one 128-bit mask per atom (for the bridge test) and as a CSR list of (neighbour, bond), the identifiers
// of every radius, the bond sets of radius 1 .. R as 16 words per atom (32 KB at R = 4) and the ligand's bit row.  No atomics except
// the LDS atomicOr into the bit row, which commutes.  A ligand reads its own rows only: the same bits alone or anywhere in a library.
//   phase 0  all threads copy the bond list; a bond that leaves its ligand is marked and skipped from then on
//   phase 1  thread a owns atom a: adjacency mask and degree from the bond list
//   phase 2  thread 0: prefix sums of the degrees; all threads: the bridge test per bond (strided), a breadth-first search from one
//            end that may not use the bond itself, as bond_in_ring of pd_ligand_features
//   phase 3  thread a: its CSR segment, in-ring = a bond that is no bridge, id_0 (or the given invariant)
//   phase 4  for r = 1 .. R: thread a hashes r, id_{r-1}(a) and its neighbours' (o2, id_{r-1}) in ascending order - the next pair is
//            found by a scan of the segment for the smallest (o2, id, position) above the last one, so no degree bounds a register
//            array; all threads: word w of env_r(a) = env_{r-1}(a) | union over neighbours (env_{r-1}(b) | bond a-b), one item per
//            (atom, word)
//   phase 5  thread f owns feature (a, r), r >= 1 (strided): a digest of its bond set; then kept = no feature (a', r') with the same
//            set and a smaller (r', id, a') - a closed predicate, no serial walk.  Kept features OR their bit into the row
//   phase 6  ids, kept, the bit row and the two counts are written
// A ligand whose rows leave the arrays is not written (the host layer refuses it before any launch).
//
// tanimoto_kernel: tiles of 16 rows x 16 columns, both staged whole in LDS with a row stride of W + 1 words (the sixteen rows a wave
// reads lie in sixteen banks), one thread per (row, column).  nearest_kernel: one block per row of a; thread t scans the columns t,
// t + 256, .. and keeps its own k best in LDS (slot-major, so the 256 lists lie in 256 consecutive words), ordered by the EXACT
// fraction (c1 u2 against c2 u1, both below 2^25) and then the smaller column; k rounds of a block-wide best-of-heads give the answer.
// maxmin: per pick, one launch raises every row's largest similarity to the picked rows against the newest pick (read from device
// memory) and leaves each block's best candidate, one launch of a single block selects among them.  Nothing is read back.
#include "common.h"
#include "hash32.h"
#include "mask128.h"
#include "physdock_hip.h"

namespace {

constexpr int FP_MAX_L = PD_LIGAND_FEATURES_MAX_ATOMS;
constexpr int FP_MAX_B = PD_LIGAND_FEATURES_MAX_BONDS;
constexpr int FP_MAX_G = 65535;
constexpr int FP_MAX_R = PD_FINGERPRINT_MAX_RADIUS;
constexpr int FP_ENV_WORDS = FP_MAX_B / 32;
constexpr int FP_MAX_W = PD_FINGERPRINT_MAX_WORDS;
constexpr int FP_MAX_K = PD_FINGERPRINT_MAX_K;
constexpr int FP_TILE = 16;
constexpr int FP_MAX_ROWS = 65535 * FP_TILE;           // the tile grid's second dimension
constexpr unsigned char FP_SKIP = 0xFF;

__global__ __launch_bounds__(256) void morgan_kernel(const int* __restrict__ atom_start, const int* __restrict__ bond_start,
                                                    const int* __restrict__ atoms, const int* __restrict__ bonds,
                                                    const unsigned* __restrict__ invariants, unsigned* __restrict__ bits_out,
                                                    unsigned* __restrict__ ids_out, unsigned char* __restrict__ kept_out,
                                                    int* __restrict__ n_features, int* __restrict__ popcount, int n_atoms, int n_bonds,
                                                    int R, int W) {
    __shared__ unsigned env[FP_MAX_R][FP_MAX_L][FP_ENV_WORDS];
    __shared__ unsigned ident[FP_MAX_R + 1][FP_MAX_L], digest[FP_MAX_R][FP_MAX_L];
    __shared__ unsigned char keptf[FP_MAX_R + 1][FP_MAX_L];
    __shared__ Mask adj[FP_MAX_L];
    __shared__ int bo[FP_MAX_B];
    __shared__ unsigned char bi[FP_MAX_B], bj[FP_MAX_B], bridge[FP_MAX_B];
    __shared__ unsigned short csr[2 * FP_MAX_B][2];                  // (neighbour, bond)
    __shared__ unsigned short cstart[FP_MAX_L + 1], deg[FP_MAX_L];
    __shared__ unsigned row[FP_MAX_W];
    __shared__ int red[4][2];

    const int g = blockIdx.x, tid = threadIdx.x;
    const int a0 = atom_start[g], a1 = atom_start[g + 1], b0 = bond_start[g], b1 = bond_start[g + 1];
    const int L = a1 - a0, nb = b1 - b0;
    if (a0 < 0 || L < 1 || L > FP_MAX_L || a1 > n_atoms || b0 < 0 || nb < 0 || nb > FP_MAX_B || b1 > n_bonds)
        return;                                              // (uniform over the block)
    const int* my_atoms = atoms + 4 * (long long)a0;
    const int* my_bonds = bonds + 4 * (long long)b0;

    // ---- phase 0: the bond list
    for (int b = tid; b < nb; b += 256) {
        const int i = my_bonds[4 * b], j = my_bonds[4 * b + 1];
        const bool ok = (unsigned)i < (unsigned)L && (unsigned)j < (unsigned)L && i != j;
        bi[b] = ok ? (unsigned char)i : FP_SKIP;
        bj[b] = ok ? (unsigned char)j : FP_SKIP;
        bo[b] = my_bonds[4 * b + 2];
        bridge[b] = 1;
    }
    for (int w = tid; w < W; w += 256) row[w] = 0;
    __syncthreads();
    // ---- phase 1: per atom, from the bond list
    if (tid < L) {
        Mask m = {0ull, 0ull};
        int d = 0;
        for (int b = 0; b < nb; ++b) {
            const int i = bi[b], j = bj[b];
            if (i == FP_SKIP || (i != tid && j != tid)) continue;
            m = mk_or(m, mk_bit(i == tid ? j : i));
            ++d;
        }
        adj[tid] = m;
        deg[tid] = (unsigned short)d;
    }
    __syncthreads();
    // ---- phase 2: the segment starts; the bridge test per bond
    if (tid == 0) {
        int s = 0;
        for (int a = 0; a < L; ++a) { cstart[a] = (unsigned short)s; s += deg[a]; }
        cstart[L] = (unsigned short)s;
    }
    for (int b = tid; b < nb; b += 256) {
        const int i = bi[b], j = bj[b];
        if (i == FP_SKIP) continue;
        Mask seen = mk_bit(i), front = mk_andn(mk_andn(adj[i], mk_bit(j)), seen);       // j from i without the bond (i, j)
        bool ring = false;
        while (mk_any(front)) {
            if (mk_has(front, j)) { ring = true; break; }
            seen = mk_or(seen, front);
            Mask next = {0ull, 0ull}, walk = front;
            while (mk_any(walk)) {
                const int k = mk_first(walk);
                walk = mk_andn(walk, mk_bit(k));
                next = mk_or(next, adj[k]);
            }
            front = mk_andn(next, seen);
        }
        bridge[b] = ring ? 0 : 1;
    }
    __syncthreads();
    // ---- phase 3: the neighbour lists, id_0
    if (tid < L) {
        int at = cstart[tid];
        bool in_ring = false;
        for (int b = 0; b < nb; ++b) {
            const int i = bi[b], j = bj[b];
            if (i == FP_SKIP || (i != tid && j != tid)) continue;
            csr[at][0] = (unsigned short)(i == tid ? j : i);
            csr[at][1] = (unsigned short)b;
            ++at;
            in_ring = in_ring || !bridge[b];
        }
        unsigned h;
        if (invariants) {
            h = invariants[a0 + tid];
        } else {
            h = fp_push(0u, (unsigned)my_atoms[4 * tid]);
            h = fp_push(h, (unsigned)deg[tid]);
            h = fp_push(h, (unsigned)my_atoms[4 * tid + 2]);
            h = fp_push(h, (unsigned)my_atoms[4 * tid + 1]);
            h = fp_push(h, in_ring ? 1u : 0u);
            h = fp_push(h, (unsigned)(my_atoms[4 * tid + 3] & 1));
        }
        ident[0][tid] = h;
        keptf[0][tid] = 1;
    }
    __syncthreads();
    // ---- phase 4: the identifiers and the bond sets, radius by radius
    for (int r = 1; r <= R; ++r) {
        if (tid < L) {
            const unsigned* prev = ident[r - 1];
            const int s0 = cstart[tid], s1 = cstart[tid + 1];
            unsigned h = fp_push(fp_push(0u, (unsigned)r), prev[tid]);
            unsigned lo = 0, li = 0;
            int lp = -1;                                     // the last pair taken: (o2, id, position); none yet
            for (int n = s0; n < s1; ++n) {
                unsigned bo2 = 0, bid = 0;
                int bp = -1;
                for (int p = s0; p < s1; ++p) {
                    const unsigned o2 = (unsigned)bo[csr[p][1]], id = prev[csr[p][0]];
                    const bool above = lp < 0 || o2 > lo || (o2 == lo && (id > li || (id == li && p > lp)));
                    const bool below = bp < 0 || o2 < bo2 || (o2 == bo2 && (id < bid || (id == bid && p < bp)));
                    if (above && below) { bo2 = o2; bid = id; bp = p; }
                }
                h = fp_push(fp_push(h, bo2), bid);
                lo = bo2; li = bid; lp = bp;
            }
            ident[r][tid] = h;
        }
        for (int e = tid; e < L * FP_ENV_WORDS; e += 256) {
            const int a = e / FP_ENV_WORDS, w = e % FP_ENV_WORDS;
            unsigned v = r >= 2 ? env[r - 2][a][w] : 0u;
            for (int p = cstart[a], p1 = cstart[a + 1]; p < p1; ++p) {
                const int nbr = csr[p][0], b = csr[p][1];
                if (r >= 2) v |= env[r - 2][nbr][w];
                if ((b >> 5) == w) v |= 1u << (b & 31);
            }
            env[r - 1][a][w] = v;
        }
        __syncthreads();
    }
    // ---- phase 5: which features are kept
    const int nf = L * R;
    for (int f = tid; f < nf; f += 256) {
        const int r = f / L, a = f - r * L;                  // (radius r + 1)
        unsigned h = 0;
        for (int w = 0; w < FP_ENV_WORDS; ++w) h = fp_push(h, env[r][a][w]);
        digest[r][a] = h;
    }
    __syncthreads();
    int n_kept = 0;
    if (tid < L) {
        n_kept = 1;
        const unsigned k = ident[0][tid] & (unsigned)(32 * W - 1);
        atomicOr(&row[k >> 5], 1u << (k & 31));
    }
    for (int f = tid; f < nf; f += 256) {
        const int r = f / L, a = f - r * L;
        const unsigned id = ident[r + 1][a], dg = digest[r][a];
        bool keep = true;
        for (int r2 = 0; r2 <= r && keep; ++r2)
            for (int a2 = 0; a2 < L; ++a2) {
                if (digest[r2][a2] != dg) continue;
                const unsigned id2 = ident[r2 + 1][a2];
                if (!(r2 < r || id2 < id || (id2 == id && a2 < a))) continue;          // (a2, r2) does not come before (a, r)
                bool same = true;
                for (int w = 0; w < FP_ENV_WORDS; ++w) same = same && env[r2][a2][w] == env[r][a][w];
                if (same) { keep = false; break; }
            }
        keptf[r + 1][a] = keep ? 1 : 0;
        if (keep) {
            ++n_kept;
            const unsigned k = id & (unsigned)(32 * W - 1);
            atomicOr(&row[k >> 5], 1u << (k & 31));
        }
    }
    __syncthreads();
    // ---- phase 6: the outputs
    const int R1 = R + 1;
    for (int e = tid; e < L * R1; e += 256) {
        const int a = e / R1, r = e - a * R1;
        ids_out[(long long)a0 * R1 + e] = ident[r][a];
        kept_out[(long long)a0 * R1 + e] = keptf[r][a];
    }
    int pop = 0;
    for (int w = tid; w < W; w += 256) {
        bits_out[(long long)g * W + w] = row[w];
        pop += __popc(row[w]);
    }
    const int s_kept = wave_sum(n_kept), s_pop = wave_sum(pop);
    if ((tid & 63) == 0) { red[tid >> 6][0] = s_kept; red[tid >> 6][1] = s_pop; }
    __syncthreads();
    if (tid == 0) {
        n_features[g] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
        popcount[g] = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
    }
}

// the similarity of c common bits in a union of u: an empty union gives 1, as plif_ratio of plif.hip
__device__ __forceinline__ float fp_ratio(int c, int u) { return u == 0 ? 1.f : (float)c / (float)u; }

// one candidate of an ordering by similarity: c common bits, a union of u, column j.  u < 0: no candidate (it comes last)
struct Cand {
    int c, u, j;
};
// x comes before y: the larger exact fraction (an empty union counts as 1 / 1), then the smaller column
__device__ __forceinline__ bool fp_before(Cand x, Cand y) {
    if (x.u < 0 || y.u < 0) return y.u < 0 && x.u >= 0;
    const int c1 = x.u == 0 ? 1 : x.c, u1 = x.u == 0 ? 1 : x.u, c2 = y.u == 0 ? 1 : y.c, u2 = y.u == 0 ? 1 : y.u;
    const int l = c1 * u2, r = c2 * u1;                      // c, u <= 4096 words of bits: below 2^25
    return l > r || (l == r && x.j < y.j);
}
// the reverse order for MaxMin: the smaller fraction first, then the smaller index
__device__ __forceinline__ bool fp_before_min(Cand x, Cand y) {
    if (x.u < 0 || y.u < 0) return y.u < 0 && x.u >= 0;
    const int c1 = x.u == 0 ? 1 : x.c, u1 = x.u == 0 ? 1 : x.u, c2 = y.u == 0 ? 1 : y.c, u2 = y.u == 0 ? 1 : y.u;
    const int l = c1 * u2, r = c2 * u1;
    return l < r || (l == r && x.j < y.j);
}

// the first of the block's 256 candidates in the order `before` (a strict total order on distinct columns), returned to every thread
template <bool MIN>
__device__ __forceinline__ Cand fp_block_first(Cand v, Cand* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Cand w = {__shfl_xor(v.c, o), __shfl_xor(v.u, o), __shfl_xor(v.j, o)};
        if (MIN ? fp_before_min(w, v) : fp_before(w, v)) v = w;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    Cand best = red[0];
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (MIN ? fp_before_min(red[k], best) : fp_before(red[k], best)) best = red[k];
    return best;
}

__global__ __launch_bounds__(256) void tanimoto_kernel(const unsigned* __restrict__ a, const unsigned* __restrict__ b,
                                                      float* __restrict__ sim, int* __restrict__ common, int n, int m, int W) {
    __shared__ unsigned rows[2][FP_TILE][FP_MAX_W + 1];
    const int tid = threadIdx.x, tp = tid >> 4, tq = tid & 15;
    const int p0 = blockIdx.y * FP_TILE, q0 = blockIdx.x * FP_TILE;
    for (int e = tid; e < 2 * FP_TILE * W; e += 256) {
        const int side = e / (FP_TILE * W), r = (e / W) % FP_TILE, w = e % W;
        const int src = (side ? q0 : p0) + r;
        unsigned v = 0;
        if (src < (side ? m : n)) v = (side ? b : a)[(long long)src * W + w];
        rows[side][r][w] = v;
    }
    __syncthreads();
    int c = 0, pa = 0, pb = 0;
    for (int w = 0; w < W; ++w) {
        const unsigned x = rows[0][tp][w], y = rows[1][tq][w];
        c += __popc(x & y);
        pa += __popc(x);
        pb += __popc(y);
    }
    const int p = p0 + tp, q = q0 + tq;
    if (p < n && q < m) {
        sim[(long long)p * m + q] = fp_ratio(c, pa + pb - c);
        if (common) common[(long long)p * m + q] = c;
    }
}

__global__ __launch_bounds__(256) void nearest_kernel(const unsigned* __restrict__ a, const unsigned* __restrict__ b,
                                                     int* __restrict__ index, float* __restrict__ similarity,
                                                     int* __restrict__ common, int m, int W, int k, int exclude_self) {
    __shared__ unsigned mine[FP_MAX_W];
    __shared__ int lc[FP_MAX_K][256], lu[FP_MAX_K][256], lj[FP_MAX_K][256];
    __shared__ Cand red[4];
    const int tid = threadIdx.x, i = blockIdx.x;
    int pa = 0;
    for (int w = tid; w < W; w += 256) mine[w] = a[(long long)i * W + w];
    for (int s = 0; s < k; ++s) { lc[s][tid] = 0; lu[s][tid] = -1; lj[s][tid] = 0; }
    __syncthreads();
    for (int w = 0; w < W; ++w) pa += __popc(mine[w]);
    for (int j = tid; j < m; j += 256) {
        if (exclude_self && j == i) continue;
        const unsigned* src = b + (long long)j * W;
        int c = 0, pb = 0;
        for (int w = 0; w < W; ++w) {
            const unsigned y = src[w];
            c += __popc(mine[w] & y);
            pb += __popc(y);
        }
        const Cand v = {c, pa + pb - c, j};
        if (!fp_before(v, Cand{lc[k - 1][tid], lu[k - 1][tid], lj[k - 1][tid]})) continue;
        int s = k - 1;                                       // insertion into the thread's own list, best first
        while (s > 0 && fp_before(v, Cand{lc[s - 1][tid], lu[s - 1][tid], lj[s - 1][tid]})) {
            lc[s][tid] = lc[s - 1][tid]; lu[s][tid] = lu[s - 1][tid]; lj[s][tid] = lj[s - 1][tid];
            --s;
        }
        lc[s][tid] = v.c; lu[s][tid] = v.u; lj[s][tid] = v.j;
    }
    int head = 0;
    for (int s = 0; s < k; ++s) {
        Cand v = {0, -1, 0};
        if (head < k) v = Cand{lc[head][tid], lu[head][tid], lj[head][tid]};
        const Cand best = fp_block_first<false>(v, red);
        if (head < k && v.u >= 0 && v.j == best.j && best.u >= 0) ++head;
        if (tid == 0) {
            const long long o = (long long)i * k + s;
            index[o] = best.u >= 0 ? best.j : -1;
            similarity[o] = best.u >= 0 ? fp_ratio(best.c, best.u) : __int_as_float(0x7FC00000);
            common[o] = best.u >= 0 ? best.c : 0;
        }
    }
}

// MaxMin state in the workspace: run_c, run_u int32 [n] (each row's largest similarity to the picked rows; u < 0: none yet),
// picked int32 [n], then one Cand per block of the update launch
__global__ __launch_bounds__(256) void maxmin_init_kernel(int* __restrict__ run_c, int* __restrict__ run_u, int* __restrict__ picked,
                                                         int* __restrict__ picks, float* __restrict__ max_similarity, int n, int first) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) { run_c[i] = 0; run_u[i] = -1; picked[i] = i == first ? 1 : 0; }
    if (i == 0) { picks[0] = first; max_similarity[0] = __int_as_float(0x7FC00000); }
}

__global__ __launch_bounds__(256) void maxmin_update_kernel(const unsigned* __restrict__ bits, int* __restrict__ run_c,
                                                           int* __restrict__ run_u, const int* __restrict__ picked,
                                                           const int* __restrict__ picks, Cand* __restrict__ block_best, int n, int W,
                                                           int t) {
    __shared__ unsigned pick_row[FP_MAX_W];
    __shared__ Cand red[4];
    const int tid = threadIdx.x, i = blockIdx.x * 256 + tid;
    const int p = picks[t - 1];                              // the newest pick, on the device
    const bool ok = (unsigned)p < (unsigned)n;
    for (int w = tid; w < W; w += 256) pick_row[w] = ok ? bits[(long long)p * W + w] : 0u;
    __syncthreads();
    Cand v = {0, -1, 0};
    if (i < n) {
        int pp = 0, c = 0, pi = 0;
        const unsigned* src = bits + (long long)i * W;
        for (int w = 0; w < W; ++w) {
            const unsigned y = src[w];
            c += __popc(pick_row[w] & y);
            pi += __popc(y);
            pp += __popc(pick_row[w]);
        }
        Cand now = {c, pp + pi - c, 0}, run = {run_c[i], run_u[i], 0};
        if (run.u < 0 || fp_before_min(run, now)) {          // the new similarity is larger (on a tie the values are equal)
            run = now;
            run_c[i] = now.c; run_u[i] = now.u;
        }
        if (!picked[i]) v = Cand{run.c, run.u, i};
    }
    const Cand best = fp_block_first<true>(v, red);
    if (tid == 0) block_best[blockIdx.x] = best;
}

__global__ __launch_bounds__(256) void maxmin_select_kernel(const Cand* __restrict__ block_best, int* __restrict__ picked,
                                                           int* __restrict__ picks, float* __restrict__ max_similarity, int n_blocks,
                                                           int t) {
    __shared__ Cand red[4];
    Cand v = {0, -1, 0};
    for (int k = threadIdx.x; k < n_blocks; k += 256) {
        const Cand w = block_best[k];
        if (fp_before_min(w, v)) v = w;
    }
    const Cand best = fp_block_first<true>(v, red);
    if (threadIdx.x == 0) {
        picks[t] = best.u >= 0 ? best.j : -1;
        max_similarity[t] = best.u >= 0 ? fp_ratio(best.c, best.u) : __int_as_float(0x7FC00000);
        if (best.u >= 0) picked[best.j] = 1;
    }
}

inline bool fp_bad_words(int W) { return W < 1 || W > FP_MAX_W; }

}  // namespace

PD_EXPORT int pd_morgan_fingerprint(const int* atom_start, const int* bond_start, const int* atoms, const int* bonds,
                                    const unsigned* atom_invariants, unsigned* bits, unsigned* ids, unsigned char* kept, int* n_features,
                                    int* popcount, int n_ligands, int n_atoms, int n_bonds, int radius, int n_bits, void* stream) {
    if (!atom_start || !bond_start || !atoms || !bits || !ids || !kept || !n_features || !popcount) return PD_ERR_ARG;
    if (n_ligands < 1 || n_atoms < n_ligands || n_bonds < 0 || (n_bonds > 0 && !bonds)) return PD_ERR_ARG;
    if (radius < 0 || radius > FP_MAX_R || (n_bits != 512 && n_bits != 1024 && n_bits != 2048 && n_bits != 4096)) return PD_ERR_ARG;
    if (pd_misaligned(atom_start, 4) || pd_misaligned(bond_start, 4) || pd_misaligned(atoms, 4) || pd_misaligned(bonds, 4) ||
        pd_misaligned(atom_invariants, 4) || pd_misaligned(bits, 4) || pd_misaligned(ids, 4) || pd_misaligned(n_features, 4) ||
        pd_misaligned(popcount, 4))
        return PD_ERR_ARG;
    if (n_ligands > FP_MAX_G || n_atoms > (long long)n_ligands * FP_MAX_L) return PD_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(morgan_kernel, dim3(n_ligands), dim3(256), 0, (hipStream_t)stream, atom_start, bond_start, atoms, bonds,
                       atom_invariants, bits, ids, kept, n_features, popcount, n_atoms, n_bonds, radius, n_bits / 32);
    return pd_check_launch();
}

PD_EXPORT int pd_fingerprint_tanimoto(const unsigned* a, const unsigned* b, float* sim, int* common, int n, int m, int n_words,
                                      void* stream) {
    if (!a || !b || !sim || n < 1 || m < 1 || fp_bad_words(n_words)) return PD_ERR_ARG;
    if (pd_misaligned(a, 4) || pd_misaligned(b, 4) || pd_misaligned(sim, 4) || pd_misaligned(common, 4)) return PD_ERR_ARG;
    if (n > FP_MAX_ROWS || m > FP_MAX_ROWS) return PD_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(tanimoto_kernel, dim3((m + FP_TILE - 1) / FP_TILE, (n + FP_TILE - 1) / FP_TILE), dim3(256), 0, (hipStream_t)stream,
                       a, b, sim, common, n, m, n_words);
    return pd_check_launch();
}

PD_EXPORT int pd_fingerprint_nearest(const unsigned* a, const unsigned* b, int* index, float* similarity, int* common, int n, int m,
                                     int n_words, int k, int exclude_self, void* stream) {
    if (!a || !b || !index || !similarity || !common || n < 1 || m < 1 || fp_bad_words(n_words)) return PD_ERR_ARG;
    if (exclude_self != 0 && exclude_self != 1) return PD_ERR_ARG;
    if (k < 1 || k > FP_MAX_K || k > m - exclude_self) return PD_ERR_ARG;
    if (pd_misaligned(a, 4) || pd_misaligned(b, 4) || pd_misaligned(index, 4) || pd_misaligned(similarity, 4) || pd_misaligned(common, 4))
        return PD_ERR_ARG;
    if (n > FP_MAX_ROWS || m > FP_MAX_ROWS) return PD_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(nearest_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, a, b, index, similarity, common, m, n_words, k,
                       exclude_self);
    return pd_check_launch();
}

PD_EXPORT int pd_fingerprint_maxmin_workspace_numel(int n) {
    if (n < 1) return PD_ERR_ARG;
    if (n > FP_MAX_ROWS) return PD_ERR_UNSUPPORTED;
    return 3 * n + 3 * ((n + 255) / 256);
}

PD_EXPORT int pd_fingerprint_maxmin(const unsigned* bits, int* ws, int ws_numel, int* picks, float* max_similarity, int n, int n_words,
                                    int n_pick, int first, void* stream) {
    if (!bits || !ws || !picks || !max_similarity || n < 1 || fp_bad_words(n_words)) return PD_ERR_ARG;
    if (n_pick < 1 || n_pick > n || first < 0 || first >= n) return PD_ERR_ARG;
    if (pd_misaligned(bits, 4) || pd_misaligned(ws, 4) || pd_misaligned(picks, 4) || pd_misaligned(max_similarity, 4)) return PD_ERR_ARG;
    if (n > FP_MAX_ROWS) return PD_ERR_UNSUPPORTED;
    if (ws_numel < pd_fingerprint_maxmin_workspace_numel(n)) return PD_ERR_ARG;
    const int n_blocks = (n + 255) / 256;
    int *run_c = ws, *run_u = ws + n, *picked = ws + 2 * n;
    Cand* block_best = (Cand*)(ws + 3 * n);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(maxmin_init_kernel, dim3(n_blocks), dim3(256), 0, s, run_c, run_u, picked, picks, max_similarity, n, first);
    for (int t = 1; t < n_pick; ++t) {
        hipLaunchKernelGGL(maxmin_update_kernel, dim3(n_blocks), dim3(256), 0, s, bits, run_c, run_u, (const int*)picked,
                           (const int*)picks, block_best, n, n_words, t);
        hipLaunchKernelGGL(maxmin_select_kernel, dim3(1), dim3(256), 0, s, (const Cand*)block_best, picked, picks, max_similarity,
                           n_blocks, t);
    }
    return pd_check_launch();
}
