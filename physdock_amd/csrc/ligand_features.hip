// Ligand features from the molecular graph: the int8 tables of the reference's get_features_from_ref_mol (PhysDock/data/tools/rdkit.py)
// and the packed blocks ref_feat [L][167] and rel_tok_feat [L][L][42] of FeatureLoader._update_smi (feature_loader.py:327-352), for a
// whole library of ligands in one launch.  The reference computes them with RDKit on the host; this is the package's own definition,
// written down in tests/ligand_features_ref.py and physdock_amd/ligand.py - not RDKit's bytes.
//
// ligand_features_kernel, one block of 256 threads per ligand, L <= 128 atoms.  In LDS: the adjacency as one 128-bit mask per atom, the
// graph distances [L][L] as bytes and one 16-bit word per atom pair for what its bond says.  Integers only; the one float operation
// is the conversion of a small integer (0, 1, the truncated order, the charge) when a block is written.  No atomics: every LDS and
// global location has one writer.  A ligand reads its own rows of the tables only, so its results are the same bits alone or anywhere
// in a library.
//   phase 1  thread a owns atom a: it walks the ligand's bonds and builds its own adjacency mask, its degree, the number of its
//            aromatic bonds, twice the sum of its other orders, and whether it is a pi atom (a bond of order >= 1.5)
//   phase 2  thread a: donor (N, O, S, no pi bond, charge <= 0) and whether a conjugated single bond touches it (a single bond between
//            two pi atoms or a pi atom and a donor); hybridisation from degree + h_count + lone pairs
//   phase 3  thread b owns bond b (strided): type, conjugation, and bond_in_ring by a breadth-first search from one end that may not
//            use the bond itself; it writes the pair word at (i, j) and (j, i)
//            threads 0 .. 127: breadth-first search from atom a over the masks -> row a of the distances, min(30, d), unreachable 30
//            threads 128 .. 255: depth-first search from atom a - 128 for chordless cycles of 3 .. 8 atoms through it.  A path p0 .. pk
//            is extended by w only if w is adjacent to none of p1 .. p(k-1); if w is adjacent to p0 the cycle p0 .. pk w is chordless
//            and the path ends there.
//   phase 4  all threads write the atom rows, the pair rows and the two float blocks with flat indices (coalesced).
// No index is followed out of a table: a bond that leaves its ligand is skipped and a ligand whose rows leave the arrays is not
// written (the host layer refuses both before any launch).
#include "common.h"
#include "mask128.h"
#include "physdock_hip.h"

namespace {

constexpr int LF_MAX_L = PD_LIGAND_FEATURES_MAX_ATOMS;
constexpr int LF_MAX_B = PD_LIGAND_FEATURES_MAX_BONDS;
constexpr int LF_MAX_G = 65535;
constexpr int LF_REF = 167, LF_REL = 42, LF_ATOM_ROW = 16, LF_PAIR_ROW = 8, LF_FAR = 30;

// valence electrons by atomic number (index 0 unused): the group of a main-group element, the group number of a transition metal, 3 for
// the lanthanides and actinides (physdock_amd/ligand.py GROUP_ELECTRONS)
__device__ const unsigned char LF_GROUP_ELECTRONS[129] = {
    0, 1, 2,                                                                                    // H He
    1, 2, 3, 4, 5, 6, 7, 8,                                                                     // Li .. Ne
    1, 2, 3, 4, 5, 6, 7, 8,                                                                     // Na .. Ar
    1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 3, 4, 5, 6, 7, 8,                                    // K .. Kr
    1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 3, 4, 5, 6, 7, 8,                                    // Rb .. Xe
    1, 2, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 3, 4, 5, 6, 7, 8,   // Cs .. Rn
    1, 2, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 3, 4, 5, 6, 7, 8,   // Fr .. Og
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// pair word: bit 0 bonded, bits 1-3 type, bits 4-6 truncated order, bit 7 in ring, bit 8 conjugated, bit 9 aromatic
__device__ __forceinline__ int lf_pair_column(unsigned w, int d, int col) {
    switch (col) {
        case 0: return d;
        case 1: return (int)(w & 1u);
        case 2: return (int)((w >> 1) & 7u);
        case 3: return (int)((w >> 4) & 7u);
        case 4: return (int)((w >> 7) & 1u);
        case 5: return (int)((w >> 8) & 1u);
        case 6: return (int)((w >> 9) & 1u);
        default: return 0;
    }
}

__global__ __launch_bounds__(256) void ligand_features_kernel(const int* __restrict__ atom_start, const int* __restrict__ bond_start,
                                                             const long long* __restrict__ pair_start, const int* __restrict__ atoms,
                                                             const int* __restrict__ bonds, signed char* __restrict__ atom_table,
                                                             signed char* __restrict__ pair_table, float* __restrict__ ref_feat,
                                                             float* __restrict__ rel_tok_feat, int n_atoms, int n_bonds,
                                                             long long n_pairs) {
    __shared__ Mask adj[LF_MAX_L];
    __shared__ unsigned char dist[LF_MAX_L * LF_MAX_L];
    __shared__ unsigned short pairw[LF_MAX_L * LF_MAX_L];
    __shared__ signed char a_table[LF_MAX_L][LF_ATOM_ROW];
    __shared__ unsigned char a_pi[LF_MAX_L], a_donor[LF_MAX_L], a_conj[LF_MAX_L];

    const int g = blockIdx.x, tid = threadIdx.x;
    const int a0 = atom_start[g], a1 = atom_start[g + 1], b0 = bond_start[g], b1 = bond_start[g + 1];
    const long long p0 = pair_start[g];
    const int L = a1 - a0, nb = b1 - b0;
    if (a0 < 0 || L < 1 || L > LF_MAX_L || a1 > n_atoms || b0 < 0 || nb < 0 || nb > LF_MAX_B || b1 > n_bonds || p0 < 0 ||
        p0 + (long long)L * L > n_pairs)
        return;                                              // (uniform over the block)
    const int* my_atoms = atoms + 4 * (long long)a0;
    const int* my_bonds = bonds + 4 * (long long)b0;

    for (int e = tid; e < L * L; e += 256) pairw[e] = 0;
    // ---- phase 1: per atom, from the bond list
    int z = 0, charge = 0, h = 0, flags = 0, deg = 0, n_arom = 0, sum2 = 0;
    if (tid < L) {
        z = my_atoms[4 * tid]; charge = my_atoms[4 * tid + 1]; h = my_atoms[4 * tid + 2]; flags = my_atoms[4 * tid + 3];
        Mask m = {0ull, 0ull};
        bool pi = false;
        for (int b = 0; b < nb; ++b) {
            const int i = my_bonds[4 * b], j = my_bonds[4 * b + 1], o2 = my_bonds[4 * b + 2];
            if ((unsigned)i >= (unsigned)L || (unsigned)j >= (unsigned)L || i == j) continue;
            if (i != tid && j != tid) continue;
            m = mk_or(m, mk_bit(i == tid ? j : i));
            ++deg;
            if (o2 == 3) ++n_arom; else sum2 += o2;
            pi = pi || o2 >= 3;
        }
        adj[tid] = m;
        a_pi[tid] = pi ? 1 : 0;
        a_donor[tid] = (!pi && charge <= 0 && (z == 7 || z == 8 || z == 16)) ? 1 : 0;
    }
    __syncthreads();
    // ---- phase 2: per atom, a conjugated single bond touches it; hybridisation
    if (tid < L) {
        bool on_conj = false;
        for (int b = 0; b < nb; ++b) {
            const int i = my_bonds[4 * b], j = my_bonds[4 * b + 1], o2 = my_bonds[4 * b + 2];
            if ((unsigned)i >= (unsigned)L || (unsigned)j >= (unsigned)L || i == j) continue;
            if ((i != tid && j != tid) || o2 != 2) continue;
            on_conj = on_conj || (a_pi[i] && a_pi[j]) || (a_pi[i] && a_donor[j]) || (a_donor[i] && a_pi[j]);
        }
        a_conj[tid] = on_conj ? 1 : 0;
        const int v = h + (sum2 >> 1) + (n_arom ? n_arom + 1 : 0);
        const int ge = (unsigned)z <= 128u ? (int)LF_GROUP_ELECTRONS[z] : 0;
        int lone = ge - charge - v;
        lone = lone > 0 ? lone >> 1 : 0;
        const int n = deg + h + lone;
        int hyb = n <= 1 ? 0 : (n <= 6 ? n - 1 : 6);
        if (a_donor[tid] && n == 4 && on_conj) hyb = 2;
        const int chiral = (flags >> 1) & 3;
        signed char* row = a_table[tid];
        row[0] = (signed char)charge;
        row[1] = (signed char)(z - 1);
        row[2] = (signed char)(((flags & 1) || n_arom) ? 1 : 0);
        row[3] = (signed char)(deg < 8 ? deg : 8);
        row[4] = (signed char)hyb;
        row[5] = (signed char)(h < 8 ? h : 8);
        row[6] = (signed char)(chiral == 2 ? 0 : (chiral == 1 ? 1 : 2));
        for (int c = 13; c < LF_ATOM_ROW; ++c) row[c] = 0;
    }
    __syncthreads();
    // ---- phase 3a: per bond
    for (int b = tid; b < nb; b += 256) {
        const int i = my_bonds[4 * b], j = my_bonds[4 * b + 1], o2 = my_bonds[4 * b + 2];
        if ((unsigned)i >= (unsigned)L || (unsigned)j >= (unsigned)L || i == j) continue;
        const unsigned type = o2 == 2 ? 0u : (o2 == 4 ? 1u : (o2 == 6 ? 2u : (o2 == 3 ? 3u : 4u)));
        const bool arom = o2 == 3;
        bool conj = arom;
        if (o2 == 2) conj = (a_pi[i] && a_pi[j]) || (a_pi[i] && a_donor[j]) || (a_donor[i] && a_pi[j]);
        if (o2 >= 4) conj = a_conj[i] || a_conj[j];
        // j from i without the bond (i, j)
        Mask seen = mk_bit(i), front = mk_andn(adj[i], mk_bit(j));
        front = mk_andn(front, seen);
        bool ring = false;
        while (mk_any(front)) {
            if (mk_has(front, j)) { ring = true; break; }
            seen = mk_or(seen, front);
            Mask next = {0ull, 0ull};
            Mask walk = front;
            while (mk_any(walk)) {
                const int k = mk_first(walk);
                walk = mk_andn(walk, mk_bit(k));
                next = mk_or(next, adj[k]);
            }
            front = mk_andn(next, seen);
        }
        const unsigned w = 1u | (type << 1) | ((unsigned)((o2 >> 1) & 7) << 4) | (ring ? 1u << 7 : 0u) | (conj ? 1u << 8 : 0u) |
                           (arom ? 1u << 9 : 0u);
        pairw[i * L + j] = (unsigned short)w;
        pairw[j * L + i] = (unsigned short)w;
    }
    // ---- phase 3b: distances (threads 0 .. 127) and ring sizes (threads 128 .. 255)
    if (tid < L) {
        unsigned char* row = dist + tid * L;
        for (int k = 0; k < L; ++k) row[k] = LF_FAR;
        row[tid] = 0;
        Mask seen = mk_bit(tid), front = mk_andn(adj[tid], seen);
        int d = 1;
        while (mk_any(front)) {
            seen = mk_or(seen, front);
            Mask next = {0ull, 0ull};
            Mask walk = front;
            while (mk_any(walk)) {
                const int k = mk_first(walk);
                walk = mk_andn(walk, mk_bit(k));
                row[k] = (unsigned char)(d < LF_FAR ? d : LF_FAR);
                next = mk_or(next, adj[k]);
            }
            front = mk_andn(next, seen);
            ++d;
        }
    } else if (tid >= 128 && tid - 128 < L) {
        const int s = tid - 128;
        Mask cand[7], chord[7];
        int path[8];
        unsigned sizes = 0;
        Mask inpath = mk_bit(s);
        int k = 0;
        path[0] = s;
        cand[0] = adj[s];
        chord[0] = Mask{0ull, 0ull};
        while (true) {
            if (!mk_any(cand[k])) {
                if (k == 0) break;
                inpath = mk_andn(inpath, mk_bit(path[k]));
                --k;
                continue;
            }
            const int w = mk_first(cand[k]);
            cand[k] = mk_andn(cand[k], mk_bit(w));
            if (k >= 1 && mk_has(adj[w], s)) {              // the cycle p0 .. pk w of k + 2 atoms
                sizes |= 1u << (k + 2);
                continue;
            }
            if (k >= 6) continue;                            // a longer path closes no cycle of 8 atoms or fewer
            chord[k + 1] = k >= 1 ? mk_or(chord[k], adj[path[k]]) : Mask{0ull, 0ull};
            path[k + 1] = w;
            inpath = mk_or(inpath, mk_bit(w));
            cand[k + 1] = mk_andn(mk_andn(adj[w], inpath), chord[k + 1]);
            ++k;
        }
        for (int n = 3; n <= 8; ++n) a_table[s][7 + n - 3] = (signed char)((sizes >> n) & 1u);
    }
    __syncthreads();
    // ---- phase 4: the outputs
    signed char* at = atom_table + (long long)a0 * LF_ATOM_ROW;
    for (int e = tid; e < L * LF_ATOM_ROW; e += 256) at[e] = a_table[e / LF_ATOM_ROW][e % LF_ATOM_ROW];
    float* rf = ref_feat + (long long)a0 * LF_REF;
    for (int e = tid; e < L * LF_REF; e += 256) {
        const int a = e / LF_REF, c = e - a * LF_REF;
        const signed char* row = a_table[a];
        int v = 0;
        if (c < 3) v = 0;                                    // ref_pos: filled by the caller
        else if (c == 3) v = row[0];
        else if (c < 132) v = (c - 4) == row[1];
        else if (c == 132) v = row[2];
        else if (c < 142) v = (c - 133) == row[3];
        else if (c < 149) v = (c - 142) == row[4];
        else if (c < 158) v = (c - 149) == row[5];
        else if (c < 161) v = (c - 158) == row[6];
        else v = row[7 + c - 161];
        rf[e] = (float)v;
    }
    signed char* pt = pair_table + p0 * LF_PAIR_ROW;
    for (int e = tid; e < L * L * LF_PAIR_ROW; e += 256) {
        const int p = e / LF_PAIR_ROW;
        pt[e] = (signed char)lf_pair_column(pairw[p], dist[p], e % LF_PAIR_ROW);
    }
    float* rt = rel_tok_feat + p0 * LF_REL;
    for (int e = tid; e < L * L * LF_REL; e += 256) {
        const int p = e / LF_REL, c = e - p * LF_REL;
        const unsigned w = pairw[p];
        int v;
        if (c < 32) v = c == (int)dist[p];
        else if (c < 37) v = (c - 32) == (int)((w >> 1) & 7u);
        else v = lf_pair_column(w, 0, c == 37 ? 1 : c - 35);          // token_bonds, then as_double, in_ring, conjugated, aromatic
        rt[e] = (float)v;
    }
}

}  // namespace

PD_EXPORT int pd_ligand_features(const int* atom_start, const int* bond_start, const long long* pair_start, const int* atoms,
                                 const int* bonds, signed char* atom_table, signed char* pair_table, float* ref_feat, float* rel_tok_feat,
                                 int G, int n_atoms, int n_bonds, long long n_pairs, void* stream) {
    if (!atom_start || !bond_start || !pair_start || !atoms || !atom_table || !pair_table || !ref_feat || !rel_tok_feat) return PD_ERR_ARG;
    if (G < 1 || n_atoms < G || n_bonds < 0 || n_pairs < n_atoms || (n_bonds > 0 && !bonds)) return PD_ERR_ARG;
    if (pd_misaligned(atom_start, 4) || pd_misaligned(bond_start, 4) || pd_misaligned(pair_start, 8) || pd_misaligned(atoms, 4) ||
        pd_misaligned(bonds, 4) || pd_misaligned(ref_feat, 4) || pd_misaligned(rel_tok_feat, 4))
        return PD_ERR_ARG;
    if (G > LF_MAX_G || n_atoms > (long long)G * LF_MAX_L || n_pairs > (long long)G * LF_MAX_L * LF_MAX_L) return PD_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(ligand_features_kernel, dim3(G), dim3(256), 0, (hipStream_t)stream, atom_start, bond_start, pair_start, atoms, bonds,
                       atom_table, pair_table, ref_feat, rel_tok_feat, n_atoms, n_bonds, n_pairs);
    return pd_check_launch();
}
