// One ligand's graph in LDS for the kernels that walk it (substructure.hip): the bond list, the adjacency as one 128-bit mask per atom,
// the bridge flag of every bond and the state of the bond between two atoms as a byte matrix.  The steps are phases 0 - 2 of
// morgan_kernel (fingerprint.hip) and the bridge test is bond_in_ring of pd_ligand_features: a breadth-first search from one end of
// the bond that may not use the bond itself.  A bond that leaves its ligand or joins an atom to itself is marked and skipped.
#pragma once
#include "mask128.h"
#include "physdock_hip.h"

constexpr int LG_MAX_L = PD_LIGAND_FEATURES_MAX_ATOMS;
constexpr int LG_MAX_B = PD_LIGAND_FEATURES_MAX_BONDS;
constexpr unsigned char LG_NONE = 0xFF;

struct LigandGraph {
    Mask adj[LG_MAX_L];
    unsigned state[LG_MAX_L][LG_MAX_L / 4];                 // bytes: the state of the bond (a, b), LG_NONE without one
    int bo[LG_MAX_B];
    unsigned char bi[LG_MAX_B], bj[LG_MAX_B], bridge[LG_MAX_B];
    unsigned char deg[LG_MAX_L], ring[LG_MAX_L], arom_bond[LG_MAX_L];
};

// the state of a bond: 2 * (0 single, 1 double, 2 triple, 3 aromatic, 4 other) + (1 when it is no bridge), bond_type of ligand.py
__device__ __forceinline__ int lg_bond_state(int o2, bool in_ring) {
    const int cls = o2 == 2 ? 0 : (o2 == 4 ? 1 : (o2 == 6 ? 2 : (o2 == 3 ? 3 : 4)));
    return 2 * cls + (in_ring ? 1 : 0);
}
__device__ __forceinline__ int lg_state(const LigandGraph& g, int a, int b) {
    return ((const unsigned char*)g.state[a])[b];
}

// All NT threads of the block call it; L atoms (1 .. LG_MAX_L), nb bonds (0 .. LG_MAX_B), my_bonds the ligand's rows (i, j, o2, -).
// On return (after its last barrier) every field is set.
template <int NT>
__device__ __forceinline__ void lg_build(LigandGraph& g, const int* __restrict__ my_bonds, int L, int nb) {
    const int tid = threadIdx.x;
    for (int b = tid; b < nb; b += NT) {
        const int i = my_bonds[4 * b], j = my_bonds[4 * b + 1];
        const bool ok = (unsigned)i < (unsigned)L && (unsigned)j < (unsigned)L && i != j;
        g.bi[b] = ok ? (unsigned char)i : LG_NONE;
        g.bj[b] = ok ? (unsigned char)j : LG_NONE;
        g.bo[b] = my_bonds[4 * b + 2];
        g.bridge[b] = 1;
    }
    for (int e = tid; e < LG_MAX_L * (LG_MAX_L / 4); e += NT) (&g.state[0][0])[e] = 0xFFFFFFFFu;
    __syncthreads();
    for (int a = tid; a < L; a += NT) {
        Mask m = {0ull, 0ull};
        int d = 0, ar = 0;
        for (int b = 0; b < nb; ++b) {
            const int i = g.bi[b], j = g.bj[b];
            if (i == LG_NONE || (i != a && j != a)) continue;
            m = mk_or(m, mk_bit(i == a ? j : i));
            ++d;
            ar |= g.bo[b] == 3;
        }
        g.adj[a] = m;
        g.deg[a] = (unsigned char)(d > 255 ? 255 : d);
        g.arom_bond[a] = (unsigned char)ar;
    }
    __syncthreads();
    for (int b = tid; b < nb; b += NT) {
        const int i = g.bi[b], j = g.bj[b];
        if (i == LG_NONE) continue;
        Mask seen = mk_bit(i), front = mk_andn(mk_andn(g.adj[i], mk_bit(j)), seen);     // j from i without the bond (i, j)
        bool ring = false;
        while (mk_any(front)) {
            if (mk_has(front, j)) { ring = true; break; }
            seen = mk_or(seen, front);
            Mask next = {0ull, 0ull}, walk = front;
            while (mk_any(walk)) {
                const int k = mk_first(walk);
                walk = mk_andn(walk, mk_bit(k));
                next = mk_or(next, g.adj[k]);
            }
            front = mk_andn(next, seen);
        }
        g.bridge[b] = ring ? 0 : 1;
        const unsigned char s = (unsigned char)lg_bond_state(g.bo[b], ring);
        ((unsigned char*)g.state[i])[j] = s;
        ((unsigned char*)g.state[j])[i] = s;
    }
    __syncthreads();
    for (int a = tid; a < L; a += NT) {
        int r = 0;
        for (int b = 0; b < nb; ++b) {
            const int i = g.bi[b], j = g.bj[b];
            if (i != LG_NONE && (i == a || j == a) && !g.bridge[b]) r = 1;
        }
        g.ring[a] = (unsigned char)r;
    }
    __syncthreads();
}
