// Substructure search: which ligands of a library contain a query pattern, how often and on which atoms?  The exact half of 2-D
// screening next to the fingerprints of fingerprint.hip: reactive-group filters before docking, a series picked by its scaffold, the
// warhead atoms to restrain.  Nothing in the reference does this; the definition is the package's own, written down in
// tests/substructure_ref.py (physdock_amd/smarts.py reads the queries) - not RDKit's.  Integers from end to end.
//
// A query is 1 .. 32 atoms, each a postfix program over a stack of truth values (PD_SUBSTRUCT_OP_*: element, aromatic, degree, h_count,
// connectivity, ring, charge, a class bit, not / and / or), and up to 64 bonds (lo, hi, mask), lo < hi, sorted by hi: the mask names
// the allowed ones of the ten bond states, 2 * order class + ring.  An embedding maps the query atoms injectively to atoms of one
// ligand so that every program is true and every query bond lies on a ligand bond of an allowed state.  The search is depth-first
// in the written order of the query atoms: atom 0 on every atom that passes its program, ascending (an anchor); atom k on the
// neighbours of the image of its parent (its lowest earlier neighbour) that pass program k and are free, ascending.  One candidate
// is one step and every anchor has max_steps of them, so the result does not depend on the schedule, exhausted budgets included.
//
// search_kernel, one block of 128 threads per (ligand, 32 queries): the ligand's graph in LDS (ligand_graph.h, 16 KB of bond states,
// the adjacency masks), then query by query:
//   stage   the bonds, the level starts and the parents; thread a runs the programs on atom a and a wave ballot makes the 128-bit
//           compatibility mask of every query atom - no atomics
//   search  thread a is anchor a: an iterative depth-first search whose stack (the image of every level, one byte) lies in LDS, level-
//           major so that the threads of a wave at one level touch consecutive bytes; the atoms in use are a Mask in registers, the
//           candidates of a level one AND of three masks.  An embedding found is counted, ORed into the thread's hit mask and tested:
//           it is *unique* when the same search restricted to its own atoms finds it first, i.e. it is the lexicographically
//           smallest embedding onto that atom set (a second stack in LDS; nothing is stored)
//   reduce  the counts as two 16-bit halves by wave sums (a 64-bit total, saturated), the hit masks by an LDS atomicOr, which commutes
// The block owns bit q % 32 of its word of both hit rows for every atom of its ligand and writes the words once.  A ligand or a query
// whose rows leave the arrays is not written.  matches_kernel, one block per ligand and one query: the anchors count up to M
// embeddings each, thread 0 makes the prefix sums, the anchors search again and write their rows at their offsets; the rest is -1.
#include "common.h"
#include "ligand_graph.h"

namespace {

constexpr int SS_NT = 128;
constexpr int SS_MAX_G = 65535;
constexpr int SS_MAX_Q = 1024;
constexpr int SS_QA = PD_SUBSTRUCT_MAX_QUERY_ATOMS;
constexpr int SS_QB = PD_SUBSTRUCT_MAX_QUERY_BONDS;
constexpr int SS_OPS = PD_SUBSTRUCT_MAX_OPS;
constexpr int SS_MAX_M = PD_SUBSTRUCT_MAX_MATCHES;

struct SsTables {
    const int *atom_start, *op_start, *ops, *bond_start, *bonds;
    int n_queries, n_atoms, n_ops, n_bonds;
};

struct SsQuery {
    Mask compat[SS_QA];
    unsigned short bmask[SS_QB];
    unsigned char blo[SS_QB];
    unsigned char parent[SS_QA], lvl[SS_QA + 1];
    int nq;
};

struct SsAtom {
    int z, charge, h, deg, cls;
    bool arom, ring;
};

struct SsFound {
    unsigned n, n_unique;
    bool spent;
    Mask hits;
};

__device__ __forceinline__ bool ss_eval(const int* __restrict__ ops, int n, const SsAtom& a) {
    unsigned st = 0;
    for (int i = 0; i < n; ++i) {
        const unsigned op = (unsigned)ops[i];
        const int arg = (int)(op >> 8);
        bool v = false;
        switch (op & 0xFFu) {
            case PD_SUBSTRUCT_OP_NOT: st ^= 1u; continue;
            case PD_SUBSTRUCT_OP_AND: { const unsigned b = st & 1u; st >>= 1; st &= ~1u | b; continue; }
            case PD_SUBSTRUCT_OP_OR: { const unsigned b = st & 1u; st >>= 1; st |= b; continue; }
            case PD_SUBSTRUCT_OP_TRUE: v = true; break;
            case PD_SUBSTRUCT_OP_Z: v = a.z == arg; break;
            case PD_SUBSTRUCT_OP_AROMATIC: v = a.arom; break;
            case PD_SUBSTRUCT_OP_ALIPHATIC: v = !a.arom; break;
            case PD_SUBSTRUCT_OP_DEGREE: v = a.deg == arg; break;
            case PD_SUBSTRUCT_OP_H_COUNT: v = a.h == arg; break;
            case PD_SUBSTRUCT_OP_CONNECTIVITY: v = a.deg + a.h == arg; break;
            case PD_SUBSTRUCT_OP_RING: v = a.ring; break;
            case PD_SUBSTRUCT_OP_CHARGE: v = a.charge == arg - 128; break;
            case PD_SUBSTRUCT_OP_CLASS: v = arg < 32 && ((a.cls >> arg) & 1) != 0; break;
            case PD_SUBSTRUCT_OP_ELEMENT_ALIPHATIC: v = a.z == arg && !a.arom; break;
            case PD_SUBSTRUCT_OP_ELEMENT_AROMATIC: v = a.z == arg && a.arom; break;
            default: break;
        }
        st = (st << 1) | (v ? 1u : 0u);
    }
    return (st & 1u) != 0;
}

// Query q into LDS, its compatibility masks from the programs run on this thread's atom (valid = the thread owns one).  Every
// thread of the block calls it; false (for all of them) when the query's rows leave the tables or break the limits.
__device__ bool ss_stage(SsQuery& Q, const SsTables& T, int q, const SsAtom& atom, bool valid) {
    const int tid = threadIdx.x;
    const int qa0 = T.atom_start[q], qa1 = T.atom_start[q + 1], qb0 = T.bond_start[q], qb1 = T.bond_start[q + 1];
    const int nq = qa1 - qa0, nqb = qb1 - qb0;
    if (qa0 < 0 || nq < 1 || nq > SS_QA || qa1 > T.n_atoms || qb0 < 0 || nqb < 0 || nqb > SS_QB || qb1 > T.n_bonds)
        return false;                                        // (uniform over the block)
    __syncthreads();                                         // the last query is no longer read
    int bad = 0;
    if (tid < nqb) {
        const int lo = T.bonds[4 * (qb0 + tid)], hi = T.bonds[4 * (qb0 + tid) + 1], mask = T.bonds[4 * (qb0 + tid) + 2];
        bad |= lo < 0 || lo >= hi || hi >= nq;
        Q.blo[tid] = (unsigned char)(lo & 31);
        Q.bmask[tid] = (unsigned short)(mask & 0x3FF);
    }
    if (tid <= nq) {                                         // level k owns the bonds whose later atom is k: they are sorted by it
        int below = 0, own = 0, parent = 255;
        for (int b = 0; b < nqb; ++b) {
            const int lo = T.bonds[4 * (qb0 + b)], hi = T.bonds[4 * (qb0 + b) + 1];
            below += hi < tid;
            if (hi == tid) { ++own; parent = lo < parent ? lo : parent; }
            bad |= b > 0 && hi < T.bonds[4 * (qb0 + b - 1) + 1];
        }
        Q.lvl[tid] = (unsigned char)below;
        if (tid < nq) {
            Q.parent[tid] = (unsigned char)(parent & 31);
            bad |= tid > 0 && own == 0;                      // an atom without an earlier neighbour
            const int o0 = T.op_start[qa0 + tid], o1 = T.op_start[qa0 + tid + 1];
            bad |= o0 < 0 || o1 - o0 < 1 || o1 - o0 > SS_OPS || o1 > T.n_ops;
        }
    }
    if (tid == 0) Q.nq = nq;
    if (__syncthreads_or(bad)) return false;
    for (int k = 0; k < nq; ++k) {
        const int o0 = T.op_start[qa0 + k], n = T.op_start[qa0 + k + 1] - o0;
        const bool v = valid && ss_eval(T.ops + o0, n, atom);
        const u64 word = __ballot(v);
        if ((tid & 63) == 0) {
            if (tid == 0) Q.compat[k].lo = word;
            else Q.compat[k].hi = word;
        }
    }
    __syncthreads();
    return true;
}

// are all bonds of query atom k to earlier atoms met when k sits on c?  st: this thread's stack
__device__ __forceinline__ bool ss_bonds_ok(const LigandGraph& G, const SsQuery& Q, const unsigned char* st, int k, int c) {
    for (int e = Q.lvl[k], e1 = Q.lvl[k + 1]; e < e1; ++e) {
        const int s = lg_state(G, c, st[Q.blo[e] * SS_NT]);
        if (s == LG_NONE || !((Q.bmask[e] >> s) & 1)) return false;
    }
    return true;
}

// is the embedding in `st` the first one the search finds among the atoms `own` (the atoms of the embedding itself)?
__device__ bool ss_is_smallest(const LigandGraph& G, const SsQuery& Q, const unsigned char* st, unsigned char* us, Mask own) {
    const int nq = Q.nq;
    if (nq == 1) return true;
    Mask anchors = mk_and(own, Q.compat[0]);
    while (mk_any(anchors)) {
        const int a = mk_first(anchors);
        anchors = mk_andn(anchors, mk_bit(a));
        us[0] = (unsigned char)a;
        Mask used = mk_bit(a);
        int k = 1, last = -1;
        while (k >= 1) {
            Mask cand = mk_and(mk_andn(mk_and(G.adj[us[Q.parent[k] * SS_NT]], Q.compat[k]), used), own);
            if (last >= 0) cand = mk_and(cand, mk_above(last));
            if (!mk_any(cand)) {
                if (--k >= 1) { last = us[k * SS_NT]; used = mk_andn(used, mk_bit(last)); }
                continue;
            }
            const int c = mk_first(cand);
            last = c;
            if (!ss_bonds_ok(G, Q, us, k, c)) continue;
            us[k * SS_NT] = (unsigned char)c;
            if (k == nq - 1) {
                bool same = true;
                for (int j = 0; j < nq; ++j) same = same && us[j * SS_NT] == st[j * SS_NT];
                return same;
            }
            used = mk_or(used, mk_bit(c));
            ++k;
            last = -1;
        }
    }
    return true;                                             // (not reached: the embedding itself is found)
}

// The embeddings with query atom 0 on `anchor`, in order.  want_unique: test every one; count_unique: only unique ones count
// towards `limit` and are written.  out: rows of nq local atom indices, or NULL.  It ends when `limit` embeddings have counted.
__device__ SsFound ss_anchor(const LigandGraph& G, const SsQuery& Q, unsigned char* st, unsigned char* us, int anchor, int max_steps,
                             bool want_unique, bool count_unique, unsigned limit, int* __restrict__ out) {
    SsFound r = {0u, 0u, false, Mask{0ull, 0ull}};
    const int nq = Q.nq;
    if (max_steps < 1) { r.spent = true; return r; }
    int steps = 1, k = 1, last = -1;
    unsigned counted = 0;
    st[0] = (unsigned char)anchor;
    Mask used = mk_bit(anchor);
    bool full = nq == 1;                                     // an embedding stands in the stack
    while (true) {
        if (full) {
            const Mask own = nq == 1 ? used : mk_or(used, mk_bit(st[(nq - 1) * SS_NT]));
            ++r.n;
            r.hits = mk_or(r.hits, own);
            const bool u = want_unique ? ss_is_smallest(G, Q, st, us, own) : true;
            r.n_unique += u ? 1u : 0u;
            if (u || !count_unique) {
                if (out)
                    for (int j = 0; j < nq; ++j) out[(long long)counted * nq + j] = st[j * SS_NT];
                if (++counted >= limit) break;
            }
            full = false;
            if (nq == 1) break;
        }
        if (k < 1) break;
        Mask cand = mk_andn(mk_and(G.adj[st[Q.parent[k] * SS_NT]], Q.compat[k]), used);
        if (last >= 0) cand = mk_and(cand, mk_above(last));
        if (!mk_any(cand)) {
            if (--k >= 1) { last = st[k * SS_NT]; used = mk_andn(used, mk_bit(last)); }
            continue;
        }
        if (steps >= max_steps) { r.spent = true; break; }
        ++steps;
        const int c = mk_first(cand);
        last = c;
        if (!ss_bonds_ok(G, Q, st, k, c)) continue;
        st[k * SS_NT] = (unsigned char)c;
        if (k == nq - 1) { full = true; continue; }
        used = mk_or(used, mk_bit(c));
        ++k;
        last = -1;
    }
    return r;
}

// the ligand's rows and this thread's atom; false (uniform) when the rows leave the arrays
__device__ __forceinline__ bool ss_ligand(const int* atom_start, const int* bond_start, int g, int n_atoms, int n_bonds, int& a0, int& L,
                                          int& b0, int& nb) {
    a0 = atom_start[g];
    b0 = bond_start[g];
    const int a1 = atom_start[g + 1], b1 = bond_start[g + 1];
    L = a1 - a0;
    nb = b1 - b0;
    return !(a0 < 0 || L < 1 || L > LG_MAX_L || a1 > n_atoms || b0 < 0 || nb < 0 || nb > LG_MAX_B || b1 > n_bonds);
}

__device__ __forceinline__ SsAtom ss_atom(const LigandGraph& G, const int* __restrict__ atoms, const int* __restrict__ atom_classes,
                                          int a0, int a, bool valid) {
    SsAtom r = {0, 0, 0, 0, 0, false, false};
    if (!valid) return r;
    const int* row = atoms + 4 * (long long)(a0 + a);
    r.z = row[0]; r.charge = row[1]; r.h = row[2];
    r.deg = G.deg[a];
    r.cls = atom_classes ? atom_classes[a0 + a] : 0;
    r.arom = (row[3] & 1) != 0 || G.arom_bond[a] != 0;
    r.ring = G.ring[a] != 0;
    return r;
}

__global__ __launch_bounds__(SS_NT) void search_kernel(const int* __restrict__ atom_start, const int* __restrict__ bond_start,
                                                       const int* __restrict__ atoms, const int* __restrict__ bonds, SsTables T,
                                                       const int* __restrict__ atom_classes, int* __restrict__ n_embeddings,
                                                       int* __restrict__ n_unique, int* __restrict__ status,
                                                       unsigned* __restrict__ atom_hits, unsigned* __restrict__ anchor_hits, int n_atoms,
                                                       int n_bonds, int max_steps) {
    __shared__ LigandGraph G;
    __shared__ SsQuery Q;
    __shared__ unsigned char stack[2][SS_QA][SS_NT];
    __shared__ unsigned hit[4];
    __shared__ int red[2][4];

    const int g = blockIdx.x, chunk = blockIdx.y, tid = threadIdx.x;
    int a0, L, b0, nb;
    if (!ss_ligand(atom_start, bond_start, g, n_atoms, n_bonds, a0, L, b0, nb)) return;
    lg_build<SS_NT>(G, bonds + 4 * (long long)b0, L, nb);
    const bool valid = tid < L;
    const SsAtom atom = ss_atom(G, atoms, atom_classes, a0, tid, valid);
    const int QW = (T.n_queries + 31) / 32;
    unsigned atom_word = 0, anchor_word = 0;

    for (int qi = 0; qi < 32; ++qi) {
        const int q = 32 * chunk + qi;
        if (q >= T.n_queries) break;
        if (!ss_stage(Q, T, q, atom, valid)) continue;
        if (tid < 4) hit[tid] = 0;
        SsFound f = {0u, 0u, false, Mask{0ull, 0ull}};
        if (valid && mk_has(Q.compat[0], tid))
            f = ss_anchor(G, Q, &stack[0][0][tid], &stack[1][0][tid], tid, max_steps, true, false, 0xFFFFFFFFu, nullptr);
        __syncthreads();                                     // hit[] is cleared
        if (mk_any(f.hits)) {
            if ((unsigned)f.hits.lo) atomicOr(&hit[0], (unsigned)f.hits.lo);
            if ((unsigned)(f.hits.lo >> 32)) atomicOr(&hit[1], (unsigned)(f.hits.lo >> 32));
            if ((unsigned)f.hits.hi) atomicOr(&hit[2], (unsigned)f.hits.hi);
            if ((unsigned)(f.hits.hi >> 32)) atomicOr(&hit[3], (unsigned)(f.hits.hi >> 32));
        }
        // a thread's counts are below 2^31 (its steps are): two 16-bit halves summed over 128 threads stay below 2^23
        const int s0 = wave_sum((int)(f.n & 0xFFFFu)), s1 = wave_sum((int)(f.n >> 16));
        const int u0 = wave_sum((int)(f.n_unique & 0xFFFFu)), u1 = wave_sum((int)(f.n_unique >> 16));
        if ((tid & 63) == 0) { red[tid >> 6][0] = s0; red[tid >> 6][1] = s1; red[tid >> 6][2] = u0; red[tid >> 6][3] = u1; }
        const int spent = __syncthreads_or(f.spent ? 1 : 0);
        if (tid == 0) {
            const long long n = ((long long)(red[0][1] + red[1][1]) << 16) + (red[0][0] + red[1][0]);
            const long long u = ((long long)(red[0][3] + red[1][3]) << 16) + (red[0][2] + red[1][2]);
            const long long o = (long long)g * T.n_queries + q;
            n_embeddings[o] = n > 0x7FFFFFFFll ? 0x7FFFFFFF : (int)n;
            n_unique[o] = u > 0x7FFFFFFFll ? 0x7FFFFFFF : (int)u;
            status[o] = spent ? 2 : 0;
        }
        if (valid) {
            if ((hit[tid >> 5] >> (tid & 31)) & 1u) atom_word |= 1u << qi;
            if (f.n) anchor_word |= 1u << qi;
        }
    }
    if (valid) {
        atom_hits[(long long)(a0 + tid) * QW + chunk] = atom_word;
        anchor_hits[(long long)(a0 + tid) * QW + chunk] = anchor_word;
    }
}

__global__ __launch_bounds__(SS_NT) void matches_kernel(const int* __restrict__ atom_start, const int* __restrict__ bond_start,
                                                        const int* __restrict__ atoms, const int* __restrict__ bonds, SsTables T,
                                                        const int* __restrict__ atom_classes, int* __restrict__ matches,
                                                        int* __restrict__ n_written, int n_atoms, int n_bonds, int q, int nq, int M,
                                                        int unique_only, int max_steps) {
    __shared__ LigandGraph G;
    __shared__ SsQuery Q;
    __shared__ unsigned char stack[2][SS_QA][SS_NT];
    __shared__ int count[SS_NT], offset[SS_NT];
    __shared__ int total;

    const int g = blockIdx.x, tid = threadIdx.x;
    int a0, L, b0, nb;
    if (!ss_ligand(atom_start, bond_start, g, n_atoms, n_bonds, a0, L, b0, nb)) return;
    lg_build<SS_NT>(G, bonds + 4 * (long long)b0, L, nb);
    const bool valid = tid < L;
    const SsAtom atom = ss_atom(G, atoms, atom_classes, a0, tid, valid);
    if (!ss_stage(Q, T, q, atom, valid) || Q.nq != nq) return;          // (uniform)
    const bool anchor = valid && mk_has(Q.compat[0], tid);
    const bool uniq = unique_only != 0;
    int mine = 0;
    if (anchor) {
        const SsFound f = ss_anchor(G, Q, &stack[0][0][tid], &stack[1][0][tid], tid, max_steps, uniq, uniq, (unsigned)M, nullptr);
        mine = (int)(uniq ? f.n_unique : f.n);               // at most M
    }
    count[tid] = mine;
    __syncthreads();
    if (tid == 0) {
        int s = 0;
        for (int a = 0; a < SS_NT; ++a) { offset[a] = s; s = s + count[a] > M ? M : s + count[a]; }
        total = s;
        n_written[g] = s;
    }
    __syncthreads();
    int* rows = matches + (long long)g * M * nq;
    const int room = M - offset[tid];
    if (anchor && mine > 0 && room > 0)
        ss_anchor(G, Q, &stack[0][0][tid], &stack[1][0][tid], tid, max_steps, uniq, uniq, (unsigned)(mine < room ? mine : room),
                  rows + (long long)offset[tid] * nq);
    for (int e = total * nq + tid; e < M * nq; e += SS_NT) rows[e] = -1;
}

inline int ss_check_tables(const int* atom_start, const int* bond_start, const int* atoms, const int* bonds, const int* q_atom_start,
                           const int* q_op_start, const int* q_ops, const int* q_bond_start, const int* q_bonds,
                           const int* atom_classes, int G, int n_atoms, int n_bonds, int Q, int nqa, int nops, int nqb, int max_steps) {
    if (!atom_start || !bond_start || !atoms || !q_atom_start || !q_op_start || !q_ops || !q_bond_start) return PD_ERR_ARG;
    if (G < 1 || Q < 1 || n_atoms < G || n_bonds < 0 || (n_bonds > 0 && !bonds) || max_steps < 0) return PD_ERR_ARG;
    if (nqb < 0 || (nqb > 0 && !q_bonds)) return PD_ERR_ARG;
    if (pd_misaligned(atom_start, 4) || pd_misaligned(bond_start, 4) || pd_misaligned(atoms, 4) || pd_misaligned(bonds, 4) ||
        pd_misaligned(q_atom_start, 4) || pd_misaligned(q_op_start, 4) || pd_misaligned(q_ops, 4) || pd_misaligned(q_bond_start, 4) ||
        pd_misaligned(q_bonds, 4) || pd_misaligned(atom_classes, 4))
        return PD_ERR_ARG;
    if (G > SS_MAX_G || Q > SS_MAX_Q || n_atoms > (long long)G * LG_MAX_L) return PD_ERR_UNSUPPORTED;
    // a pattern beyond the limits: more atoms, ops or bonds than Q patterns of the largest size can hold
    if (nqa < Q || nqa > Q * SS_QA || nops < nqa || nops > (long long)nqa * SS_OPS || nqb > Q * SS_QB) return PD_ERR_ARG;
    return PD_OK;
}

}  // namespace

PD_EXPORT int pd_substructure_search(const int* atom_start, const int* bond_start, const int* atoms, const int* bonds,
                                     const int* q_atom_start, const int* q_op_start, const int* q_ops, const int* q_bond_start,
                                     const int* q_bonds, const int* atom_classes, int* n_embeddings, int* n_unique, int* status,
                                     unsigned* atom_hits, unsigned* anchor_hits, int n_ligands, int n_atoms, int n_bonds, int n_queries,
                                     int n_query_atoms, int n_ops, int n_query_bonds, int max_steps, void* stream) {
    if (!n_embeddings || !n_unique || !status || !atom_hits || !anchor_hits) return PD_ERR_ARG;
    if (pd_misaligned(n_embeddings, 4) || pd_misaligned(n_unique, 4) || pd_misaligned(status, 4) || pd_misaligned(atom_hits, 4) ||
        pd_misaligned(anchor_hits, 4))
        return PD_ERR_ARG;
    const int rc = ss_check_tables(atom_start, bond_start, atoms, bonds, q_atom_start, q_op_start, q_ops, q_bond_start, q_bonds,
                                   atom_classes, n_ligands, n_atoms, n_bonds, n_queries, n_query_atoms, n_ops, n_query_bonds, max_steps);
    if (rc != PD_OK) return rc;
    const SsTables T = {q_atom_start, q_op_start, q_ops, q_bond_start, q_bonds, n_queries, n_query_atoms, n_ops, n_query_bonds};
    hipLaunchKernelGGL(search_kernel, dim3(n_ligands, (n_queries + 31) / 32), dim3(SS_NT), 0, (hipStream_t)stream, atom_start,
                       bond_start, atoms, bonds, T, atom_classes, n_embeddings, n_unique, status, atom_hits, anchor_hits, n_atoms, n_bonds,
                       max_steps);
    return pd_check_launch();
}

PD_EXPORT int pd_substructure_matches(const int* atom_start, const int* bond_start, const int* atoms, const int* bonds,
                                      const int* q_atom_start, const int* q_op_start, const int* q_ops, const int* q_bond_start,
                                      const int* q_bonds, const int* atom_classes, int* matches, int* n_written, int n_ligands,
                                      int n_atoms, int n_bonds, int n_queries, int n_query_atoms, int n_ops, int n_query_bonds, int query,
                                      int query_atoms, int max_matches, int unique_only, int max_steps, void* stream) {
    if (!matches || !n_written || pd_misaligned(matches, 4) || pd_misaligned(n_written, 4)) return PD_ERR_ARG;
    const int rc = ss_check_tables(atom_start, bond_start, atoms, bonds, q_atom_start, q_op_start, q_ops, q_bond_start, q_bonds,
                                   atom_classes, n_ligands, n_atoms, n_bonds, n_queries, n_query_atoms, n_ops, n_query_bonds, max_steps);
    if (rc != PD_OK) return rc;
    if (query < 0 || query >= n_queries || query_atoms < 1 || query_atoms > SS_QA || max_matches < 1 || max_matches > SS_MAX_M ||
        (unique_only != 0 && unique_only != 1))
        return PD_ERR_ARG;
    const SsTables T = {q_atom_start, q_op_start, q_ops, q_bond_start, q_bonds, n_queries, n_query_atoms, n_ops, n_query_bonds};
    hipLaunchKernelGGL(matches_kernel, dim3(n_ligands), dim3(SS_NT), 0, (hipStream_t)stream, atom_start, bond_start, atoms, bonds, T,
                       atom_classes, matches, n_written, n_atoms, n_bonds, query, query_atoms, max_matches, unique_only, max_steps);
    return pd_check_launch();
}
