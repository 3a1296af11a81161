// The confidence losses of the training-time forward (PhysDock/models/loss.py:184-207,320-532): per-atom lDDT of a pose batch
// against the ground truth (cal_lddt), the token frames of express_coordinates_in_frame, and the binned softmax cross entropy of
// the pLDDT, PDE and PAE heads with its gradient to the logits.  fp32 throughout.  As in loss.hip no [A,T], [T,T] or one-hot
// tensor exists: every atom-token and token-token pair is formed in registers, the target bin of a row on the fly.  Reductions
// are ordered (per-block partials in the caller's workspace, one final block in float64, no floating-point atomics), so a call
// gives the same bits every time; no launcher allocates, reads back or synchronises, so every launch can be captured.
// Every target is a HARD bin of a distance, so divisions that feed a bin index are IEEE `/` and distances are
// sqrt((dx^2 + dy^2) + dz^2) without contraction: lDDT is a ratio of two sums of multiples of 0.25, exact in fp32 in any order.
#include "common.h"
#include "physdock_hip.h"

namespace {

constexpr int LA = 256;          // atoms per block of the lDDT kernel (one lane per atom)
constexpr int LC = 256;          // token centres staged in LDS per round
constexpr int RPW = 16;          // rows (atoms / token pairs) per wave of the cross-entropy kernel, one lane per bin
constexpr int RPB = 4 * RPW;     // rows per block of 4 waves
constexpr int FR = 13;           // floats per token frame: e1, e2, e3, origin b, valid

enum { MODE_PLDDT = -1, MODE_PDE = 0, MODE_PAE = 1 };

__device__ __forceinline__ float dist2_rn(float dx, float dy, float dz) {     // as loss.hip: (dx^2 + dy^2) + dz^2, no contraction
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// ------------------------------------------------------------------ cal_lddt (loss.py:320-372)
// block = (tile of LA atoms, pose b); the T centres of the pose and of x_gt are staged LC at a time, every lane reads them as
// LDS broadcasts.  lddt[b][a] = sum_t w_t score_t / sum_t w_t, w = ((d_gt < 30) nuc + (d_gt < 15) (1 - nuc)) polymer,
// score = 1/4 #{c in .5, 1, 2, 4 : |d_pred - d_gt| < c}; no epsilon: an empty inclusion set gives 0 / 0 = NaN as in the reference.
__global__ __launch_bounds__(LA) void lddt_atoms_kernel(const float* __restrict__ xp, const float* __restrict__ xg,
                                                       const long long* __restrict__ centre, const float* __restrict__ is_dna,
                                                       const float* __restrict__ is_rna, const float* __restrict__ is_polymer,
                                                       float* __restrict__ out, int A, int T) {
    __shared__ float sp[LC * 3], sg[LC * 3], snuc[LC], spol[LC];
    const int a = blockIdx.x * LA + threadIdx.x;
    const bool in = a < A;
    const float* X = xp + (long long)blockIdx.y * A * 3;
    const float px = in ? X[3 * a] : 0.f, py = in ? X[3 * a + 1] : 0.f, pz = in ? X[3 * a + 2] : 0.f;
    const float gx = in ? xg[3 * a] : 0.f, gy = in ? xg[3 * a + 1] : 0.f, gz = in ? xg[3 * a + 2] : 0.f;
    float num = 0.f, den = 0.f;
    for (int t0 = 0; t0 < T; t0 += LC) {
        const int n = min(LC, T - t0);
        __syncthreads();
        for (int e = threadIdx.x; e < n; e += LA) {
            const long long c = centre[t0 + e];
            sp[3 * e] = X[3 * c]; sp[3 * e + 1] = X[3 * c + 1]; sp[3 * e + 2] = X[3 * c + 2];
            sg[3 * e] = xg[3 * c]; sg[3 * e + 1] = xg[3 * c + 1]; sg[3 * e + 2] = xg[3 * c + 2];
            snuc[e] = is_dna[t0 + e] + is_rna[t0 + e];
            spol[e] = is_polymer[t0 + e];
        }
        __syncthreads();
        for (int t = 0; t < n; ++t) {
            const float dp = sqrtf(dist2_rn(px - sp[3 * t], py - sp[3 * t + 1], pz - sp[3 * t + 2]));
            const float dg = sqrtf(dist2_rn(gx - sg[3 * t], gy - sg[3 * t + 1], gz - sg[3 * t + 2]));
            const float dl = fabsf(dp - dg);
            const float score = 0.25f * (((dl < 0.5f ? 1.f : 0.f) + (dl < 1.f ? 1.f : 0.f)) + ((dl < 2.f ? 1.f : 0.f) + (dl < 4.f ? 1.f : 0.f)));
            const float nuc = snuc[t];
            const float w = ((dg < 30.f ? 1.f : 0.f) * nuc + (dg < 15.f ? 1.f : 0.f) * (1.f - nuc)) * spol[t];
            num += w * score;
            den += w;
        }
    }
    if (in) out[(long long)blockIdx.y * A + a] = num / den;
}

// ------------------------------------------------------------------ express_coordinates_in_frame (loss.py:184-207)
// one lane per token: frames[t] = e1 | e2 | e3 | b | (cos theta < 0.906308), with the reference's +1e-6 on every component INSIDE
// the three norms (so e1, e2 are not exactly unit vectors, as there)
__device__ __forceinline__ float norm_eps(float x, float y, float z) { return sqrtf(dist2_rn(x + 1e-6f, y + 1e-6f, z + 1e-6f)); }

__global__ __launch_bounds__(256) void conf_frames_kernel(const float* __restrict__ x, const long long* __restrict__ f0,
                                                         const long long* __restrict__ f1, const long long* __restrict__ f2,
                                                         float* __restrict__ frames, int T) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const long long ia = f0[t], ib = f1[t], ic = f2[t];
    const float bx = x[3 * ib], by = x[3 * ib + 1], bz = x[3 * ib + 2];
    const float ax = x[3 * ia] - bx, ay = x[3 * ia + 1] - by, az = x[3 * ia + 2] - bz;
    const float cx = x[3 * ic] - bx, cy = x[3 * ic + 1] - by, cz = x[3 * ic + 2] - bz;
    const float n1 = norm_eps(ax, ay, az), n2 = norm_eps(cx, cy, cz);
    const float w1x = ax / n1, w1y = ay / n1, w1z = az / n1, w2x = cx / n2, w2y = cy / n2, w2z = cz / n2;
    const float cosv = __fadd_rn(__fadd_rn(__fmul_rn(w1x, w2x), __fmul_rn(w1y, w2y)), __fmul_rn(w1z, w2z));
    const float sx = w1x + w2x, sy = w1y + w2y, sz = w1z + w2z, dx = w2x - w1x, dy = w2y - w1y, dz = w2z - w1z;
    const float ns = norm_eps(sx, sy, sz), nd = norm_eps(dx, dy, dz);
    const float e1x = sx / ns, e1y = sy / ns, e1z = sz / ns, e2x = dx / nd, e2y = dy / nd, e2z = dz / nd;
    float* o = frames + (long long)t * FR;
    o[0] = e1x; o[1] = e1y; o[2] = e1z;
    o[3] = e2x; o[4] = e2y; o[5] = e2z;
    o[6] = __fsub_rn(__fmul_rn(e1y, e2z), __fmul_rn(e1z, e2y));
    o[7] = __fsub_rn(__fmul_rn(e1z, e2x), __fmul_rn(e1x, e2z));
    o[8] = __fsub_rn(__fmul_rn(e1x, e2y), __fmul_rn(e1y, e2x));
    o[9] = bx; o[10] = by; o[11] = bz;
    o[12] = cosv < 0.906308f ? 1.f : 0.f;
}

// coordinates of point q in frame F (R d, R rows e1, e2, e3)
__device__ __forceinline__ void in_frame(const float* __restrict__ F, float qx, float qy, float qz, float& u0, float& u1, float& u2) {
    const float dx = qx - F[9], dy = qy - F[10], dz = qz - F[11];
    u0 = __fadd_rn(__fadd_rn(__fmul_rn(F[0], dx), __fmul_rn(F[1], dy)), __fmul_rn(F[2], dz));
    u1 = __fadd_rn(__fadd_rn(__fmul_rn(F[3], dx), __fmul_rn(F[4], dy)), __fmul_rn(F[5], dz));
    u2 = __fadd_rn(__fadd_rn(__fmul_rn(F[6], dx), __fmul_rn(F[7], dy)), __fmul_rn(F[8], dz));
}

// ------------------------------------------------------------------ binned softmax cross entropy (loss.py:375-532)
struct CeArgs {
    const float* logits;            // [R][nb]
    const float* ex;                // x_exists [A]
    const float* lddt;              // pLDDT: lDDT of pose 0 [A]
    const float* xp;                // pairs: pose 0 [A][3]
    const float* xg;                // pairs: x_gt [A][3]
    const long long* centre;        // pairs: [T]
    const float* fp;                // PAE: frames of pose 0 [T][13]
    const float* fg;                // PAE: frames of x_gt [T][13]
    float min_bin, range;           // pairs: bin = clamp(long((e - min_bin) / range * nb), 0, nb - 1)
    int nb, T;
    long long R;                    // rows: A (pLDDT) or T * T
};

// torch.clamp(v.long(), 0, nb - 1); a NaN goes to bin 0 (its conversion is the most negative integer there)
__device__ __forceinline__ int to_bin(float v, int nb) {
    if (!(v >= 0.f)) return 0;
    return v >= (float)nb ? nb - 1 : (int)v;
}

// sum of the row masks in float64: pLDDT sum_a e_a, pairs sum_ij e_ci e_cj = (sum_i e_ci)^2
__device__ __forceinline__ double mask_sum(const float* __restrict__ ex, const long long* __restrict__ centre, int n, double* sh) {
    double s = 0;
    for (int t = threadIdx.x; t < n; t += 256) s += centre ? ex[centre[t]] : ex[t];
    s = block_sum_det<256>(s, sh);
    return centre ? s * s : s;
}

// coef[0] = scale / (1e-9 + sum m); a zero scale gives an exact zero
__global__ __launch_bounds__(256) void conf_ce_coef(const float* __restrict__ ex, const long long* __restrict__ centre,
                                                   const float* __restrict__ scale, float* __restrict__ coef, int n) {
    __shared__ double sh[256];
    const double s = mask_sum(ex, centre, n, sh);
    if (threadIdx.x == 0) coef[0] = scale[0] == 0.f ? 0.f : (float)((double)scale[0] / (1e-9 + s));
}

// One wave per row, one lane per bin (nb <= 64): the row of logits is read once, coalesced; lanes 0..RPW-1 first form the target
// bin and the mask m of the wave's RPW rows, which are then broadcast row by row.  Per row
//   ce = -m (z_bin - log sum_c exp z_c), z = p m        (label m . log_softmax(p m))
//   g  = coef m^3 (softmax(z) - onehot(bin))             (written where grad is given; an exact zero where m = 0 or coef = 0)
// part[blk] = sum over the block's rows of m ce, the four waves added in a fixed order.
template <int MODE>
__global__ __launch_bounds__(256) void conf_ce_kernel(CeArgs a, const float* __restrict__ coefp, float* __restrict__ part,
                                                     float* __restrict__ grad) {
    __shared__ float red[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nb = a.nb;
    const long long r0 = (long long)blockIdx.x * RPB + w * RPW;
    int bin = 0;
    float m = 0.f;
    if (lane < RPW && r0 + lane < a.R) {
        const long long r = r0 + lane;
        if (MODE == MODE_PLDDT) {
            m = a.ex[r];
            bin = to_bin(a.lddt[r] * (float)nb, nb);
        } else {
            const int i = (int)(r / a.T), j = (int)(r % a.T);
            const long long ci = a.centre[i], cj = a.centre[j];
            m = a.ex[ci] * a.ex[cj];
            float e;
            if (MODE == MODE_PDE) {
                const float dp = sqrtf(dist2_rn(a.xp[3 * ci] - a.xp[3 * cj], a.xp[3 * ci + 1] - a.xp[3 * cj + 1], a.xp[3 * ci + 2] - a.xp[3 * cj + 2]));
                const float dg = sqrtf(dist2_rn(a.xg[3 * ci] - a.xg[3 * cj], a.xg[3 * ci + 1] - a.xg[3 * cj + 1], a.xg[3 * ci + 2] - a.xg[3 * cj + 2]));
                e = fabsf(dp - dg);
            } else {
                const float* Fp = a.fp + (long long)i * FR;
                const float* Fg = a.fg + (long long)i * FR;
                float p0, p1, p2, g0, g1, g2;
                in_frame(Fp, a.xp[3 * cj], a.xp[3 * cj + 1], a.xp[3 * cj + 2], p0, p1, p2);
                in_frame(Fg, a.xg[3 * cj], a.xg[3 * cj + 1], a.xg[3 * cj + 2], g0, g1, g2);
                e = sqrtf(dist2_rn(p0 - g0, p1 - g1, p2 - g2)) * Fg[12] * Fp[12];
            }
            bin = to_bin((e - a.min_bin) / a.range * (float)nb, nb);
        }
    }
    const float coef = grad ? coefp[0] : 0.f;
    const bool on = lane < nb;
    float acc = 0.f;
    for (int rr = 0; rr < RPW; ++rr) {
        const long long row = r0 + rr;
        if (row >= a.R) break;                                              // wave-uniform
        const float mr = __shfl(m, rr);
        const int br = __shfl(bin, rr);
        const float z = on ? a.logits[row * nb + lane] * mr : -INFINITY;
        const float mx = wave_max(z);
        const float ez = on ? expf(z - mx) : 0.f;
        const float s = wave_sum(ez);
        const float zb = __shfl(z, br);
        const float ce = -mr * ((zb - mx) - logf(s));
        acc += mr * ce;                                                     // not skipped where m = 0: 0 * NaN stays NaN as in the reference
        if (grad && on) {
            const float f = coef * (mr * mr * mr);
            grad[row * nb + lane] = (coef == 0.f || mr == 0.f) ? 0.f : f * (ez / s - (lane == br ? 1.f : 0.f));
        }
    }
    if (lane == 0) red[w] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// out = sum_blk part / (1e-9 + sum m) (masked_mean), partials added in a fixed order in float64
__global__ __launch_bounds__(256) void conf_ce_final(const float* __restrict__ part, const float* __restrict__ ex,
                                                    const long long* __restrict__ centre, float* __restrict__ out, int n, int nblk) {
    __shared__ double sh[256];
    const double sm = mask_sum(ex, centre, n, sh);
    double se = 0;
    for (int e = threadIdx.x; e < nblk; e += 256) se += part[e];
    se = block_sum_det<256>(se, sh);
    if (threadIdx.x == 0) out[0] = (float)(se / (1e-9 + sm));
}

inline long long ce_blocks(long long R) { return (R + RPB - 1) / RPB; }

template <int MODE>
int launch_ce(const CeArgs& a, int n_mask, const float* scale, float* ws, float* out, float* grad, hipStream_t st) {
    const long long nblk = ce_blocks(a.R);
    if (nblk > 0x7fffffffLL) return PD_ERR_UNSUPPORTED;
    float* coef = ws;
    float* part = ws + 4;
    if (grad) hipLaunchKernelGGL(conf_ce_coef, dim3(1), dim3(256), 0, st, a.ex, a.centre, scale, coef, n_mask);
    hipLaunchKernelGGL(conf_ce_kernel<MODE>, dim3((unsigned)nblk), dim3(256), 0, st, a, coef, part, grad);
    hipLaunchKernelGGL(conf_ce_final, dim3(1), dim3(256), 0, st, part, a.ex, a.centre, out, n_mask, (int)nblk);
    return pd_check_launch();
}

}  // namespace

PD_EXPORT int pd_conf_loss_workspace_numel(int B, int A, int T) {
    if (B < 1 || A < 1 || T < 1) return PD_ERR_ARG;
    const long long R = (long long)T * T > A ? (long long)T * T : A;
    const long long n = 4 + ce_blocks(R);                                   // coef (+3 pad) + one partial per block of 64 rows
    return n > 0x7fffffffLL ? PD_ERR_UNSUPPORTED : (int)n;
}

PD_EXPORT int pd_lddt_atoms(const float* x_pred, const float* x_gt, const long long* centre, const float* is_dna, const float* is_rna,
                            const float* is_polymer, float* lddt, int B, int A, int T, void* stream) {
    if (!x_pred || !x_gt || !centre || !is_dna || !is_rna || !is_polymer || !lddt || B < 1 || A < 1 || T < 1) return PD_ERR_ARG;
    if (B > 65535) return PD_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(lddt_atoms_kernel, dim3((A + LA - 1) / LA, B), dim3(LA), 0, (hipStream_t)stream, x_pred, x_gt, centre, is_dna,
                       is_rna, is_polymer, lddt, A, T);
    return pd_check_launch();
}

PD_EXPORT int pd_conf_frames(const float* x, const long long* frame_atom_0, const long long* frame_atom_1,
                             const long long* frame_atom_2, float* frames, int A, int T, void* stream) {
    if (!x || !frame_atom_0 || !frame_atom_1 || !frame_atom_2 || !frames || A < 1 || T < 1) return PD_ERR_ARG;
    hipLaunchKernelGGL(conf_frames_kernel, dim3((T + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, frame_atom_0, frame_atom_1,
                       frame_atom_2, frames, T);
    return pd_check_launch();
}

PD_EXPORT int pd_conf_loss_plddt(const float* p_plddt, const float* lddt, const float* x_exists, int no_bins, const float* scale,
                                 float* ws, float* out, float* g_plddt, int A, void* stream) {
    if (!p_plddt || !lddt || !x_exists || !ws || !out || (g_plddt && !scale) || A < 1 || no_bins < 1) return PD_ERR_ARG;
    if (no_bins > 64) return PD_ERR_UNSUPPORTED;                            // one lane per bin
    CeArgs a = {p_plddt, x_exists, lddt, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 1.f, no_bins, 1, (long long)A};
    return launch_ce<MODE_PLDDT>(a, A, scale, ws, out, g_plddt, (hipStream_t)stream);
}

PD_EXPORT int pd_conf_loss_pairs(int mode, const float* p_pair, const float* x_pred0, const float* x_gt, const float* x_exists,
                                 const long long* centre, const float* frames_pred, const float* frames_gt, float min_bin,
                                 float bin_range, int no_bins, const float* scale, float* ws, float* out, float* g_pair, int A, int T,
                                 void* stream) {
    if (!p_pair || !x_pred0 || !x_gt || !x_exists || !centre || !ws || !out || (g_pair && !scale) || A < 1 || T < 1 || no_bins < 1 ||
        (mode != MODE_PDE && mode != MODE_PAE) || (mode == MODE_PAE && (!frames_pred || !frames_gt)))
        return PD_ERR_ARG;
    if (no_bins > 64) return PD_ERR_UNSUPPORTED;
    CeArgs a = {p_pair, x_exists, nullptr, x_pred0, x_gt, centre, frames_pred, frames_gt, min_bin, bin_range, no_bins, T, (long long)T * T};
    return mode == MODE_PDE ? launch_ce<MODE_PDE>(a, T, scale, ws, out, g_pair, (hipStream_t)stream)
                            : launch_ce<MODE_PAE>(a, T, scale, ws, out, g_pair, (hipStream_t)stream);
}
