// Gradients of the five loss terms (loss.hip) with respect to the network's outputs x_denoised [B,A,3] and p_distogram [T,T,bins]:
// the first stage of a backward pass.  What is built is what torch autograd gives for the reference's code (PhysDock/models/
// loss.py:78-181,245-318,535-559): |.| has derivative 0 at 0, a zero distance has a zero direction, torch.clamp blocks the weighted
// MSE above 1e4.  As in the forward, no [B,A,A], [B,T,T] or [T,T,bins] intermediate exists (g_p is the one [T,T,bins] array, the
// output); every reduction is ordered (no floating-point atomics), so a call gives the same bits every time, and no launch
// allocates or reads back, so the backward can be captured.
// Each launcher reads its upstream scale from device memory (term weight x upstream gradient x finite flag, formed by the caller):
// a zero scale writes / adds an exact zero, never 0 * NaN, so a skipped non-finite term adds no gradient.  The x launchers write
// (accumulate = 0) or add to (accumulate = 1) one g_x; the caller fixes the launch order.
#include "loss_common.h"
#include "physdock_hip.h"

namespace {

constexpr int GT = 64;        // row atoms per block of the smooth-lDDT sweep (one lane per row atom)
constexpr int GB = 4;         // samples per block: the ground-truth distances of a tile are formed once per GB samples
constexpr int GS = 16;        // columns per wave (strip of a 64-column tile)
constexpr int GQ = 4;         // column tiles in flight per block: 16 waves = 4 tiles x 4 strips

__device__ __forceinline__ float dist2_rn(float dx, float dy, float dz) {     // as loss.hip: (dx^2 + dy^2) + dz^2, no contraction
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// sigmoid(d - c) for c = 0.5, 1, 2, 4 from one exponential e = exp(-d), as loss.hip's lddt_eps4
struct Sig4 { float s0, s1, s2, s3; };
__device__ __forceinline__ Sig4 sig4(float d) {
    const float e = __builtin_amdgcn_exp2f(-PD_LOG2E * d);
    return {__builtin_amdgcn_rcpf(fmaf(1.6487212707f, e, 1.f)), __builtin_amdgcn_rcpf(fmaf(2.7182818285f, e, 1.f)),
            __builtin_amdgcn_rcpf(fmaf(7.3890560989f, e, 1.f)), __builtin_amdgcn_rcpf(fmaf(54.598150033f, e, 1.f))};
}
// 4 eps'(d) = sum_c s (1 - s)
__device__ __forceinline__ float dsig4(const Sig4& s) {
    return (fmaf(-s.s0, s.s0, s.s0) + fmaf(-s.s1, s.s1, s.s1)) + (fmaf(-s.s2, s.s2, s.s2) + fmaf(-s.s3, s.s3, s.s3));
}
__device__ __forceinline__ float sgn(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }     // torch.sign: 0 at 0

// ------------------------------------------------------------------ smooth lDDT (loss.py:162-181)
// d loss / d x_bi = (1/B) / (1e-9 + sum m) * sum_j 2 m_ij eps'(delta_ij) sign(delta_ij) (x_i - x_j) / d_ij  (m symmetric).
// Full-row sweep: block = (row tile of 64 atoms, GB samples), lane = row atom; the 16 waves take 4 column tiles at a time, wave w
// the 16-column strip (w & 3) of tile 4 k + (w >> 2).  Each unordered pair is visited twice (once from each row), no partial
// gradient leaves the block: the 16 waves' sums are added in a fixed order in LDS.  Strips without a pair inside the clamp are
// skipped as in the forward.  raw[b][i][c] = sum_j m_ij 4 eps' sign (x_i - x_j)_c / d_ij; cnt[ti] = sum over the tile's rows of
// sum_j m_ij (written by the blocks of the first sample chunk).
__global__ __launch_bounds__(1024) void smooth_lddt_grad_kernel(const float* __restrict__ xd, const float* __restrict__ xg,
                                                               const float* __restrict__ ex, float clamp, const float* __restrict__ scale,
                                                               float* __restrict__ raw, float* __restrict__ cnt, int B, int A, int nt) {
    __shared__ float sxj[GQ][GB][GT * 3];
    __shared__ float sgj[GQ][GT * 3], sej[GQ][GT];
    __shared__ float sacc[8][GB * GT * 3];
    __shared__ float scnt[16];
    if (scale[0] == 0.f) return;                                        // block-uniform: the term is skipped
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, strip = w & 3, q = w >> 2, gtid = tid & 255;
    const int ti = blockIdx.x, b0 = blockIdx.y * GB, nb = min(GB, B - b0);
    const int i = ti * GT + lane;
    const bool in = i < A;
    const float gx = in ? xg[3 * i] : 0.f, gy = in ? xg[3 * i + 1] : 0.f, gz = in ? xg[3 * i + 2] : 0.f, ei = in ? ex[i] : 0.f;
    float px[GB], py[GB], pz[GB], ax[GB], ay[GB], az[GB];
#pragma unroll
    for (int bb = 0; bb < GB; ++bb) {
        const long long o = ((long long)(b0 + bb) * A + i) * 3;
        const bool ok = in && bb < nb;
        px[bb] = ok ? xd[o] : 0.f; py[bb] = ok ? xd[o + 1] : 0.f; pz[bb] = ok ? xd[o + 2] : 0.f;
        ax[bb] = 0.f; ay[bb] = 0.f; az[bb] = 0.f;
    }
    float c = 0.f;
    for (int t0 = 0; t0 < nt; t0 += GQ) {
        const int tj = t0 + q, j0 = tj * GT;
        __syncthreads();
        if (tj < nt) {
            for (int e = gtid; e < nb * GT * 3; e += 256) {
                const int bb = e / (GT * 3), r = e % (GT * 3);
                sxj[q][bb][r] = (j0 * 3 + r < A * 3) ? xd[(long long)(b0 + bb) * A * 3 + j0 * 3 + r] : 0.f;
            }
            if (gtid < GT * 3) sgj[q][gtid] = (j0 * 3 + gtid < A * 3) ? xg[j0 * 3 + gtid] : 0.f;
            if (gtid < GT) sej[q][gtid] = (j0 + gtid < A) ? ex[j0 + gtid] : 0.f;
        }
        __syncthreads();
        if (tj >= nt) continue;                                         // wave-uniform
        float dg[GS], mk[GS];
        unsigned act = 0;
#pragma unroll
        for (int jj = 0; jj < GS; ++jj) {
            const int j = strip * GS + jj;
            dg[jj] = sqrtf(dist2_rn(gx - sgj[q][3 * j], gy - sgj[q][3 * j + 1], gz - sgj[q][3 * j + 2]));
            mk[jj] = (dg[jj] < clamp ? 1.f : 0.f) * ei * sej[q][j];
            c += mk[jj];
            if (__ballot(mk[jj] != 0.f)) act |= 1u << jj;
        }
        if (!act) continue;
#pragma unroll
        for (int bb = 0; bb < GB; ++bb) {
            if (bb >= nb) break;
#pragma unroll
            for (int jj = 0; jj < GS; ++jj) {
                if (!(act >> jj & 1)) continue;                         // wave-uniform
                const int j = strip * GS + jj;
                const float dx = px[bb] - sxj[q][bb][3 * j], dy = py[bb] - sxj[q][bb][3 * j + 1], dz = pz[bb] - sxj[q][bb][3 * j + 2];
                const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                const float r = __builtin_amdgcn_rsqf(d2);
                const float del = d2 * r - dg[jj];
                float f = mk[jj] * dsig4(sig4(fabsf(del))) * sgn(del) * r, ux = dx, uy = dy, uz = dz;
                if (d2 < 1.17549435e-38f) {
                    // zero distance: zero direction.  A d2 below the normal range (two atoms closer than 1e-19) is no zero
                    // distance, but v_rsq_f32 takes it for one and answers inf (f = 0 * inf): form the unit direction from
                    // differences scaled by 2^96.  No d2 >= FLT_MIN comes here, so every other pair keeps its bits.
                    f = 0.f;
                    if (dx != 0.f || dy != 0.f || dz != 0.f) {
                        ux = dx * 0x1p+96f; uy = dy * 0x1p+96f; uz = dz * 0x1p+96f;
                        const float s2 = fmaf(uz, uz, fmaf(uy, uy, ux * ux)), rs = __builtin_amdgcn_rsqf(s2);
                        const float dls = s2 * rs * 0x1p-96f - dg[jj];
                        f = mk[jj] * dsig4(sig4(fabsf(dls))) * sgn(dls) * rs;
                    }
                }
                ax[bb] = fmaf(f, ux, ax[bb]); ay[bb] = fmaf(f, uy, ay[bb]); az[bb] = fmaf(f, uz, az[bb]);
            }
        }
    }
    // fixed-order sum of the 16 waves: waves 8..15 store, waves 0..7 add theirs on top, then slots 0..7 in order
    __syncthreads();
    if (w >= 8) {
#pragma unroll
        for (int bb = 0; bb < GB; ++bb) {
            float* s = sacc[w - 8] + (bb * GT + lane) * 3;
            s[0] = ax[bb]; s[1] = ay[bb]; s[2] = az[bb];
        }
    }
    c = wave_sum(c);
    if (lane == 0) scnt[w] = c;
    __syncthreads();
    if (w < 8) {
#pragma unroll
        for (int bb = 0; bb < GB; ++bb) {
            float* s = sacc[w] + (bb * GT + lane) * 3;
            s[0] = ax[bb] + s[0]; s[1] = ay[bb] + s[1]; s[2] = az[bb] + s[2];
        }
    }
    __syncthreads();
    if (tid < GB * GT * 3) {
        const int bb = tid / (GT * 3), r = tid % (GT * 3), row = ti * GT + r / 3;
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) v += sacc[k][tid];
        if (bb < nb && row < A) raw[((long long)(b0 + bb) * A + row) * 3 + r % 3] = v;
    }
    if (tid == 0 && blockIdx.y == 0) {
        float n = 0.f;
        for (int k = 0; k < 16; ++k) n += scnt[k];
        cnt[ti] = n;
    }
}

// g_x (+)= coef * raw, coef = scale / 2 / (B (1e-9 + sum_t cnt[t])): 1/4 of eps' times the 2 of the symmetric mask
__global__ __launch_bounds__(256) void smooth_lddt_grad_apply(const float* __restrict__ raw, const float* __restrict__ cnt,
                                                             const float* __restrict__ scale, float* __restrict__ g, int B, int A,
                                                             int nt, int accumulate) {
    __shared__ float scoef;
    if (threadIdx.x == 0) {
        double n = 0;
        if (scale[0] != 0.f)                                            // else the sweep did not run and cnt is stale
            for (int t = 0; t < nt; ++t) n += cnt[t];
        scoef = scale[0] == 0.f ? 0.f : (float)((double)scale[0] * 0.5 / ((double)B * (1e-9 + n)));
    }
    __syncthreads();
    const float coef = scoef;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)B * A * 3) return;
    const float v = coef == 0.f ? 0.f : coef * raw[e];
    g[e] = accumulate ? g[e] + v : v;
}

// ------------------------------------------------------------------ bond + key-residue terms (loss.py:245-318,535-559)
// coef[0] = scale_bond * mean_b scale_b(sd_bond) / B / (sum bonds + eps), coef[1] likewise with the key mask and sd_key
__global__ __launch_bounds__(256) void centre_grad_coef(const float* __restrict__ bonds, const float* __restrict__ is_key,
                                                       const float* __restrict__ is_lig, const float* __restrict__ t_hat,
                                                       float sd_bond, float sd_key, float eps, const float* __restrict__ scale,
                                                       float* __restrict__ coef, int B, int T) {
    __shared__ double sh[256];
    double nb = 0, nk = 0, nl = 0;
    for (long long e = threadIdx.x; e < (long long)T * T; e += 256) nb += bonds[e];
    for (int t = threadIdx.x; t < T; t += 256) { nk += is_key[t]; nl += is_lig[t]; }
    nb = block_sum_det<256>(nb, sh); nk = block_sum_det<256>(nk, sh); nl = block_sum_det<256>(nl, sh);
    const double wb = mean_edm_scale(t_hat, B, sd_bond, sh), wk = mean_edm_scale(t_hat, B, sd_key, sh);
    if (threadIdx.x == 0) {
        coef[0] = scale[0] == 0.f ? 0.f : (float)((double)scale[0] * wb / B / (nb + eps));
        coef[1] = scale[1] == 0.f ? 0.f : (float)((double)scale[1] * wk / B / (nk * nl + eps));
    }
}

// one wave per (token i, sample b), lanes over j: tg[b][i] = coef0 sum_j (b_ij + b_ji) 2 diff u_ij
//                                                      + coef1 sum_j (k_i l_j + k_j l_i) 2 eps eps' sign(diff) u_ij,  u_ij = (p_i - p_j) / d_ij
__global__ __launch_bounds__(256) void centre_grad_kernel(const float* __restrict__ xd, const float* __restrict__ xg,
                                                         const long long* __restrict__ centre, const float* __restrict__ bonds,
                                                         const float* __restrict__ is_key, const float* __restrict__ is_lig,
                                                         const float* __restrict__ coef, float* __restrict__ tg, int B, int A, int T) {
    const int lane = threadIdx.x & 63, b = blockIdx.y * 4 + (threadIdx.x >> 6), i = blockIdx.x;
    const float cb = coef[0], ck = coef[1];
    if (b >= B || (cb == 0.f && ck == 0.f)) return;                    // whole wave; no block-level synchronisation below
    const float* X = xd + (long long)b * A * 3;
    const long long ci = centre[i];
    const float px = X[3 * ci], py = X[3 * ci + 1], pz = X[3 * ci + 2];
    const float gx = xg[3 * ci], gy = xg[3 * ci + 1], gz = xg[3 * ci + 2];
    const float ki = is_key[i], li = is_lig[i];
    float bx = 0.f, by = 0.f, bz = 0.f, kx = 0.f, ky = 0.f, kz = 0.f;
    for (int j = lane; j < T; j += 64) {
        const float tb = bonds[(long long)i * T + j] + bonds[(long long)j * T + i], km = ki * is_lig[j] + is_key[j] * li;
        if (tb == 0.f && km == 0.f) continue;
        const long long cj = centre[j];
        const float qx = X[3 * cj], qy = X[3 * cj + 1], qz = X[3 * cj + 2];
        const float dp = sqrtf(dist2_rn(qx - px, qy - py, qz - pz));
        if (!(dp > 0.f)) continue;                                     // zero distance: zero direction (torch.norm at 0)
        const float dgt = sqrtf(dist2_rn(xg[3 * cj] - gx, xg[3 * cj + 1] - gy, xg[3 * cj + 2] - gz));
        const float diff = dp - dgt, inv = 1.f / dp;
        const float fb = tb * 2.f * diff * inv;
        const Sig4 s = sig4(fabsf(diff));
        const float e = 0.25f * ((s.s0 + s.s1) + (s.s2 + s.s3)), ep = 0.25f * dsig4(s);
        const float fk = km * 2.f * e * ep * sgn(diff) * inv;
        const float dx = px - qx, dy = py - qy, dz = pz - qz;
        bx = fmaf(fb, dx, bx); by = fmaf(fb, dy, by); bz = fmaf(fb, dz, bz);
        kx = fmaf(fk, dx, kx); ky = fmaf(fk, dy, ky); kz = fmaf(fk, dz, kz);
    }
    bx = wave_sum(bx); by = wave_sum(by); bz = wave_sum(bz);
    kx = wave_sum(kx); ky = wave_sum(ky); kz = wave_sum(kz);
    if (lane == 0) {
        float* o = tg + ((long long)b * T + i) * 3;
        o[0] = (cb == 0.f ? 0.f : cb * bx) + (ck == 0.f ? 0.f : ck * kx);
        o[1] = (cb == 0.f ? 0.f : cb * by) + (ck == 0.f ? 0.f : ck * ky);
        o[2] = (cb == 0.f ? 0.f : cb * bz) + (ck == 0.f ? 0.f : ck * kz);
    }
}

// x_denoised[:, centre] backward without atomics: the first token k of every centre atom adds the token gradients of all tokens
// with that atom in token order, then adds the sum to g_x (one thread per (sample, atom) writes)
__global__ __launch_bounds__(256) void centre_grad_scatter(const long long* __restrict__ centre, const float* __restrict__ coef,
                                                          const float* __restrict__ tg, float* __restrict__ g, int B, int A, int T) {
    const int k = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (k >= T || (coef[0] == 0.f && coef[1] == 0.f)) return;
    const long long ck = centre[k];
    for (int j = 0; j < k; ++j)
        if (centre[j] == ck) return;
    const float* t = tg + (long long)b * T * 3;
    float sx = t[3 * k], sy = t[3 * k + 1], sz = t[3 * k + 2];
    for (int j = k + 1; j < T; ++j)
        if (centre[j] == ck) { sx += t[3 * j]; sy += t[3 * j + 1]; sz += t[3 * j + 2]; }
    float* o = g + ((long long)b * A + ck) * 3;
    o[0] += sx; o[1] += sy; o[2] += sz;
}

// ------------------------------------------------------------------ distogram cross entropy (loss.py:78-115)
// coef = scale / (1e-9 + sum_ij m_ij), sum_ij e_i e_j = (sum_i e_i)^2 in float64
__global__ __launch_bounds__(256) void distogram_grad_coef(const float* __restrict__ ex, const long long* __restrict__ pb,
                                                          const float* __restrict__ scale, float* __restrict__ coef, int T) {
    __shared__ double sh[256];
    double s = 0;
    for (int t = threadIdx.x; t < T; t += 256) s += ex[pb[t]];
    s = block_sum_det<256>(s, sh);
    if (threadIdx.x == 0) coef[0] = scale[0] == 0.f ? 0.f : (float)((double)scale[0] / (1e-9 + s * s));
}

// g_p[i][j][k] = coef m^3 (softmax(m p_ij)_k - onehot(bin_ij)_k), m = e_i e_j: the logits of 256 pairs are staged in LDS as in the
// forward, each lane overwrites its own row with the gradient, the block stores it coalesced
__global__ __launch_bounds__(256) void distogram_grad_kernel(const float* __restrict__ logits, const float* __restrict__ xg,
                                                            const float* __restrict__ ex, const long long* __restrict__ pb,
                                                            const float* __restrict__ bound2, const float* __restrict__ coefp,
                                                            float* __restrict__ gp, int T, int nbins) {
    extern __shared__ float sl[];
    const int ld = nbins | 1;
    const long long P = (long long)T * T, p0 = (long long)blockIdx.x * 256;
    const int np = (int)min((long long)256, P - p0);
    const float coef = coefp[0];
    if (coef != 0.f) {
        for (int e = threadIdx.x; e < np * nbins; e += 256) sl[(e / nbins) * ld + e % nbins] = logits[p0 * nbins + e];
        __syncthreads();
        if ((int)threadIdx.x < np) {
            const long long p = p0 + threadIdx.x;
            const int i = (int)(p / T), j = (int)(p % T);
            const long long ai = pb[i], aj = pb[j];
            const float m = ex[ai] * ex[aj];
            const float d2 = dist2_rn(xg[3 * ai] - xg[3 * aj], xg[3 * ai + 1] - xg[3 * aj + 1], xg[3 * ai + 2] - xg[3 * aj + 2]);
            int bin = 0;
            for (int k = 0; k < nbins - 1; ++k) bin += d2 > bound2[k];
            float* l = sl + threadIdx.x * ld;
            float mx = -INFINITY;
            for (int k = 0; k < nbins; ++k) mx = fmaxf(mx, l[k] * m);
            float s = 0.f;
            for (int k = 0; k < nbins; ++k) s += expf(l[k] * m - mx);
            const float f = coef * (m * m * m), inv = 1.f / s;
            for (int k = 0; k < nbins; ++k) l[k] = f * (expf(l[k] * m - mx) * inv - (k == bin ? 1.f : 0.f));
        }
        __syncthreads();
        for (int e = threadIdx.x; e < np * nbins; e += 256) gp[p0 * nbins + e] = sl[(e / nbins) * ld + e % nbins];
    } else {
        for (int e = threadIdx.x; e < np * nbins; e += 256) gp[p0 * nbins + e] = 0.f;
    }
}

// ------------------------------------------------------------------ weighted MSE after alignment (loss.py:118-159)
__global__ __launch_bounds__(256) void weighted_mse_grad_part(const float* __restrict__ xd, const float* __restrict__ al,
                                                             const float* __restrict__ w, float* __restrict__ part, int A) {
    __shared__ float red[4];
    const long long base = (long long)blockIdx.x * A * 3;
    float s = 0.f;
    for (int a = threadIdx.x; a < A; a += 256) {
        const float dx = xd[base + 3 * a] - al[base + 3 * a], dy = xd[base + 3 * a + 1] - al[base + 3 * a + 1],
                    dz = xd[base + 3 * a + 2] - al[base + 3 * a + 2];
        s = fmaf(w[a], fmaf(dz, dz, fmaf(dy, dy, dx * dx)), s);
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// coef = scale * 2 mean_b scale_b(16) / (3 (1e-9 + B sum w)) where the pre-clamp value is <= 1e4 (torch.clamp passes the gradient
// there and nowhere else; a NaN value passes none), 0 elsewhere
__global__ __launch_bounds__(256) void weighted_mse_grad_coef(const float* __restrict__ part, const float* __restrict__ w,
                                                             const float* __restrict__ t_hat, const float* __restrict__ scale,
                                                             float* __restrict__ coef, int B, int A) {
    __shared__ double sh[256];
    double s = 0, n = 0;
    for (int b = threadIdx.x; b < B; b += 256) s += part[b];
    for (int a = threadIdx.x; a < A; a += 256) n += w[a];
    s = block_sum_det<256>(s, sh); n = block_sum_det<256>(n, sh);
    const double sc = mean_edm_scale(t_hat, B, 16.0, sh);
    if (threadIdx.x == 0) {
        const double v = sc * (s / (1e-9 + (double)B * n)) / 3.0;
        coef[0] = (v <= 10000.0 && scale[0] != 0.f) ? (float)((double)scale[0] * 2.0 * sc / (3.0 * (1e-9 + (double)B * n))) : 0.f;
    }
}

__global__ __launch_bounds__(256) void weighted_mse_grad_apply(const float* __restrict__ xd, const float* __restrict__ al,
                                                              const float* __restrict__ w, const float* __restrict__ coefp,
                                                              float* __restrict__ g, int B, int A, int accumulate) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)B * A * 3) return;
    const float coef = coefp[0];
    const float v = coef == 0.f ? 0.f : coef * w[(e / 3) % A] * (xd[e] - al[e]);
    g[e] = accumulate ? g[e] + v : v;
}

inline unsigned elem_blocks(long long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

PD_EXPORT int pd_loss_grad_workspace_numel(int B, int A, int T) {
    if (B < 1 || A < 1 || T < 1) return PD_ERR_ARG;
    long long n = 3LL * B * A + (A + GT - 1) / GT;                            // smooth lDDT: raw [B][A][3] + cnt [nt]
    n = n > 4 + 3LL * B * T ? n : 4 + 3LL * B * T;                            // centre pairs: coef [2] (+2 pad) + token grads [B][T][3]
    n = n > B + 1LL ? n : B + 1LL;                                            // weighted MSE: part [B] + coef
    return n > 0x7fffffffLL ? PD_ERR_UNSUPPORTED : (int)n;                    // distogram: coef [1]
}

PD_EXPORT int pd_loss_smooth_lddt_grad(const float* x_denoised, const float* x_gt, const float* x_exists, float max_clamp_distance,
                                       const float* scale, float* ws, float* g_x, int B, int A, int accumulate, void* stream) {
    if (!x_denoised || !x_gt || !x_exists || !scale || !ws || !g_x || B < 1 || A < 1) return PD_ERR_ARG;
    const int nt = (A + GT - 1) / GT;
    if ((B + GB - 1) / GB > 65535 || 3LL * B * A > 0x7fffffffLL) return PD_ERR_UNSUPPORTED;
    float* cnt = ws + 3LL * B * A;
    hipLaunchKernelGGL(smooth_lddt_grad_kernel, dim3(nt, (B + GB - 1) / GB), dim3(1024), 0, (hipStream_t)stream, x_denoised, x_gt,
                       x_exists, max_clamp_distance, scale, ws, cnt, B, A, nt);
    hipLaunchKernelGGL(smooth_lddt_grad_apply, dim3(elem_blocks(3LL * B * A)), dim3(256), 0, (hipStream_t)stream, ws, cnt, scale, g_x,
                       B, A, nt, accumulate);
    return pd_check_launch();
}

PD_EXPORT int pd_loss_centre_pairs_grad(const float* x_denoised, const float* x_gt, const long long* centre, const float* token_bonds,
                                        const float* is_key_res, const float* is_ligand, const float* t_hat, float sigma_data_bond,
                                        float sigma_data_key, float eps, const float* scale, float* ws, float* g_x, int B, int A, int T,
                                        int accumulate, void* stream) {
    if (!x_denoised || !x_gt || !centre || !token_bonds || !is_key_res || !is_ligand || !t_hat || !scale || !ws || !g_x || B < 1 ||
        A < 1 || T < 1)
        return PD_ERR_ARG;
    if ((B + 3) / 4 > 65535 || B > 65535) return PD_ERR_UNSUPPORTED;
    if (!accumulate && hipMemsetAsync(g_x, 0, sizeof(float) * 3 * (size_t)B * A, (hipStream_t)stream) != hipSuccess) return PD_ERR_LAUNCH;
    float* coef = ws;
    float* tg = ws + 4;
    hipLaunchKernelGGL(centre_grad_coef, dim3(1), dim3(256), 0, (hipStream_t)stream, token_bonds, is_key_res, is_ligand, t_hat,
                       sigma_data_bond, sigma_data_key, eps, scale, coef, B, T);
    hipLaunchKernelGGL(centre_grad_kernel, dim3(T, (B + 3) / 4), dim3(256), 0, (hipStream_t)stream, x_denoised, x_gt, centre, token_bonds,
                       is_key_res, is_ligand, coef, tg, B, A, T);
    hipLaunchKernelGGL(centre_grad_scatter, dim3((T + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, centre, coef, tg, g_x, B, A, T);
    return pd_check_launch();
}

PD_EXPORT int pd_loss_distogram_grad(const float* p_distogram, const float* x_gt, const float* x_exists, const long long* pseudo_beta,
                                     const float* boundaries_sq, int no_bins, const float* scale, float* ws, float* g_p, int A, int T,
                                     void* stream) {
    if (!p_distogram || !x_gt || !x_exists || !pseudo_beta || !boundaries_sq || !scale || !ws || !g_p || A < 1 || T < 1 || no_bins < 2)
        return PD_ERR_ARG;
    if (no_bins > 63) return PD_ERR_UNSUPPORTED;
    const long long nblk = ((long long)T * T + 255) / 256;
    hipLaunchKernelGGL(distogram_grad_coef, dim3(1), dim3(256), 0, (hipStream_t)stream, x_exists, pseudo_beta, scale, ws, T);
    hipLaunchKernelGGL(distogram_grad_kernel, dim3((unsigned)nblk), dim3(256), 256 * (no_bins | 1) * sizeof(float), (hipStream_t)stream,
                       p_distogram, x_gt, x_exists, pseudo_beta, boundaries_sq, ws, g_p, T, no_bins);
    return pd_check_launch();
}

PD_EXPORT int pd_loss_weighted_mse_grad(const float* x_denoised, const float* x_gt_aligned, const float* weights, const float* t_hat,
                                        const float* scale, float* ws, float* g_x, int B, int A, int accumulate, void* stream) {
    if (!x_denoised || !x_gt_aligned || !weights || !t_hat || !scale || !ws || !g_x || B < 1 || A < 1) return PD_ERR_ARG;
    hipLaunchKernelGGL(weighted_mse_grad_part, dim3(B), dim3(256), 0, (hipStream_t)stream, x_denoised, x_gt_aligned, weights, ws, A);
    hipLaunchKernelGGL(weighted_mse_grad_coef, dim3(1), dim3(256), 0, (hipStream_t)stream, ws, weights, t_hat, scale, ws + B, B, A);
    hipLaunchKernelGGL(weighted_mse_grad_apply, dim3(elem_blocks(3LL * B * A)), dim3(256), 0, (hipStream_t)stream, x_denoised,
                       x_gt_aligned, weights, ws + B, g_x, B, A, accumulate);
    return pd_check_launch();
}
