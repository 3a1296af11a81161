// The five terms of the training / validation loss (reference PhysDock/models/loss.py:78-181,245-318,535-559,576-625), forward only.
// The reference materialises [B,A,A], [B,T,T] and [T,T,39] fp32 tensors; here every pair is formed in registers from LDS tiles and
// reduced in the block.  All reductions are two-pass and ordered: a block writes its partial sums to the workspace, a single-block
// second pass adds them in a fixed order in float64, so a call gives the same bits every time (no floating-point atomics).
// Masked entries keep the reference's arithmetic: it MULTIPLIES by the mask, so a non-finite coordinate poisons the sum even where
// the mask is zero (0 * NaN = NaN); the kernels that skip masked pairs add 0 * (x + y + z) of every coordinate they load.
#include "loss_common.h"
#include "physdock_hip.h"

namespace {

constexpr int LT = 64;     // atoms per tile side of the smooth-lDDT kernel (one lane per row atom)
constexpr int LBC = 12;    // samples per block: the ground-truth distances of a tile are computed once per LBC samples
constexpr int LJW = LT / 4;   // column atoms per wave

__device__ __forceinline__ float dist2_rn(float dx, float dy, float dz) {     // (dx^2 + dy^2) + dz^2, no fma contraction
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// 4 * eps(d) = sum_c sigmoid(d - c), c in {0.5, 1, 2, 4}, d >= 0: one exponential e = exp(-d), then 1 / (1 + exp(c) e) per c
__device__ __forceinline__ float lddt_eps4(float d) {
    const float e = __builtin_amdgcn_exp2f(-PD_LOG2E * d);
    return __builtin_amdgcn_rcpf(fmaf(1.6487212707f, e, 1.f)) + __builtin_amdgcn_rcpf(fmaf(2.7182818285f, e, 1.f)) +
           __builtin_amdgcn_rcpf(fmaf(7.3890560989f, e, 1.f)) + __builtin_amdgcn_rcpf(fmaf(54.598150033f, e, 1.f));
}

// ------------------------------------------------------------------ smooth lDDT (loss.py:162-181)
// block = (tile pair p = (ti <= tj), chunk of LBC samples); lane = row atom i, wave w = columns 16 w .. 16 w + 15 of the tile.
// part[p][b] = wgt * sum_{i,j in tile} mask_ij * eps(|d_pred - d_gt|), cnt[p] = wgt * sum mask_ij, wgt = 2 above the diagonal
// (the pair terms are symmetric in i, j).
__global__ __launch_bounds__(256) void smooth_lddt_kernel(const float* __restrict__ xd, const float* __restrict__ xg,
                                                         const float* __restrict__ ex, float clamp, float* __restrict__ part,
                                                         float* __restrict__ cnt, int B, int A, int nt) {
    __shared__ float sxi[LBC][LT * 3], sxj[LBC][LT * 3];
    __shared__ float sgj[LT * 3], sej[LT];
    __shared__ float sred[4][LBC + 1];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int p = blockIdx.x, ti = 0;
    while (p >= nt - ti) { p -= nt - ti; ++ti; }
    const int tj = ti + p;
    const int b0 = blockIdx.y * LBC, nb = min(LBC, B - b0);
    const int i0 = ti * LT, j0 = tj * LT;
    for (int e = tid; e < nb * LT * 3; e += 256) {
        const int bb = e / (LT * 3), r = e % (LT * 3);
        const long long base = (long long)(b0 + bb) * A * 3;
        sxi[bb][r] = (i0 * 3 + r < A * 3) ? xd[base + i0 * 3 + r] : 0.f;
        sxj[bb][r] = (j0 * 3 + r < A * 3) ? xd[base + j0 * 3 + r] : 0.f;
    }
    if (tid < LT * 3) sgj[tid] = (j0 * 3 + tid < A * 3) ? xg[j0 * 3 + tid] : 0.f;
    if (tid < LT) sej[tid] = (j0 + tid < A) ? ex[j0 + tid] : 0.f;
    __syncthreads();
    const int i = i0 + lane;
    const bool in = i < A;
    const float gx = in ? xg[3 * i] : 0.f, gy = in ? xg[3 * i + 1] : 0.f, gz = in ? xg[3 * i + 2] : 0.f, ei = in ? ex[i] : 0.f;
    float dg[LJW], mk[LJW], c = 0.f;
    unsigned act = 0;
#pragma unroll
    for (int jj = 0; jj < LJW; ++jj) {
        const int j = w * LJW + jj;
        dg[jj] = sqrtf(dist2_rn(gx - sgj[3 * j], gy - sgj[3 * j + 1], gz - sgj[3 * j + 2]));
        mk[jj] = (dg[jj] < clamp ? 1.f : 0.f) * ei * sej[j];
        c += mk[jj];
        if (__ballot(mk[jj] != 0.f)) act |= 1u << jj;
    }
    for (int bb = 0; bb < nb; ++bb) {
        const float px = sxi[bb][3 * lane], py = sxi[bb][3 * lane + 1], pz = sxi[bb][3 * lane + 2];
        float acc = 0.f * (px + py + pz);
#pragma unroll
        for (int jj = 0; jj < LJW; ++jj) {
            if (!(act >> jj & 1)) continue;        // wave-uniform
            const int j = w * LJW + jj;
            const float qx = sxj[bb][3 * j], qy = sxj[bb][3 * j + 1], qz = sxj[bb][3 * j + 2];
            const float dx = px - qx, dy = py - qy, dz = pz - qz;
            const float d = __builtin_amdgcn_sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
            acc = fmaf(mk[jj], lddt_eps4(fabsf(d - dg[jj])), acc);
        }
        acc = wave_sum(acc);
        if (lane == 0) sred[w][bb] = acc;
    }
    c = wave_sum(c);
    if (lane == 0) sred[w][LBC] = c;
    __syncthreads();
    const float wgt = ti == tj ? 1.f : 2.f;
    if (tid < nb) part[(long long)blockIdx.x * B + b0 + tid] = wgt * 0.25f * ((sred[0][tid] + sred[1][tid]) + (sred[2][tid] + sred[3][tid]));
    if (tid == 0 && blockIdx.y == 0) cnt[blockIdx.x] = wgt * ((sred[0][LBC] + sred[1][LBC]) + (sred[2][LBC] + sred[3][LBC]));
}

// out = mean_b  sum_p part[p][b] / (1e-9 + sum_p cnt[p]); 16 groups of 64 lanes: lane = sample, group g adds the tile pairs p = g, g + 16, ...
__global__ __launch_bounds__(1024) void smooth_lddt_final(const float* __restrict__ part, const float* __restrict__ cnt,
                                                         float* __restrict__ out, int B, int np) {
    __shared__ double sh[1024];
    const int g = threadIdx.x >> 6, bl = threadIdx.x & 63;
    double n = 0;
    for (int p = threadIdx.x; p < np; p += 1024) n += cnt[p];
    n = block_sum_det<1024>(n, sh);
    double mine = 0;
    for (int b0 = 0; b0 < B; b0 += 64) {
        const int b = b0 + bl;
        double s = 0;
        if (b < B) for (int p = g; p < np; p += 16) s += part[(long long)p * B + b];
        __syncthreads();
        sh[threadIdx.x] = s;
        __syncthreads();
        if (g == 0 && b < B) {
            double tot = 0;
            for (int k = 0; k < 16; ++k) tot += sh[k * 64 + bl];
            mine += tot / (1e-9 + n);
        }
    }
    mine = block_sum_det<1024>(mine, sh);
    if (threadIdx.x == 0) out[0] = (float)(mine / B);
}

// ------------------------------------------------------------------ bond + key-residue terms (loss.py:245-318,535-559)
// one wave per (token i, sample b), lanes over j: part[(i B + b) 2 + {0,1}] = sum_j bonds_ij diff^2, sum_j key_i lig_j eps(|diff|)^2
__global__ __launch_bounds__(256) void centre_pairs_kernel(const float* __restrict__ xd, const float* __restrict__ xg,
                                                          const long long* __restrict__ centre, const float* __restrict__ bonds,
                                                          const float* __restrict__ is_key, const float* __restrict__ is_lig,
                                                          float* __restrict__ part, int B, int A, int T) {
    const int lane = threadIdx.x & 63, b = blockIdx.y * 4 + (threadIdx.x >> 6), i = blockIdx.x;
    if (b >= B) return;                  // whole wave; no block-level synchronisation below
    const float* X = xd + (long long)b * A * 3;
    const long long ci = centre[i];
    const float px = X[3 * ci], py = X[3 * ci + 1], pz = X[3 * ci + 2];
    const float gx = xg[3 * ci], gy = xg[3 * ci + 1], gz = xg[3 * ci + 2];
    const float ki = is_key[i];
    float sb = 0.f, sk = 0.f;
    for (int j = lane; j < T; j += 64) {
        const long long cj = centre[j];
        const float qx = X[3 * cj], qy = X[3 * cj + 1], qz = X[3 * cj + 2];
        const float tb = bonds[(long long)i * T + j], km = ki * is_lig[j];
        const float poison = 0.f * (qx + qy + qz);
        sb += poison; sk += poison;
        if (tb == 0.f && km == 0.f) continue;
        const float dp = sqrtf(dist2_rn(qx - px, qy - py, qz - pz));
        const float dgt = sqrtf(dist2_rn(xg[3 * cj] - gx, xg[3 * cj + 1] - gy, xg[3 * cj + 2] - gz));
        const float diff = dp - dgt;
        sb = fmaf(tb, diff * diff, sb);
        const float e = 0.25f * lddt_eps4(fabsf(diff));
        sk = fmaf(km, e * e, sk);
    }
    sb = wave_sum(sb); sk = wave_sum(sk);
    if (lane == 0) { part[((long long)i * B + b) * 2] = sb; part[((long long)i * B + b) * 2 + 1] = sk; }
}

// out[0] = mean_b scale_b(sd_bond) * mean_b S_b / (sum bonds + eps), out[1] likewise with the key mask and sd_key
__global__ __launch_bounds__(256) void centre_pairs_final(const float* __restrict__ part, const float* __restrict__ bonds,
                                                         const float* __restrict__ is_key, const float* __restrict__ is_lig,
                                                         const float* __restrict__ t_hat, float sd_bond, float sd_key, float eps,
                                                         float* __restrict__ out, int B, int T) {
    __shared__ double sh[256];
    double vb = 0, vk = 0, nb = 0, nk = 0, nl = 0;
    for (long long e = threadIdx.x; e < (long long)T * B; e += 256) { vb += part[2 * e]; vk += part[2 * e + 1]; }
    for (long long e = threadIdx.x; e < (long long)T * T; e += 256) nb += bonds[e];
    for (int t = threadIdx.x; t < T; t += 256) { nk += is_key[t]; nl += is_lig[t]; }
    vb = block_sum_det<256>(vb, sh); vk = block_sum_det<256>(vk, sh);
    nb = block_sum_det<256>(nb, sh); nk = block_sum_det<256>(nk, sh); nl = block_sum_det<256>(nl, sh);
    const double wb = mean_edm_scale(t_hat, B, sd_bond, sh), wk = mean_edm_scale(t_hat, B, sd_key, sh);
    if (threadIdx.x == 0) {
        out[0] = (float)(wb * (vb / B) / (nb + eps));
        out[1] = (float)(wk * (vk / B) / (nk * nl + eps));
    }
}

// ------------------------------------------------------------------ distogram cross entropy (loss.py:78-115)
// 256 token pairs per block; the logits of the block are loaded coalesced into LDS (row stride odd), one lane per pair then
// reads its own row.  part[2 blk] = sum m * err, part[2 blk + 1] = sum m with m = exists_i exists_j.
__global__ __launch_bounds__(256) void distogram_kernel(const float* __restrict__ logits, const float* __restrict__ xg,
                                                       const float* __restrict__ ex, const long long* __restrict__ pb,
                                                       const float* __restrict__ bound2, float* __restrict__ part, int T, int nbins) {
    extern __shared__ float sl[];
    __shared__ float red[4][2];
    const int ld = nbins | 1;
    const long long P = (long long)T * T, p0 = (long long)blockIdx.x * 256;
    const int np = (int)min((long long)256, P - p0);
    for (int e = threadIdx.x; e < np * nbins; e += 256) sl[(e / nbins) * ld + e % nbins] = logits[p0 * nbins + e];
    __syncthreads();
    float se = 0.f, sm = 0.f;
    if ((int)threadIdx.x < np) {
        const long long p = p0 + threadIdx.x;
        const int i = (int)(p / T), j = (int)(p % T);
        const long long ai = pb[i], aj = pb[j];
        const float m = ex[ai] * ex[aj];
        const float d2 = dist2_rn(xg[3 * ai] - xg[3 * aj], xg[3 * ai + 1] - xg[3 * aj + 1], xg[3 * ai + 2] - xg[3 * aj + 2]);
        int bin = 0;
        for (int k = 0; k < nbins - 1; ++k) bin += d2 > bound2[k];
        const float* l = sl + threadIdx.x * ld;
        float mx = -INFINITY;
        for (int k = 0; k < nbins; ++k) mx = fmaxf(mx, l[k] * m);
        float s = 0.f;
        for (int k = 0; k < nbins; ++k) s += expf(l[k] * m - mx);
        const float err = -m * ((l[bin] * m - mx) - logf(s));
        se = m * err; sm = m;
    }
    se = wave_sum(se); sm = wave_sum(sm);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = se; red[threadIdx.x >> 6][1] = sm; }
    __syncthreads();
    if (threadIdx.x < 2) part[2 * (long long)blockIdx.x + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

__global__ __launch_bounds__(256) void distogram_final(const float* __restrict__ part, float* __restrict__ out, int nblk) {
    __shared__ double sh[256];
    double se = 0, sm = 0;
    for (int e = threadIdx.x; e < nblk; e += 256) { se += part[2 * e]; sm += part[2 * e + 1]; }
    se = block_sum_det<256>(se, sh); sm = block_sum_det<256>(sm, sh);
    if (threadIdx.x == 0) out[0] = (float)(se / (1e-9 + sm));
}

// ------------------------------------------------------------------ weighted MSE after alignment (loss.py:118-159)
// part[b] = sum_a w_a |x_denoised - x_gt_aligned|^2
__global__ __launch_bounds__(256) void weighted_mse_kernel(const float* __restrict__ xd, const float* __restrict__ al,
                                                          const float* __restrict__ w, float* __restrict__ part, int A) {
    __shared__ float red[4];
    const long long base = (long long)blockIdx.x * A * 3;
    float s = 0.f;
    for (int a = threadIdx.x; a < A; a += 256) {
        const float dx = xd[base + 3 * a] - al[base + 3 * a], dy = xd[base + 3 * a + 1] - al[base + 3 * a + 1],
                    dz = xd[base + 3 * a + 2] - al[base + 3 * a + 2];
        s = fmaf(w[a], fmaf(dz, dz, fmaf(dy, dy, dx * dx)), s);       // not skipped where w = 0: 0 * NaN stays NaN as in the reference
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// out = min(mean_b scale_b(16) * sum_b part[b] / (1e-9 + B sum w) / 3, 10000); a NaN stays a NaN (torch.clamp)
__global__ __launch_bounds__(256) void weighted_mse_final(const float* __restrict__ part, const float* __restrict__ w,
                                                         const float* __restrict__ t_hat, float* __restrict__ out, int B, int A) {
    __shared__ double sh[256];
    double s = 0, n = 0;
    for (int b = threadIdx.x; b < B; b += 256) s += part[b];
    for (int a = threadIdx.x; a < A; a += 256) n += w[a];
    s = block_sum_det<256>(s, sh); n = block_sum_det<256>(n, sh);
    const double sc = mean_edm_scale(t_hat, B, 16.0, sh);
    if (threadIdx.x == 0) {
        const double v = sc * (s / (1e-9 + (double)B * n)) / 3.0;
        out[0] = v > 10000.0 ? 10000.f : (float)v;
    }
}

inline long long tile_pairs(int A) { const long long nt = (A + LT - 1) / LT; return nt * (nt + 1) / 2; }

}  // namespace

PD_EXPORT int pd_loss_workspace_numel(int B, int A, int T) {
    if (B < 1 || A < 1 || T < 1) return PD_ERR_ARG;
    long long n = tile_pairs(A) * (B + 1);                                  // smooth lDDT: part [np][B] + cnt [np]
    n = n > 2LL * T * B ? n : 2LL * T * B;                                  // centre pairs: [T][B][2]
    const long long nd = 2 * (((long long)T * T + 255) / 256);              // distogram: [blocks][2]
    n = n > nd ? n : nd;
    n = n > B ? n : B;                                                      // weighted MSE: [B]
    return n > 0x7fffffffLL ? PD_ERR_UNSUPPORTED : (int)n;
}

PD_EXPORT int pd_loss_smooth_lddt(const float* x_denoised, const float* x_gt, const float* x_exists, float max_clamp_distance,
                                  float* ws, float* out, int B, int A, void* stream) {
    if (!x_denoised || !x_gt || !x_exists || !ws || !out || B < 1 || A < 1) return PD_ERR_ARG;
    const int nt = (A + LT - 1) / LT;
    const long long np = tile_pairs(A);
    if (np > 0x7fffffffLL || (B + LBC - 1) / LBC > 65535) return PD_ERR_UNSUPPORTED;
    float* cnt = ws + np * B;
    hipLaunchKernelGGL(smooth_lddt_kernel, dim3((unsigned)np, (unsigned)((B + LBC - 1) / LBC)), dim3(256), 0, (hipStream_t)stream,
                       x_denoised, x_gt, x_exists, max_clamp_distance, ws, cnt, B, A, nt);
    hipLaunchKernelGGL(smooth_lddt_final, dim3(1), dim3(1024), 0, (hipStream_t)stream, ws, cnt, out, B, (int)np);
    return pd_check_launch();
}

PD_EXPORT int pd_loss_centre_pairs(const float* x_denoised, const float* x_gt, const long long* centre, const float* token_bonds,
                                   const float* is_key_res, const float* is_ligand, const float* t_hat, float sigma_data_bond,
                                   float sigma_data_key, float eps, float* ws, float* out, int B, int A, int T, void* stream) {
    if (!x_denoised || !x_gt || !centre || !token_bonds || !is_key_res || !is_ligand || !t_hat || !ws || !out || B < 1 || A < 1 || T < 1)
        return PD_ERR_ARG;
    if ((B + 3) / 4 > 65535) return PD_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(centre_pairs_kernel, dim3(T, (B + 3) / 4), dim3(256), 0, (hipStream_t)stream, x_denoised, x_gt, centre,
                       token_bonds, is_key_res, is_ligand, ws, B, A, T);
    hipLaunchKernelGGL(centre_pairs_final, dim3(1), dim3(256), 0, (hipStream_t)stream, ws, token_bonds, is_key_res, is_ligand, t_hat,
                       sigma_data_bond, sigma_data_key, eps, out, B, T);
    return pd_check_launch();
}

PD_EXPORT int pd_loss_distogram(const float* p_distogram, const float* x_gt, const float* x_exists, const long long* pseudo_beta,
                                const float* boundaries_sq, int no_bins, float* ws, float* out, int A, int T, void* stream) {
    if (!p_distogram || !x_gt || !x_exists || !pseudo_beta || !boundaries_sq || !ws || !out || A < 1 || T < 1 || no_bins < 2)
        return PD_ERR_ARG;
    if (no_bins > 63) return PD_ERR_UNSUPPORTED;         // 256 rows of (no_bins | 1) floats fit the default 64 KB of dynamic LDS
    const long long nblk = ((long long)T * T + 255) / 256;
    hipLaunchKernelGGL(distogram_kernel, dim3((unsigned)nblk), dim3(256), 256 * (no_bins | 1) * sizeof(float), (hipStream_t)stream,
                       p_distogram, x_gt, x_exists, pseudo_beta, boundaries_sq, ws, T, no_bins);
    hipLaunchKernelGGL(distogram_final, dim3(1), dim3(256), 0, (hipStream_t)stream, ws, out, (int)nblk);
    return pd_check_launch();
}

PD_EXPORT int pd_loss_weighted_mse(const float* x_denoised, const float* x_gt_aligned, const float* weights, const float* t_hat,
                                   float* ws, float* out, int B, int A, void* stream) {
    if (!x_denoised || !x_gt_aligned || !weights || !t_hat || !ws || !out || B < 1 || A < 1) return PD_ERR_ARG;
    hipLaunchKernelGGL(weighted_mse_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, x_denoised, x_gt_aligned, weights, ws, A);
    hipLaunchKernelGGL(weighted_mse_final, dim3(1), dim3(256), 0, (hipStream_t)stream, ws, weights, t_hat, out, B, A);
    return pd_check_launch();
}
