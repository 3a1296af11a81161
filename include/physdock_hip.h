/* physdock_hip.h - C ABI of libphysdock_hip.so (MI355X / gfx950).
 *
 * The reference (KexinZhangResearch/PhysDock) has no FFI layer: its hot path
 * `PhysDock.sample_diffusion` (PhysDock/models/model.py:157-282) is PyTorch all the way
 * down to ATen.  This header is the boundary this build introduces *below* the Python
 * class `physdock_amd.PhysDock` (which mirrors the reference class, model.py:55-68):
 * every entry point replaces the ATen op sequence named in its comment.
 *
 * Conventions: plain device pointers (fp32 unless noted) and sizes; `stream` is a
 * hipStream_t; return value 0 = ok, negative = error (PD_ERR_*).  No allocation, no
 * synchronisation and no global mutable state inside any launcher, so every call is
 * legal inside hipStreamBeginCapture / EndCapture (hipGraph).
 */
#ifndef PHYSDOCK_HIP_H
#define PHYSDOCK_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PD_ABI_VERSION 11

enum { PD_OUT_ROWMAJOR = 0, PD_OUT_TRANSPOSED = 1, PD_OUT_OPM = 2, PD_OUT_BIASFRAG = 3 };

/* ---- pd_gemm: Y = epilogue(prologue(A) . W^T) ---------------------------------------
 * replaces F.linear (primitives/linear.py:161) together with the norm in front of it
 * (rms_norm.py:14-19, nn.LayerNorm, adaptive_layer_norm_zero.py:18-21), the SwiGLU /
 * sigmoid gates (feed_forward.py:30-31, attentions.py:161-163), the residual add that
 * follows (transformers.py:20-21,49-53,157-158) and the two einsums
 * (attentions.py:164, outer_product_mean.py:28).                                       */
typedef struct pd_gemm_args {
    const float* A;          /* [M,K] row-major (lda) or, if a_kmajor, [K,M] */
    const float* W;          /* [N,K] row-major (ldw) or, if w_kmajor, [K,N] */
    const void* W3;          /* optional: W pre-split into three bf16 parts, fragment-major [3][ceil(N/32)][Kp/16][64][8] with Kp =
                                32*ceil(K/32), zero padded: element (n,k) at lane 32*(k%16/8) + n%32, slot k%8 (packing.split3_bf16)
                                (w = hi + mid + lo exactly).  When given and the problem is one of the full-tile row-major
                                shapes, the contraction runs as six bf16 MFMAs per block with fp32 accumulation
                                (csrc/gemm_split.hip: at least the accuracy of the fp32 MFMA, 2.67x its peak rate); W must
                                still be valid (ragged row remainders and ineligible shapes use it).  NULL: fp32 MFMA.   */
    const void* A3;          /* optional: A already normalised and split into three bf16 parts [3][M][K] (pd_norm_split); K % 32
                                == 0, no prologue fields.  Only the split-operand kernel reads it: a launch that cannot run there
                                (no W3, ragged rows, too few tiles) returns PD_ERR_UNSUPPORTED instead of using the raw A.      */
    float* Y;
    int M, N, K;
    int lda, ldw, ldy;
    int batch;               /* blockIdx.z batches with strides sA/sW/sY (floats) */
    long long sA, sW, sY;
    int a_kmajor, w_kmajor;
    /* prologue on A: a' = act((a - mean[m]) * rstd[m] * pro_w[k] + pro_b[k]); stats = [M][2] */
    const float* stats;
    const float* pro_w;      /* NULL -> 1 */
    const float* pro_b;      /* NULL -> 0 */
    int pro_rows_per_group;  /* >0: pro_w/pro_b row = (m / rows_per_group) * pro_gstride */
    int pro_gstride;
    int pro_act;             /* PD_ACT_* applied to A after the affine (also without stats) */
    /* epilogue, in this order */
    const float* rowscale_acc;   /* [M]  acc *= rowscale_acc[m]                              */
    const float* bias;           /* [N]  (+ batch * sBias)                                   */
    long long sBias;
    const float* hn_w;           /* per-head RMSNorm over each 32-column tile with base < hn_cols:
                                    weight row = (tile_base / hn_split), hn_w = [rows][32]    */
    int hn_cols, hn_split;
    float hn_eps;
    int act;                     /* PD_ACT_*; ignored when glu != 0                          */
    int glu;                     /* 1: silu(a)*b   2: a*sigmoid(b); columns packed per 64 as [a(32) | b(32)] */
    const float* rowscale;       /* [M]  v *= rowscale[m]                                    */
    const float* maskadd;        /* [M]  v += maskval where maskadd[m] == 0                  */
    float maskval;
    const float* mul;            /* gate: v *= mul[m*ldmul + n]  or per row group            */
    int ldmul;
    int mul_rows_per_group;      /* >0: v *= mul[(m / rows_per_group) * mul_gstride + n]     */
    int mul_gstride;
    float out_scale;             /* v *= out_scale (0 -> 1)                                  */
    const float* res;            /* v += res[(m % res_row_mod) * ldres + n] (may alias Y)    */
    int ldres;
    int res_row_mod;
    long long sRes;
    int out_mode;                /* PD_OUT_*                                                 */
    int T1, T2;                  /* OPM: T2 = tokens; BIASFRAG: rows m = (i,j), i<T1, j<T2   */
    int frag_transpose;          /* BIASFRAG: query = j, key = i                             */
    int vecA, vecW, vecY;        /* set by the launcher                                      */
    /* optional K-split scratch (ABI 4): float workspace.  Given it, a launch whose full tiles cannot fill the chip (few
       samples) is cut along K into `ksplit` parts per tile: a first launch stores every part's partial accumulators here, a
       second one adds them IN FIXED ORDER (bit-reproducible, no floating-point atomics) and runs the epilogue.  NULL: never.  */
    void* ksplit_ws;
    long long ksplit_ws_bytes;
    int ksplit;                  /* set by the launcher                                      */
    /* ABI 5: two-part fp16 operand format (csrc/gemm_f16.hip: three fp16 MFMAs per block instead of six bf16 ones).  Used when
       all of W2, w_inv and a_amax are given and the launch is a chip-filling full-tile row-major problem; otherwise the launch
       falls through to W3 / fp32 as before.  The caller guarantees |A'[m,k]| <= *a_amax for the A the contraction sees (after
       the prologue): a larger element overflows fp16.  pd_dit_bounds derives such bounds for the DiT blocks.                  */
    const void* W2;              /* W[n,:] * w_scale[n] as two fp16 parts (hi, lo), fragment-major [2][ceil(N/32)][Kp/16][64][8]
                                    (packing.split2_f16); w_scale[n] = power of two that brings max_k |W[n,k]| into [2^14, 2^15)      */
    const float* w_inv;          /* [N]  1 / w_scale[n]                                                                        */
    const void* A2;              /* optional: A already normalised, modulated, scaled by the power of two pd_gemm derives from
                                    *a_amax, and split into two fp16 parts [2][M][K] (pd_norm_split2); K % 32 == 0, no prologue  */
    const float* a_amax;         /* device scalar: upper bound of |A'|                                                         */
    /* ABI 6, head-norm epilogue of the fp16-format kernel only (the q|k|v projection of a DiT block): output columns
       n >= y2_col0 (k and v) are NOT stored to Y but written ALREADY SCALED AND SPLIT for the attention kernel
       (pd_attn_args.K2 / V2) into Y2, fp16 elements, row stride ldy2 = 2 * (N - y2_col0): inside a row every group of four
       columns c = n - y2_col0 = 4 g + e occupies eight consecutive elements - the four high parts at 8 g + e, the four low
       parts at 8 g + 4 + e - so that one 16-byte load yields both parts of four values.  A value is multiplied by the power
       of two pd_attention derives from the bound y2_amax[c / hn_split] (device floats: max|k|, max|v|) before it is split.
       Any launch that cannot honour Y2 fails with PD_ERR_UNSUPPORTED - it is never silently ignored.                      */
    void* Y2;
    const float* y2_amax;
    int y2_col0, ldy2;
    /* ABI 7: row statistics computed INSIDE the consuming kernel: stats == NULL and stats_inline = 1 (RMSNorm) or 2 (LayerNorm,
       two passes: mean, then centred squares - the arithmetic of pd_rowstats) with stats_eps; pro_w / pro_b / groups as with
       stats.  Two kernels do this: the fp32 streaming kernel (csrc/gemm_stream.hip: launches too small to fill the chip - few
       samples, the trunk's single / MSA tracks): a block re-reads its rows (K floats each, L2-resident) before its main loop,
       which saves the separate pd_rowstats launch - latency, not bytes; and the fp16-format ROWS kernel (csrc/gemm_f16.hip,
       gemm_f16_rows_kernel: K == 128, W2 / w_inv / a_amax given, whole 64- / 128-row tiles, plain or head-norm epilogue): a
       block keeps its rows, normalised and split once, in LDS for every column tile - one pass over A instead of one per
       column tile plus the statistics pass.  Anything else answers PD_ERR_UNSUPPORTED.                                     */
    int stats_inline;
    float stats_eps;
} pd_gemm_args;
int pd_gemm(const pd_gemm_args* args, void* stream);
/* id of the kernel instantiation pd_gemm would launch for these arguments (for profiling);
 * id % 10000 >= 5000: gemm_stream_kernel<id % 10, (id / 10000) % 10, Tile> (csrc/gemm_stream.hip) takes it,
 * Tile = (id / 100000) % 10: 0 -> <128,128,2>, 1 -> <64,64,2>, 2 -> <128,64,4>; id >= 1000000: the split-operand
 * kernel gemm_split_kernel<...> (csrc/gemm_split.hip) with the same template arguments; id >= 2000000: gemm_f16_kernel<...>
 * (csrc/gemm_f16.hip, two-part fp16 operands; tile field (id % 1000000) / 100000 = 3 / 4: gemm_f16_rows_kernel<pro, EPI, 128 / 64>) */
int pd_gemm_variant(const pd_gemm_args* args);

/* ---- pd_rowstats: per-row (mean, rstd) for the GEMM prologue --------------------------
 * mode 0: RMS  -> (0, rsqrt(mean(x^2)+eps));  mode 1: LayerNorm -> (mean, rsqrt(var+eps)).
 * x is [M,C] (ldx) or, if kmajor, [C,M] (ldx = M stride).                               */
int pd_rowstats(const float* x, float* stats, int M, int C, int ldx, int kmajor, int mode, float eps, void* stream);

/* ---- pd_rownorm: y = [res +] act(norm(x) * w + b) (standalone normalisation)            */
int pd_rownorm(const float* x, float* y, const float* res, const float* w, const float* b,
               int M, int C, int mode, float eps, int act, void* stream);

/* ---- pd_norm_split: rows normalised, modulated and split for pd_gemm_args.A3 -----------------
 * out3 [3][M][C] bf16 (hi, mid, lo: a' = hi + mid + lo exactly) of a'[m,k] = (x[m,k] - mean_m) rstd_m w[g][k] + b[g][k],
 * g = m / rows_per_group (0: one row of w / b for all; NULL w / b: 1 / 0) - the expression of pd_gemm's norm prologue
 * (rms_norm.py:14-19, adaptive_layer_norm_zero.py:16-21) evaluated ONCE per element instead of once per column block of
 * the GEMM that consumes it.  C % 32 == 0.                                                                            */
int pd_norm_split(const float* x, int ldx, int M, int C, int mode, float eps, const float* w, const float* b,
                  int rows_per_group, int gstride, void* out3, void* stream);
/* pd_norm_split2 (ABI 5): the same rows times the power of two derived from the device scalar *a_amax (an upper bound of |a'|),
 * as TWO fp16 parts out2 [2][M][C] (hi, lo) - the pre-split A operand pd_gemm_args.A2 of csrc/gemm_f16.hip.                    */
int pd_norm_split2(const float* x, int ldx, int M, int C, int mode, float eps, const float* w, const float* b,
                   int rows_per_group, int gstride, const float* a_amax, void* out2, void* stream);

/* ---- pd_transition_f16 (ABI 5): the atom-level DiT transition in one launch --------------------------------------------------
 * x[m,:] += gate[g] * W2 . ( silu(W1 y) * (W3 y) ),  y = scale1p[g] * LayerNorm(x[m,:]) + shift[g],  g = m / rows_per_group
 * (transitions.py:27-30 with adaptive_layer_norm_zero.py:16-21 and feed_forward.py:30-31): row statistics, SwiGLU projection
 * and down-projection of 64 whole rows per block, the hidden activations stay in LDS.  C = 128 and hidden = 384 only, M % 64
 * == 0 and M >= 2048 (PD_ERR_UNSUPPORTED otherwise: run pd_rowstats + two pd_gemm).  W13 / W2 are the two-part fp16
 * fragment-major forms of the packed [a(32) | b(32)] SwiGLU weights [2 hidden][C] and of W2 [C][hidden] with their inverse row
 * scales (packing.split2_f16); y_amax / h_amax are device scalars bounding |y| and |silu(a) b| (pd_dit_bounds).
 * args == NULL: one-time set-up (dynamic LDS limit), called by pd_init.                                                        */
typedef struct pd_transition_args {
    float* x;                    /* [M][C], updated in place */
    int M, C, hidden;
    const float* shift; const float* scale1p; const float* gate;      /* [C] each (+ g * gstride)                      */
    int rows_per_group, gstride; /* 0: one row of shift / scale / gate for all rows                                        */
    float eps;
    const void* W13; const float* w13_inv; const void* W2; const float* w2_inv;
    const float* y_amax; const float* h_amax;
    int rms;                     /* ABI 7: 1 = RMSNorm instead of LayerNorm (no mean subtraction): with shift = zeros, scale1p = the norm
                                    gain and gate = ones this is the trunk's pair Transition (transitions.py:15-18) on [T*T][128] rows  */
} pd_transition_args;
int pd_transition_f16(const pd_transition_args* args, void* stream);

/* ---- pd_tri_tail (ABI 7): the tail of the trunk's TriangleUpdate in one launch ------------------------------------------------
 * z[m,:] += sigmoid(W_g RMSNorm(z[m,:]) w_in + b_g) * (W_z RMSNorm(o[:,m]) w_out + b_z)     (attentions.py:163,170-171)
 * for the channel-major einsum output o [Co][M] (attentions.py:164): replaces the gate projection, the column statistics of o and
 * the K = Co projection with gate + residual (three launches, a 33 MB gate tensor) - HBM sees z in, o in, z out.  C = 128 and
 * Co = 32 only (PD_ERR_UNSUPPORTED otherwise).  W_g [C][C] / W_z [C][Co] in the two-part fp16 fragment-major form with inverse
 * row scales (packing.split2_f16); zn_amax / on_amax: device scalars bounding the normalised rows times their gains
 * (sqrt(C) max|w_in|, sqrt(Co) max|w_out|).  args == NULL: one-time set-up, called by pd_init.                               */
typedef struct pd_tri_tail_args {
    float* z;                    /* [M][C], updated in place */
    const float* o;              /* [Co][M] */
    int M, C, Co;
    const float* w_in; const float* w_out;       /* norm gains [C], [Co] */
    float eps;
    const void* Wg; const float* wg_inv; const float* bg;
    const void* Wz; const float* wz_inv; const float* bz;
    const float* zn_amax; const float* on_amax;
    int mode;                    /* 0: TriangleUpdate tail as above.  1: TriangleAttention tail (attentions.py:204,212-213):
                                    z[m,:] += (W_g RMSNorm(z[m,:]) w_in + b_g) * (W_z o[m,:] + b_z) with the attention output o [M][C]
                                    (row-major, Co = C, |o| <= *on_amax = the v bound), a RAW gate, w_out unused              */
} pd_tri_tail_args;
int pd_tri_tail(const pd_tri_tail_args* args, void* stream);

/* ---- pd_tri_attention (ABI 9): TriangleAttention up to the attention output with the q | k | v projection INSIDE the attention
 * block (reference primitives/attentions.py:194-211; csrc/tri_attn.hip).  Replaces, per instance, pd_gemm (RMSNorm prologue, q | k | v)
 * + pd_attention:  o[b, r, 32 h + d] = sum_k softmax_k( q[b,r,h,:] . k[b,k,h,:] / sqrt(32) + bias[h, r, k] ) v[b,k,h,d]  with
 * q | k | v = (z[b, r, :] / rms(z[b, r, :])) . Wf^T, Wf = the [3 C][C] projection with the norm gain folded in (Wf[n][c] = W[n][c] w[c]).
 * z2: the normalised rows, scaled, split into two fp16 parts and in fragment order, as pd_pair_bias_split writes them (same zn_amax,
 * same transpose flag); o: [T][T][C] in the pair tensor's own layout - transpose == 0: batch b = first index, sequence r = second;
 * 1: the other way round (the column variant - nothing is transposed in memory).  W2 / w_inv = packing.split2_f16(Wf, rows_per_scale =
 * 32) (two fp16 parts, fragment-major, ONE power-of-two scale per 32-row tile; w_inv[n] = its inverse); bias: fragment layout for
 * (nq = T, nk = bias_nk) ALREADY multiplied by bias_prescale = the power of two pd_attention_bias_prescale_log2 derives from
 * qkv_amax[0..1]; qkv_amax: device floats [3] bounding |q|, |k|, |v|; zn_amax: host float bounding |z / rms| (sqrt(C));
 * Treal: real key count (keys >= Treal are masked).  C = 128, nheads = 4, T <= 256, T % 4 == 0; else PD_ERR_UNSUPPORTED.        */
typedef struct pd_tri_attn_args {
    const void* z2;
    const void* W2; const float* w_inv;
    const float* bias; float bias_prescale; int bias_nk;
    float* o;
    int T, Treal, C, nheads, transpose;
    float zn_amax; const float* qkv_amax;
    float scale;                 /* 1 / sqrt(32) */
} pd_tri_attn_args;
int pd_tri_attention(const pd_tri_attn_args* args, void* stream);
int pd_tri_attn_args_size(void);

/* ---- pd_tri_mul (ABI 7): the triangle-multiplication einsum (attentions.py:164) on the two-part fp16 format ----------------------
 * transpose == 0:  o[c,i,I] = sum_{j < Treal} q[c,i,j] k[c,I,j];   transpose == 1:  o[c,a,b] = sum_{j < Treal} k[c,j,a] q[c,j,b]
 * for nch channel planes [T][T] (plane stride ch_stride floats) of q, k, o; q_amax / k_amax: device scalars bounding |q|, |k|
 * (the gated projection's linear part: ||W_n w||_2 sqrt(C) + |b_n|).  T % 4 == 0.                                              */
typedef struct pd_tri_mul_args {
    const float* q; const float* k; float* o;
    int T, Treal, nch;
    long long ch_stride;
    int transpose;
    const float* q_amax; const float* k_amax;
} pd_tri_mul_args;
int pd_tri_mul(const pd_tri_mul_args* args, void* stream);

/* ---- pd_pair_bias: attention pair bias in one streaming pass (pairbias.hip) -------------------
 * frag = fragment layout of [ (norm(x) . Wf^T + c2 + maskadd ? 0 : maskval) * out_scale ] for x [T1*T2, C] (C = 16 or 128),
 * Wf [H][C] = projection weights with the norm gain folded in (Wf[h][k] = w[k] W[h][k]), c2 [H] = projection of the norm
 * shift (NULL: 0), H in {4, 8, 16} for C = 128 and {4, 24} for C = 16; mode 0 RMS / 1 LayerNorm.  Replaces linear_z(norm_z(z))
 * of attentions.py:38-41,82-85,200-203,246,254 (= pd_rowstats + pd_gemm PD_OUT_BIASFRAG) with one read of x; stats_out
 * (optional, [T1*T2][2]) receives the (mean, rstd) pairs for the projection GEMM that follows.  T2 % 4 == 0.              */
int pd_pair_bias(const float* x, const float* Wf, const float* c2, float* stats_out, const float* maskadd, float maskval,
                 float out_scale, float* frag, int T1, int T2, int C, int H, int frag_transpose, int mode, float eps,
                 void* stream);
/* pd_pair_bias_split (ABI 9): pd_pair_bias for the TriangleAttention (x [T*T][128], H = 4, RMS) that ALSO writes x / rms(x) times the
 * power-of-two operand scale of zn_amax (= sqrt(C) 1.0001), split into two fp16 parts, in pd_tri_attention's fragment order:
 * z2 [T batches][ceil(T/32) row tiles][8 k-steps][2 parts][64 lanes][8] halves (batch / row = the pair indices, swapped when
 * frag_transpose).  Rows beyond T of the last tile are not written: zero the buffer once.                                         */
int pd_pair_bias_split(const float* x, const float* Wf, const float* c2, float* stats_out, const float* maskadd, float maskval,
                       float out_scale, float* frag, int T, int frag_transpose, float eps, void* z2, float zn_amax, void* stream);

/* ---- pd_attention: O = softmax(Q K^T * scale + bias) V, head width 32 ------------------
 * replaces F.scaled_dot_product_attention at attentions.py:48,92,130,211,259.
 * Q/K/V/O element (b, i, h, d) at ptr[b*bs + i*ss + h*32 + d].  bias is in the fragment
 * layout [H][ceil(nq/32)][ceil(nk/32)][4][64][4] and already multiplied by log2(e)
 * (written by pd_gemm PD_OUT_BIASFRAG); NULL = no bias.  bias is shared by all batches. */
typedef struct pd_attn_args {
    const float* Q; const float* K; const float* V; float* O;
    int nq, nk, nbatch, nheads;
    long long q_bs, q_ss, k_bs, k_ss, v_bs, v_ss, o_bs, o_ss;
    const float* bias;
    float scale;             /* 1/sqrt(32) */
    int bias_nk;             /* key count the bias buffer was laid out for (pd_gemm PD_OUT_BIASFRAG's T2, i.e. the PADDED
                                count when nk is the real one); 0 -> nk                                                  */
    int fp32_mfma;           /* 1: keep both contractions on v_mfma_f32_32x32x2_f32 (csrc/attention.hip); 0 (default): launches
                                that fill the chip run on the bf16 matrix pipe with 3-way split operands at fp32 accuracy
                                (csrc/attn_split.hip)                                                                      */
    float* ws;               /* optional scratch (16-byte aligned) for key-split launches, see below; may be NULL       */
    long long ws_bytes;
    int nsplit;              /* set by the launcher                                                                      */
    /* ABI 5: two-part fp16 operand format for the split-operand kernel (csrc/attn_split.hip, NP = 2): q, k, v are multiplied by
       powers of two derived from UPPER BOUNDS of their magnitudes and split into (hi, lo) fp16 parts; three partial products per
       block instead of six.  The bounds must hold (a larger element overflows fp16): either by value, or in device memory
       (f16_amax[0..2] = max|q|, max|k|, max|v|, read by the kernel - graph-capturable, no host round trip).                   */
    int f16x3;               /* 1: use the fp16 format (needs the bounds below); 0: bf16 x 6 (any fp32 input)              */
    float f16_q_amax, f16_k_amax, f16_v_amax;
    const float* f16_amax;   /* optional device array [3]; overrides the by-value bounds                                  */
    void* O2;                /* optional, f16x3 launches only: instead of O, write the output ALREADY SPLIT for the projection that
                                follows - two fp16 parts [2][nbatch*nq][nheads*32] of o times the power of two derived from the v
                                bound (|o| <= max|v|), i.e. pd_gemm_args.A2 with a_amax = &f16_amax[2]; rows are (batch, query)
                                in order, so it needs o_bs = nq * o_ss and o_ss = nheads * 32.  16-byte aligned.              */
    /* ABI 6, f16x3 launches only: K and V already scaled (by the powers of two this kernel derives from f16_amax[1] /
       f16_amax[2]) and split into two fp16 parts by the producing projection (pd_gemm_args.Y2 layout): the high parts of dims
       4 g .. 4 g + 3 of (b, key, h) at K2[b * kv2_bs + key * kv2_ss + 64 h + 8 g ..], the low parts four elements further
       (fp16 elements; 16-byte aligned).  The staging of a key tile is then a copy - every query block of a (batch, head) no
       longer re-splits the same K and V.  K / V (fp32) are ignored when K2 / V2 are given; both or neither.               */
    const void* K2;
    const void* V2;
    long long kv2_bs, kv2_ss;
    /* ABI 7, f16x3 launches only: > 0 = the bias fragments were produced ALREADY MULTIPLIED by this power of two - the product of
       the q and k operand scales the kernel derives from f16_amax[0..1] (pd_attention_bias_prescale_log2 computes its exponent
       from the same bounds on the host; the producer folds it into out_scale).  The pipelined kernel (csrc/attn_pipe.hip) then
       takes the bias tile as the INITIAL VALUE of the score accumulator - no bias add.  0 with a bias: the launch stays on
       attn_parts_kernel (csrc/attn_f16.hip), which adds an unscaled bias; < 0: keep the launch on attn_parts_kernel (A/B runs).   */
    float bias_prescale;
    /* ABI 8: rows of one part plane of O2 when the launch covers only a slice of the samples that share the O2 buffer (the low parts
       sit o2_rows * nheads * 32 elements behind the high parts); 0: nbatch * nq.                                                      */
    long long o2_rows;
    /* ABI 10: several systems in one launch (PhysDock.sample_diffusion_many).  Consecutive runs of group_samples batches share one
       bias set: batch b reads the fragments at bias + (b / group_samples) * bias_gstride floats, all laid out for the same bias_nk
       (the padded key count).  nk_group (device int[G], or NULL = nk for every group) holds each group's real key count; nk is
       the launch's bound (every group count is clamped to [1, nk]) and what the launcher picks its kernel by.  group_samples = 0:
       every batch shares group 0 (the behaviour before ABI 10).  Every kernel family honours the fields.                          */
    int group_samples;
    long long bias_gstride;
    const int* nk_group;
} pd_attn_args;
/* Launches that cannot fill the chip (nbatch * nheads * ceil(nq/128) < 512 blocks) with a long key range are split into
 * up to 8 key chunks when ws holds nsplit * nbatch * nq * nheads * 34 floats; a second kernel merges the chunks. */
int pd_attention(const pd_attn_args* args, void* stream);
/* waves per block (4 or 8 = template argument of attn_kernel) pd_attention picks for these arguments; 4 + 100 * nsplit for
 * a key-split launch; 1000 + waves for attn_split_kernel<waves>, 2000 + waves for attn_parts_kernel<waves, 2>, 2000 + 4 +
 * 100 * nsplit for a key-split launch on attn_parts_kernel<4, 2, false, true> (profiling) */
int pd_attention_variant(const pd_attn_args* args);
/* log2 of the power of two a bias producer folds into out_scale for f16x3 launches with bias_prescale (ABI 7): the q and k operand
 * scales of the fp16 format for these bounds (scale = 1/sqrt(32)); host arithmetic identical to the kernel's.  3000 + waves =
 * attn_pipe_kernel<waves, ., .> in pd_attention_variant's numbering.                                                        */
int pd_attention_bias_prescale_log2(float q_amax, float k_amax, float scale);

/* ---- pair-representation / pooling kernels (pair.hip) ----------------------------------
 * pd_atom_pair_init : ap = cl_l + cm_m + v*(Wp.d + Wd/(1+|d|) + Wv)   (diffusion_conditioning.py:116-124)
 * pd_pair_gather_add: ap[l,m] += zt[a2t[l], a2t[m]]                    (diffusion_conditioning.py:237)
 * pd_pair_init_z    : z = s_i + s_j + RelPos + bonds                   (diffusion_conditioning.py:65-94,187-189)
 * pd_segment_pool   : token mean of contiguous atom rows (/(n+1e-3))   (transformers.py:205-212)
 * pd_unpool_add     : ba[b,l] += us[b, a2t[l]]                         (transformers.py:214-216)
 * pd_gather_rows_add: y[r] += x[idx[r]]                                (diffusion_conditioning.py:236)
 * pd_axpby          : out = a*sa + b*(sb_ptr ? sb_ptr[0]*sb : sb)
 * pd_template_mask  : z_mask * templ_feat[...,D-1] * same_chain        (diffusion_conditioning.py:41-42)
 * Index tensors keep the loader's dtypes: int64 (uid, a2t, residue_index) / int32 (asym, sym, entity). */
/* pd_atom_pair_ffn  : ap += W2 . (silu(W1 ap) * (W3 ap)) in one pass, c_ap = 16 / hidden = 128 only (other shapes:
 *                      PD_ERR_UNSUPPORTED, use two pd_gemm)         (diffusion_conditioning.py:125-126, feed_forward.py:26-31) */
int pd_atom_pair_ffn(float* ap, const float* W1, const float* W3, const float* W2, long long rows, int c_ap, int hidden,
                     void* stream);
int pd_atom_pair_init(const float* pos, const long long* uid, const float* cl, const float* cm, const float* Wp,
                      const float* Wd, const float* Wv, float* ap, int A, int c_ap, void* stream);
int pd_pair_gather_add(float* ap, const float* zt, const long long* a2t, int A, int T, int c_ap, void* stream);
int pd_pair_init_z(const float* si, const float* sj, const float* WT, const float* wb, const int* asym, const int* sym,
                   const int* ent, const long long* res, const float* rel_tok_feat, const float* bonds, float* z, int T,
                   int CZ, void* stream);
int pd_segment_pool(const float* u, const int* tok_start, const float* add, float* out, int B, int A, int T, int C,
                    void* stream);
int pd_unpool_add(float* ba, const float* us, const long long* a2t, int B, int A, int T, int C, void* stream);
/* ABI 10, G systems of B samples each in one launch (PhysDock.sample_diffusion_many): sample g B + b of the [G B] rows belongs to
 * system g and reads that system's own table - tok_start [G][T + 1], add [G][T][C] (or NULL), a2t [G][A].  At G = 1 each is
 * bit-identical to its single-system counterpart.                                                                               */
int pd_segment_pool_g(const float* u, const int* tok_start, const float* add, float* out, int G, int B, int A, int T, int C,
                      void* stream);
int pd_unpool_add_g(float* ba, const float* us, const long long* a2t, int G, int B, int A, int T, int C, void* stream);
/* pd_downscale_pool (ABI 8): linear_downscale + SiLU + token mean pooling + s of the denoiser in one launch (reference
 * layers/transformers.py:205-212; csrc/pool.hip): out[b,t,:] = sum_{atoms l of t} silu(W ba[b,l,:] + bias) / (n_t + 1e-3) + add[t,:].
 * ba [B][A][128]; W2 / w_inv = the two fp16 parts of W [N][128] (fragment-major) and its inverse row scales (packing.split2_f16) -
 * the A operand's power-of-two scale is the block's own: the maximum of the tile it stages; tok_start [T + 1]; tpb tokens per block
 * (1..32) with the caller's guarantee that tpb consecutive tokens hold at most 64 atoms (the table is device memory: a block that
 * finds more writes NaN into its tokens' rows instead of a wrong mean).  PD_ERR_UNSUPPORTED: other shapes.                         */
int pd_downscale_pool(const float* ba, const void* W2, const float* w_inv, const float* bias, const int* tok_start, const float* add,
                      float* out, int B, int A, int T, int Cin, int N, int tpb, void* stream);
/* ABI 10: the same for G systems of B samples (tok_start [G][T + 1], add [G][T][N]); tpb must hold for every system of the group */
int pd_downscale_pool_g(const float* ba, const void* W2, const float* w_inv, const float* bias, const int* tok_start, const float* add,
                        float* out, int G, int B, int A, int T, int Cin, int N, int tpb, void* stream);
int pd_gather_rows_add(float* y, const float* x, const long long* idx, int R, int C, void* stream);
int pd_axpby(float* out, const float* a, float sa, const float* b, const float* sb_ptr, float sb, long long n, void* stream);
/* pd_template_feat  : templ_feat [T,T,no_bins+1] = [distogram bins of the pseudo-beta distance | mask] * mask, mask = z_mask *
 *                      protein_i * protein_j (feature_loader.py:944-968 inference branch; tensor_utils.py:689-703); lower =
 *                      the no_bins fp32 bin edges linspace(3.25, 50.75, no_bins)^2 computed by the host (slice) */
int pd_template_feat(const float* x, const long long* pseudo_beta_atom, const float* z_mask, const float* is_protein,
                     const float* lower, float* out, int T, int no_bins, void* stream);
int pd_template_mask(const float* z_mask, const float* templ_feat, const int* asym, float* out, int T, int D, void* stream);
/* ConfidenceModule entry / exit passes (confidence.hip; reference models/layers/confidence_module.py:56-88):
 * pd_confidence_pair_init: out[i,j,:] = z[i,j,:] + si[i,:] + sj[j,:] + WdT[bin(|xc_i - xc_j|), :], xc = x[centre[.]], bin =
 *                          nearest of linspace(3.375, 24.375, 13) (first on ties), WdT = linear_d.weight^T [13][C]   (:68-72)
 * pd_pair_symmetrize     : out[i,j,:] = z[i,j,:] + z[j,i,:] (out != z)                                             (:75)
 * pd_atom_dist_embed     : ap[i,j,:] = |x_i - x_j| w + b, Linear(1, c_ap)                                           (:80)     */
int pd_confidence_pair_init(const float* z, const float* si, const float* sj, const float* WdT, const float* x,
                            const long long* centre, float* out, int T, int C, void* stream);
int pd_pair_symmetrize(const float* z, float* out, int T, int C, void* stream);
int pd_atom_dist_embed(const float* x, const float* w, const float* b, float* ap, int A, int C, void* stream);
/* The same passes for a chunk of P poses per launch (additive exports of ABI 11; Engine.confidence_poses).  x holds the poses
 * x_stride floats apart; outputs are pose-major ([P][T*T][C] / [P][A*A][C]).  Every pose's slice is bit-identical to the
 * single-pose launcher's output: same thread map, same order of operations.
 * pd_confidence_pair_init_poses: z, si and sj are read ONCE per launch; per pose only the row of WdT changes
 * pd_pair_symmetrize_poses     : z, out [P][T*T][C] (out != z)
 * pd_atom_dist_embed_poses     : ap [P][A*A][C]                                                                             */
int pd_confidence_pair_init_poses(const float* z, const float* si, const float* sj, const float* WdT, const float* x,
                                  const long long* centre, float* out, int T, int C, int P, long long x_stride, void* stream);
int pd_pair_symmetrize_poses(const float* z, float* out, int T, int C, int P, void* stream);
int pd_atom_dist_embed_poses(const float* x, const float* w, const float* b, float* ap, int A, int C, int P, long long x_stride,
                             void* stream);

/* ---- feature tensorisation + PDB writer (features.hip) ------------------------
 * The steps either side of the sampler: FeatureLoader.transform (feature_loader.py:970-998) and
 * FeatureLoader.write_pdb_block (:1230-1283).  Raw per-system arrays in, model feature tensors out; poses in, PDB bytes out.
 * pd_target_feat    : [one_hot(restype, n_class) | profile | deletion_mean] -> [T, n_class + n_profile + 1]      (:805-809)
 * pd_msa_feat       : rows inds[] of (msa, deletion_matrix) -> [n_rows_out, T, n_class + 2] =
 *                     [one_hot | clamp(del,0,1) | atan(del/3) * two_over_pi]; two_over_pi = the host's fp32 2/(2 acos 0) (:813-826)
 * pd_outer_mask     : out[i,j] = m[i] m[j]  (z_mask, ap_mask)                                                     (:982-983)
 * pd_chain_contacts : per chain pair p = (pairs[2p], pairs[2p+1]) (atoms chain_start[c] .. chain_start[c+1]): closest atom pair
 *                     under |xa-xb| + (1 - mask_a mask_b) 1000, first in (a,b) order on ties; below `threshold` the two atoms'
 *                     tokens are set to 1 in between[T,T] (symmetric; caller zeroes it); min_out / arg_out [n_pairs] optional  (:882-900)
 * pd_pdb_format     : out[b, n, 0:81] = tmpl[n, 0:81] with columns 31-54 replaced by x[b, atom[n], 0:3] as "%8.3f" (Python
 *                     float formatting of the fp32 value, ties to even, "-0.000" kept); *overflow counts values that do not fit
 *                     the field (printed as '*')                                                                  (:1259-1270) */
int pd_target_feat(const long long* restype, const float* profile, const float* deletion_mean, float* out, int T, int n_class,
                   int n_profile, void* stream);
int pd_msa_feat(const long long* msa, const float* deletion_matrix, const long long* inds, float two_over_pi, float* out,
                int n_rows_out, int T, int n_class, void* stream);
int pd_outer_mask(const float* m, float* out, int N, void* stream);
int pd_chain_contacts(const float* x, const float* a_mask, const int* chain_start, const int* pairs, int n_pairs,
                      const long long* a2t, float threshold, float* between, int T, float* min_out, long long* arg_out,
                      void* stream);
int pd_pdb_format(const float* x, const unsigned char* tmpl, const int* atom, unsigned char* out, int* overflow, int B, int A,
                  int N, void* stream);

/* ---- per-step sampler kernels (sampler.hip) ------------------------------------------------
 * pd_augment       : centre_random_augmentation + noise injection      (tensor_utils.py:576-586, model.py:70-85)
 *                    parity mode: rot_u[4][B], trans[B][3], noise[B][A][3]; perf mode: Philox(seed, sample0+b, step)
 * pd_init_noise    : x0 = sigma_0 * N(0,1) from Philox                  (model.py:148)
 * pd_precond       : ba = Wx.(x_hat*c_in) + bx + a                      (transformers.py:218-223)
 * pd_denoise       : x_den = c_skip*x_hat + c_out*Wr.LN(ba)             (transformers.py:228-233)
 * pd_kabsch_align  : weighted_rigid_align (moves x_gt onto x_pred)      (tensor_utils.py:724-778)
 * pd_template_match: eps metric, argmin, write template into ref_pos   (model.py:231-241; redocking.py:326-335);
 *                    with eps_out [B][Cn] given the metric runs one workgroup per (conformer, sample), same values
 * pd_pose_dist     : pairwise distances of conformers                   (model.py:186)
 * pd_euler         : d_cur mix + Euler step                             (model.py:245-281)
 * pd_timestep_embed: sinusoidal embedding                               (timestep_embeddings.py:64-81)   */
int pd_augment(const float* x, float x_scale, const float* mask, const float* rot_u, const float* trans,
               const float* noise, float lambda, float sdev, const unsigned long long* seed, int step, int sample0,
               float* out, int B, int A, void* stream);
int pd_init_noise(float* x, const unsigned long long* seed, int sample0, float sigma0, int B, int A, void* stream);
int pd_precond(const float* x_hat, float c_in, const float* c_in_b, const float* Wx, const float* bx, const float* a,
               float* ba, int B, int A, int C, void* stream);
/* ABI 10: G systems of B samples, a [G][A][C] (system g's samples read a[g]); c_in_b, if given, [G B]                        */
int pd_precond_g(const float* x_hat, float c_in, const float* c_in_b, const float* Wx, const float* bx, const float* a,
                 float* ba, int G, int B, int A, int C, void* stream);
int pd_denoise(const float* ba, const float* x_hat, const float* nw, const float* nb, const float* Wr, float eps,
               float c_skip, float c_out, const float* cs_b, const float* co_b, float* x_den, int B, int A, int C,
               void* stream);
int pd_kabsch_align(const float* x_pred, const float* pred_mask, const float* x_gt, long long gt_bstride, const float* w,
                    float* out, int B, int A, void* stream);
int pd_template_match(const float* x, const int* lig_idx, const float* ref_dist, const float* poses, float* batch_ref_pos,
                      float* eps_out, int* sel_out, int B, int A, int L, int Cn, void* stream);
int pd_pose_dist(const float* poses, float* D, int Cn, int L, void* stream);
/* pairwise RMSD matrix of n poses over the atoms idx[0..L) (NULL: first L atoms) and, if ref != NULL, the RMSD of
 * every pose to ref: the device half of the ranking step (redocking.py:357-423)                  */
int pd_pairwise_rmsd(const float* x, const int* idx, const float* ref, float* D, float* rmsd_ref, int n, int A, int L,
                     void* stream);
/* symmetry-corrected form of pd_pairwise_rmsd (sym_rmsd.hip; ABI 11, additive): perms_t [L][M] is a table of M permutations of
 * the L ligand atoms, atom-major (perms_t[a*M + m] = image of atom a under row m; row 0 the identity by convention).  For i < j
 *   D[i,j] = D[j,i] = sqrt( min_m (1/L) sum_a |x_i[idx[a]] - x_j[idx[perms[m][a]]]|^2 ),   D[i,i] = 0,
 * rmsd_ref[i] the same against ref [A,3] and best_perm_ref[i] the smallest m that attains the fp32 minimum (ref, and
 * best_perm_ref on its own, may be NULL).  Each sum runs over a in ascending order in one thread and the minimum is exact.
 * L <= 1024, M <= 65535, n <= 65535 (else PD_ERR_UNSUPPORTED).                                                              */
int pd_sym_rmsd(const float* x, const int* idx, const float* ref, const unsigned short* perms_t, float* D, float* rmsd_ref,
                int* best_perm_ref, int n, int A, int L, int M, void* stream);
/* best-fit (superposed) form of pd_sym_rmsd (bestfit_rmsd.hip, whose header comment holds the kernel's structure; ABI 11, additive): the
 * ligand-only RMSD minimised over rigid superpositions AND over the table rows - the conformer accuracy of a pose, wherever the ligand
 * sits (RDKit's GetBestRMS).  Rectangular: rows xa [na][Aa][3] gathered through idx_a [L], columns xb [nb][Ab][3] through idx_b [L]
 * (fp32; a NULL idx means atoms 0 .. L-1 and needs A >= L; the caller guarantees 0 <= idx < A - an entry outside is not followed and
 * makes its structure count as not finite).  perms_t [L][M] as for pd_sym_rmsd; NULL with M = 1: the identity alone.  With a, b the two
 * ligands centred on their unweighted centroids in float64, G their sums of squared norms and N Horn's 4x4 matrix (1987):
 *   msd(a, b, m) = min over PROPER rotations R of (1/L) sum_k |R a[k] - b[perms[m][k]]|^2 = (G_a + G_b - 2 lambda_max(N(a, b o perms[m]))) / L
 *   D[i,j]         (float) sqrt(max(0, min_m msd)): the float64 result rounded once; 0 for L = 1
 *   best_perm[i,j] (nullable, int32 [na][nb]) the smallest m that attains the float64 minimum
 *   quat[i,j]      (nullable, float64 [na][nb][4]) the unit eigenvector (w, x, y, z) of lambda_max for that m, first non-zero component
 *                  positive: R(quat) a ~ b o perms[m]; any optimal rotation where lambda_max is degenerate (collinear atoms, L <= 2)
 * A mirror image is not a match.  A non-finite coordinate in either structure gives NaN, -1 and NaN.  symmetric != 0 covers xb == xa (xb
 * NULL or xa, nb == na; idx_b / Ab unused): only i < j is computed (row i fixed, row j permuted) and mirrored, the diagonal is an exact 0;
 * best_perm and quat must then be NULL (PD_ERR_ARG).  ws: pd_bestfit_rmsd_workspace_numel(na, nb, L) = (na + nb) (3 L + 2) doubles (per
 * structure the centred coordinates, G and a finite flag; written by the first of the two launches, read by the second).  lambda_max by
 * cyclic Jacobi in float64, every sum in a fixed order, an exact minimum over m, no atomics: a value depends on its two structures and
 * the table alone - not on na, nb, the launch shape or the rest of the batch - and is bit-identical from call to call.  No allocation,
 * no synchronisation.  A NULL required pointer, a misaligned pointer (8 bytes for ws / quat, 4 for float / int, 2 for perms_t), a size
 * < 1 or a short workspace: PD_ERR_ARG; L > 1024, M > 65535, na or nb > 65535: PD_ERR_UNSUPPORTED.  A rejected call launches nothing.
 * tests/bestfit_rmsd_ref.py is the written definition.                                                                                */
int pd_bestfit_rmsd_workspace_numel(int na, int nb, int L);
int pd_bestfit_rmsd(const float* xa, const int* idx_a, const float* xb, const int* idx_b, const unsigned short* perms_t, double* ws,
                    long long ws_numel, float* D, int* best_perm, double* quat, int na, int nb, int Aa, int Ab, int L, int M,
                    int symmetric, void* stream);
/* Binding modes of n poses: greedy leader clustering on a distance matrix, best pose first, as Vina, AutoDock, GNINA and rDock report
 * them (cluster.hip; ABI 11, additive; the consumer of pd_pairwise_rmsd / pd_sym_rmsd and of 1 - pd_plif_pairwise - the reference runs
 * K-means(5) of scikit-learn on the host, redocking.py:389-416).  D [n][n] symmetric with a zero diagonal; order [n] the pose ids best
 * first, a permutation of 0 .. n-1 (an entry outside 0 .. n-1 is skipped and never followed); valid [n] bytes (NULL: all valid); score
 * [n] (NULL: none).  labels = -1, k = 0; for r = 0 .. n-1 and i = order[r], unless i is invalid or labelled: i leads cluster k, i and
 * every valid unlabelled j with D[i][j] <= cutoff (fp32, inclusive, false for a NaN) get label k, k += 1.  Invalid poses keep -1.
 *   labels[i], dist_to_leader[i]   the pose's cluster and D[its leader][i] (-1 and NaN for an invalid pose)
 *   leader[k], size[k], radius[k]  the leading pose, the number of members, the exact maximum of D[leader][member]
 *   medoid[k]                      the member i with the smallest s_i = sum over the OTHER members j, ascending, of (double)D[j][i] (fp64;
 *                                  a NaN counts as +inf), the smallest i on a tie
 *   spread[k]                      (float)((sum of s_i over the members, ascending) / (double)(size (size - 1))), 0 for a singleton
 *   mean_score[k]                  (float)((sum of (double)score[i] over the members, ascending) / (double)size), NaN without score
 *   n_clusters[0]                  k at the end
 * The per-cluster arrays hold n entries; those at k >= n_clusters are -1 (leader, medoid), 0 (size) and NaN (the floats).  ws:
 * pd_pose_clusters_workspace_numel(n) = n doubles (the s_i), written before they are read.  Only the rows of D that belong to leaders
 * and the columns of the poses are read.  Three launches, no atomics, no allocation, no synchronisation; maxima and sums in the
 * stated order: bit-identical from launch to launch.  n < 1, a NULL required pointer, a misaligned pointer (4 bytes for float / int,
 * 8 for ws), a negative or non-finite cutoff or a short workspace: PD_ERR_ARG; n > PD_POSE_CLUSTERS_MAX_POSES: PD_ERR_UNSUPPORTED.  A
 * rejected call writes nothing.  tests/pose_clusters_ref.py is the written definition.                                             */
#define PD_POSE_CLUSTERS_MAX_POSES 8192
int pd_pose_clusters_workspace_numel(int n);
int pd_pose_clusters(const float* D, const int* order, float cutoff, const unsigned char* valid, const float* score, double* ws,
                     long long ws_numel, int* labels, float* dist_to_leader, int* leader, int* size, float* radius, int* medoid,
                     float* spread, float* mean_score, int* n_clusters, int n, void* stream);
/* Distance-geometry conformers of one ligand: C independent float64 minimisations of a bounds error function from random 4-D
 * coordinates (conformers.hip; ABI 11, additive; the reference calls RDKit ETKDG on the host, redocking.py:231-243 - this is the
 * package's own definition, no metric-matrix eigen-solve and no torsion-knowledge terms; tests/conformers_ref.py is the written
 * definition).  Tables, built once per ligand (physdock_amd/conformers.py): lo, up [L][L] float64, the triangle-smoothed distance
 * bounds, symmetric; centres [n_centres][4] int32 (c, n1, n2, n3) with vol_lo <= vol_hi [n_centres] of the same sign.
 *   E(x), x [L][4] = sum_{i<j} [d2 > up2] (d2 / up2 - 1)^2 + [d2 < lo2] (2 lo2 / (lo2 + d2) - 1)^2     (d over four coordinates)
 *                  + w_chi sum_centres viol(V)^2 + w_4d sum_a x[a][3]^2
 *   V = (n1 - c) . ((n2 - c) x (n3 - c)) over the first three coordinates, viol = the distance of V to [vol_lo, vol_hi]
 * pd_dg_error_grad    : err [C] (nullable) = E and grad [C][L][4] (nullable) = dE/dx of pos [C][L][4]; not both NULL
 * pd_embed_conformers : one block per conformer, one launch.  Start: `start` [C][L][4], or if NULL uniform in [-box, box]^4, x =
 *                       (2 u - 1) box with u = (r_k + 0.5) 2^-32 in double and r = Philox4x32-10(key = seed, counter = (conformer,
 *                       atom, 0, 0)).  Stage 1 minimises E with (w_chi, w_4d) = (1, 0.1), stage 2 with (0.2, 1.0): the BFGS / lnsrch
 *                       of pd_mmff_relax (same constants, no gradient scaling) in dim = 4 L; a stage stops on max|grad| < grad_tol
 *                       (status 0), after max_iters accepted steps (1) or when the line search finds no lower point (2), as
 *                       pd_vina_refine.  Then the fourth coordinate is dropped, the conformer centred and rounded once to fp32 into
 *                       x [C][L][3].  ok [C] = 1 when, in 3-D and in double, the largest bound violation max(d - up, lo - d) is <=
 *                       0.1, every centre's V has the sign of vol_lo and max|x[a][3]| <= 0.1; else the row of x is zeros.  err [C] = E
 *                       at the end of stage 2, max_violation [C] that largest violation, iterations / status [C][2] per stage.
 *                       ws: pd_embed_conformers_workspace_numel(C, L) = C ((4 L)^2 + 8 * 4 L) doubles (the inverse Hessian; the
 *                       tail of conformer c, at ws + c ((4 L)^2 + 32 L) + (4 L)^2, receives the point stage 2 ended at, [L][4],
 *                       then its gradient, [L][4], accepted or not; the other 6 x 4 L doubles are not touched).
 * No atomics, every sum in a fixed order: bit-identical from call to call, and a conformer's result does not depend on C or on its
 * place among the C.  No allocation, no synchronisation.  A NULL required pointer, a misaligned pointer (8 bytes for doubles, 4 for
 * float / int), C, L < 1, n_centres < 0, max_iters < 0, grad_tol < 0, box <= 0 or a short workspace: PD_ERR_ARG; L >
 * PD_DG_MAX_ATOMS, n_centres > PD_DG_MAX_CENTRES, C > PD_DG_MAX_CONFORMERS: PD_ERR_UNSUPPORTED.  A rejected call writes nothing.   */
#define PD_DG_MAX_ATOMS 128
#define PD_DG_MAX_CENTRES 64
#define PD_DG_MAX_CONFORMERS 4096
int pd_embed_conformers_workspace_numel(int C, int L);
int pd_dg_error_grad(const double* lo, const double* up, const int* centres, const double* vol_lo, const double* vol_hi,
                     const double* pos, double w_chi, double w_4d, double* err, double* grad, int C, int L, int n_centres,
                     void* stream);
int pd_embed_conformers(const double* lo, const double* up, const int* centres, const double* vol_lo, const double* vol_hi,
                        unsigned long long seed, int max_iters, double grad_tol, double box, double* ws, long long ws_numel,
                        float* x, unsigned char* ok, double* err, double* max_violation, int* iterations, int* status,
                        const double* start, int C, int L, int n_centres, void* stream);
/* PoseBusters-style geometry checks of P poses of one ligand in its receptor, without leaving the device (validity.hip; ABI 11,
 * additive; the reference runs the `posebusters` package on the host through files, PhysDock/data/relaxation.py:24-50).  Tables,
 * built once per ligand (physdock_amd/validity.py): lig_idx [L] the ligand's atoms in a pose (any order, any place); radius [A] van
 * der Waals radii; rec_mask [A] 1 = the atom counts as receptor (never a ligand atom); lig_active [L] 0 = left out of the receptor
 * and the non-bonded check (a hydrogen), never of the bond / angle checks; pair12 [n12][2], pair13 [n13][2] local ligand indices
 * of the bonded and of the 1-3 pairs with their reference distances d12_ref, d13_ref; far [L][L] 1 = the pair is four or more bonds
 * apart or in different fragments (read for a < b); planar [G][8] local indices of the groups that must be flat, padded with -1.
 * Per pose p, with d the fp32 distance sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx))):
 *   val[p][0], [1]  min, max over bonded pairs of d / d12_ref        val[p][2], [3]  the same over 1-3 pairs and d13_ref
 *   val[p][4]       min over active far pairs of d / (r_a + r_b)
 *   val[p][5]       min over (active ligand atom a, receptor atom j) of d / (r_a + r_j);  worst[p] = the (a, j) that attains it,
 *                   the lexicographically smallest pair on an exact tie
 *   val[p][6]       min over the same pairs of d (Angstrom)
 *   val[p][7]       max over groups and their atoms of the distance (Angstrom, computed in double) to the group's least-squares
 *                   plane; 0 for a group whose atoms are collinear or coincident (second eigenvalue <= 1e-10 of the largest)
 *   flags[p]        bit 0: [0] < bond_lo or [1] > bond_hi; bit 1: the same for [2], [3] and angle_lo, angle_hi; bit 2: [4] <
 *                   internal_clash; bit 3: [5] < receptor_clash; bit 4: [7] > planarity; bit 5: detached < [6] < +inf - applied
 *                   to the values as stored
 * Empty sets (n12, n13, G may be 0; there may be no receptor atom) report 1 (columns 0 - 3), +inf (4 - 6), 0 (7), worst -1, and
 * set no bit.  ws: pd_pose_validity_workspace_numel(P, A) 64-bit words of scratch (2 P ceil(A / PD_VALIDITY_REC_TILE)), written
 * before they are read.  Results are bit-identical from launch to launch: minima of identically computed values, no atomics.
 * L <= 1024, G <= 256, A <= 2^22, P <= 65535 (else PD_ERR_UNSUPPORTED).                                                          */
#define PD_VALIDITY_REC_TILE 256
typedef struct pd_validity_thresholds {
    float bond_lo, bond_hi, angle_lo, angle_hi, internal_clash, receptor_clash, planarity, detached;
} pd_validity_thresholds;
int pd_pose_validity_workspace_numel(int P, int A);
int pd_pose_validity(const float* x, const int* lig_idx, const float* radius, const unsigned char* rec_mask,
                     const unsigned char* lig_active, const int* pair12, const float* d12_ref, const int* pair13,
                     const float* d13_ref, const unsigned char* far, const int* planar, pd_validity_thresholds thr,
                     unsigned long long* ws, float* val, int* worst, int* flags, int P, int A, int L, int n12, int n13, int G,
                     void* stream);
/* Stereochemistry checks of the RECEPTOR of P poses (receptor_geometry.hip, whose header comment holds the full definition; ABI 11,
 * additive; the thresholds are PoseBusters' ligand defaults and this package's own, unvalidated for proteins).  Tables, built once
 * per system (physdock_amd/receptor_geometry.py): radius [A] van der Waals radii, NEGATIVE for an atom that takes no part;
 * excl_start [A + 1] / excl_atom: per atom the partners with a HIGHER index that the clash check leaves out (up to three bonds apart,
 * or already clashing in the reference structure); term_atoms [T][PD_RECEPTOR_TERM_WIDTH] (-1 padded) and term_ref [T], the terms
 * in the order bonds (a, b; reference length), 1-3 pairs (the same), chiral centres (centre, a, b, c; sign +-1), peptide terms (CA, C,
 * N', CA'; 1 = trans in the reference), planar groups (4 .. 10 atoms); res_term_start [R + 1] / res_term: the terms that hold an atom
 * of each residue; res_atom_start [R + 1] / res_atom: its active atoms.  Per pose p:
 *   val[p][0..3]  min, max of d / reference over the bonds, over the 1-3 pairs (fp32; 1 without terms)
 *   val[p][4]     min over active, non-excluded pairs i < j of d / (r_i + r_j) (+inf without pairs);  worst[p] the pair, the smallest
 *                 (i, j) on an exact tie, (-1, -1) without pairs
 *   val[p][5]     max distance (Angstrom, double) of a group's atom to its least-squares plane;  val[p][6] max over the peptide terms
 *                 of min(|omega|, 180 - |omega|) in degrees (double);  val[p][7] the number of centres whose signed volume has the
 *                 wrong sign or is 0
 *   counts[p][7]  failing terms of bit 0 bond_lengths, 1 bond_angles, 2 chirality, 3 peptide_twist, 4 cis_flip, 5 planarity and
 *                 failing pairs of bit 6 clash;  flags[p] bit b = counts[p][b] > 0;  residue_flags [P][R], atom_clash [P][A],
 *                 term_val [P][T] fp32, term_fail [P][T] the same bits per residue, atom (0 / 1) and term
 * A non-finite coordinate fails every term and pair it enters.  ws: pd_receptor_geometry_workspace_numel(P, A) 64-bit words, written
 * before they are read.  No atomics: bit-identical from launch to launch and whatever P.  pd_receptor_dihedrals: angles [P][R][7]
 * fp32 degrees of the [R][7][4] index table (phi, psi, omega, chi1 - chi4; -1 = undefined -> NaN), computed in double.
 * A <= 4096, R <= 4096, T <= 2^20, P <= 65535 (else PD_ERR_UNSUPPORTED).                                                        */
#define PD_RECEPTOR_TERM_WIDTH 10
typedef struct pd_receptor_thresholds {
    float bond_lo, bond_hi, angle_lo, angle_hi, clash, planarity, twist, cis;
} pd_receptor_thresholds;
int pd_receptor_geometry_workspace_numel(int P, int A);
int pd_receptor_geometry(const float* x, const float* radius, const int* excl_start, const int* excl_atom, const int* term_atoms,
                         const float* term_ref, int n_bonds, int n_angles, int n_centres, int n_peptides, int n_groups,
                         const int* res_term_start, const int* res_term, const int* res_atom_start, const int* res_atom,
                         pd_receptor_thresholds thr, unsigned long long* ws, float* val, int* worst, int* counts, int* flags,
                         unsigned char* residue_flags, unsigned char* atom_clash, float* term_val, unsigned char* term_fail, int P,
                         int A, int R, void* stream);
int pd_receptor_dihedrals(const float* x, const int* dih, float* angles, int P, int A, int R, void* stream);
/* lDDT-PLI of P poses of one ligand in its receptor against one ground truth, maximised over the ligand's automorphisms
 * (lddt_pli.hip; ABI 11, additive).  Tables, built once per system on the host (physdock_amd/lddt_pli.py): lig_idx [L] the
 * ligand's atoms in a pose; the contacts of the ground truth in CSR form - contact_start [L+1], contact_atom [n_contacts] (pose
 * atom) and contact_dist [n_contacts] (its distance to ligand atom i in the ground truth); the candidate images of every ligand
 * atom in CSR form - cand_start [L+1], cand_atom [n_cand] (local ligand index; the distinct perms[:, i], ascending); slot_t
 * [L][M], atom-major as the table of pd_sym_rmsd: cand_atom[cand_start[i] + slot_t[i*M + m]] = perms[m][i].
 * pd_lddt_pli_counts:  counts[p][cand_start[i] + s][t] = #{ contacts c of i : | |x_p[lig_idx[k]] - x_p[contact_atom[c]]| -
 *   contact_dist[c] | < thr_t },  k = cand_atom[cand_start[i] + s], the distance as sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx))).
 *   An atom takes its contacts PD_LDDT_PLI_TILE at a time.  contact_atom / contact_dist may be NULL when n_contacts == 0.
 * pd_lddt_pli_select:  best_perm[p] = the smallest m that maximises sum_i sum_t counts[p][cand_start[i] + slot_t[i*M + m]][t];
 *   conserved[p][t] = that permutation's sum over i of the counts of threshold t; per_atom[p][i] = its sum over t for atom i /
 *   (4 |N(i)|), 0 for an atom without contacts; lddt[p] = sum_t conserved[p][t] / (4 n_contacts), 0 without contacts (one fp32
 *   division of the two integers each).  The totals of up to PD_LDDT_PLI_LDS_CAND candidates are kept in LDS, beyond that they
 *   are read from counts.
 * counts [P][n_cand][4] must be 16-byte aligned.  Integer sums throughout and an exact maximum: results do not depend on the
 * launch shape.  No allocation, no synchronisation.  L <= 1024, M <= 65535, P <= 65535, L <= n_cand <= L * L, n_contacts <=
 * PD_LDDT_PLI_MAX_CONTACTS (else PD_ERR_UNSUPPORTED).                                                                          */
#define PD_LDDT_PLI_TILE 512
#define PD_LDDT_PLI_LDS_CAND 4096
#define PD_LDDT_PLI_MAX_CONTACTS ((1 << 29) - 1)
int pd_lddt_pli_counts(const float* x, const int* lig_idx, const int* contact_start, const int* contact_atom,
                       const float* contact_dist, const int* cand_start, const int* cand_atom, float thr0, float thr1, float thr2,
                       float thr3, int* counts, int P, int A, int L, int n_contacts, int n_cand, void* stream);
int pd_lddt_pli_select(const int* counts, const int* contact_start, const int* cand_start, const unsigned short* slot_t,
                       float* lddt, int* conserved, float* per_atom, int* best_perm, int P, int L, int M, int n_cand, void* stream);
/* Vina-style receptor - ligand interaction score of P poses of one ligand in its receptor and its analytic gradient on the ligand
 * atoms (vina.hip; ABI 11, additive; the intermolecular part of the AutoDock Vina scoring function, Trott & Olson 2010, heavy atoms
 * only - the reference has no counterpart on the device, it relaxes through OpenMM on the host, PhysDock/data/relaxation.py).
 * Tables, built once per system (physdock_amd/scoring.py): lig_idx [L] the ligand's atoms in a pose; type [A] one byte per pose
 * atom - bits 0 - 3 the radius class (0 C 1.9, 1 N 1.8, 2 O 1.7, 3 P 2.1, 4 S 2.0, 5 F 1.5, 6 Cl 1.8, 7 Br 2.0, 8 I 2.2, 9 and above
 * 1.2 A), bit 4 hydrophobic, bit 5 hydrogen-bond donor, bit 6 acceptor; rec_mask [A] 1 = the atom counts as receptor (never a
 * ligand atom); lig_active [L] 0 = the ligand atom takes no part (a hydrogen, a masked atom) and reports zeros.  Per pose p, over
 * the pairs (active ligand atom i, receptor atom j) with r = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx))) < 8 and d = r - (R_i + R_j):
 *   atom_terms[p][i][t]  atom i's sums of gauss1 exp(-(d/0.5)^2), gauss2 exp(-((d-3)/2)^2), repulsion d^2 (d < 0), hydrophobic
 *                        (both bit 4: 1 for d <= 0.5, 1.5 - d below 1.5) and hbond (a donor and an acceptor: 1 for d <= -0.7, -d/0.7
 *                        below 0)
 *   terms[p][t]          their sums over the ligand atoms in ascending order
 *   inter[p]             -0.0356 gauss1 - 0.00516 gauss2 + 0.840 repulsion - 0.0351 hydrophobic - 0.587 hbond  (kcal/mol)
 *   score[p]             inter[p] / (1 + 0.0585 n_rot)
 *   per_atom[p][i]       the same weighted sum of atom_terms[p][i]
 *   forces[p][i][3]      -d inter[p] / d x_i (not scaled by the n_rot factor; a pair with r == 0 contributes nothing); may be NULL
 * Two launches, no atomics, no workspace beyond the outputs, no allocation, no synchronisation.  Every sum runs in a fixed order
 * inside one pose: results are bit-identical from launch to launch and independent of P and of a pose's place among the P.
 * float and int pointers must be 4-byte aligned and n_rot >= 0 (else PD_ERR_ARG); L <= 1024, A <= 2^22, P <= 65535 (else
 * PD_ERR_UNSUPPORTED).                                                                                                        */
#define PD_VINA_TERMS 5
int pd_vina_score(const float* x, const int* lig_idx, const unsigned char* type, const unsigned char* rec_mask,
                  const unsigned char* lig_active, float n_rot, float* atom_terms, float* terms, float* inter, float* score,
                  float* per_atom, float* forces, int P, int A, int L, void* stream);
/* Local refinement of P poses of one ligand in its rigid receptor, as a rigid body and about its rotatable bonds - the move set of
 * `vina --local_only` (vina_refine.hip; ABI 11, additive; the device counterpart of the reference's host relaxation through OpenMM,
 * PhysDock/data/relaxation.py, with another energy).  Tables, built once per system (physdock_amd/refine.py): lig_idx, type,
 * rec_mask, lig_active as pd_vina_score takes them; rot [T][2] the rotatable bonds (a_k, b_k) as LOCAL ligand indices, b_k on the
 * moving side; rot_mask [T][ceil(L / 32)] bit i % 32 of word i / 32 of row k = ligand atom i moves with torsion k (b_k does, a_k does
 * not; hydrogens move with their side); intra_start [L + 1] / intra_atom [2 n_intra]: for every ligand atom the ACTIVE atoms more
 * than three bonds away from it or in another component (ascending; every pair appears from both of its atoms).  All of it float64:
 *   E(y)      inter + intra: the pair function of pd_vina_score (five weighted terms of d = r - R_i - R_j, pairs with r < 8, no force
 *             from a pair at r == 0) over (active ligand atom, receptor atom) and over the intramolecular pairs; no n_rot factor
 *   move(y,s) s in R^(6+T): for k = 0 .. T-1 rotate the atoms of row k by s[6+k] about the axis through y[a_k] along y[b_k] - y[a_k]
 *             (Rodrigues, on the coordinates as they stand), then rotate all atoms about their unweighted centroid c by the rotation
 *             vector s[3:6], then translate by s[0:3]
 *   ggrad     at s = 0: [0:3] sum_i dE/dy_i, [3:6] sum_i (y_i - c) x dE/dy_i, [6+k] sum_{i in row k} dE/dy_i . (u_k x (y_i - y[a_k]))
 * pd_vina_refine_energy: energy, inter, intra [P], grad [P][L][3] = dE/dy (zeros for an inactive atom), ggrad [P][6+T] of the poses
 * as they are; any output may be NULL.  pd_vina_refine: BFGS with the line search of pd_mmff_relax (Numerical Recipes dfpmin /
 * lnsrch, same constants) in the 6 + T coordinates, the chart re-centred after every accepted step, the direction cut to |xi|_2 <=
 * max_step (A and radians) before each line search; it stops on max|ggrad| < grad_tol (status 0), after max_iters accepted steps
 * (1) or when the line search finds no lower point (2).  x_refined [P][A][3] = x with the ligand rows replaced; energy_start, energy
 * [P] (float64); iterations (accepted steps), evaluations (of E), status [P] (int32); moved [P] (float64): RMSD of the L ligand atoms
 * between start and end; energy_trace [P][max_iters + 1] (float64, may be NULL): E at the start and after each accepted step, padded
 * with the last value.  ws: pd_vina_refine_workspace_numel(P, L, T) = P ((6+T)^2 + 3 L) doubles.  One launch, one block per pose, no
 * atomics, no allocation, no synchronisation; every sum in a fixed order: bit-identical from launch to launch, independent of P and
 * of a pose's place among the P.  NULL required pointers, misaligned pointers (4 bytes for float / int, 8 for double), sizes < 1,
 * max_iters < 0, grad_tol < 0, max_step <= 0 or a short workspace: PD_ERR_ARG; L > 1024, T > PD_VINA_REFINE_MAX_TORSIONS, A > 2^22,
 * P > 65535: PD_ERR_UNSUPPORTED.  A rejected call writes nothing.  tests/vina_refine_ref.py is the written definition.            */
#define PD_VINA_REFINE_MAX_TORSIONS 58
int pd_vina_refine_workspace_numel(int P, int L, int T);
int pd_vina_refine_energy(const float* x, const int* lig_idx, const unsigned char* type, const unsigned char* rec_mask,
                          const unsigned char* lig_active, const int* rot, const unsigned* rot_mask, const int* intra_start,
                          const int* intra_atom, int n_intra, double* energy, double* inter, double* intra, double* grad,
                          double* ggrad, int P, int A, int L, int T, void* stream);
int pd_vina_refine(const float* x, const int* lig_idx, const unsigned char* type, const unsigned char* rec_mask,
                   const unsigned char* lig_active, const int* rot, const unsigned* rot_mask, const int* intra_start,
                   const int* intra_atom, int n_intra, int max_iters, double grad_tol, double max_step, double* ws,
                   long long ws_numel, float* x_refined, double* energy_start, double* energy, int* iterations, int* evaluations,
                   int* status, double* moved, double* energy_trace, int P, int A, int L, int T, void* stream);
/* pd_vina_refine with flexible receptor side chains, the move set of `vina --flex` (vina_flex.hip; ABI 11, additive;
 * physdock_amd/flex.py builds the tables, tests/flex_refine_ref.py is the written definition).  M = L + F movable rows: rows 0 .. L-1
 * the ligand atoms of pd_vina_refine's tables, rows L .. M-1 the flexible side-chain atoms; N = T + S torsions, the ligand's T
 * first.  Tables: mov_idx [M] the rows' pose indices; type [A]; fixed_mask [A] 1 = a receptor atom that is not flexible; active [M]
 * 1 = the row takes part in E (a ligand hydrogen does not); rot [N][2] (a_k, b_k) as LOCAL rows, b_k on the moving side (for a side
 * chain a_k on the backbone side, the distal side moves); rot_mask [N][ceil(M / 32)] the rows that move with torsion k; pair_start
 * [M + 1] / pair_atom [n_pair]: for every row the ACTIVE rows it forms a pair with (ascending LOCAL rows; every pair appears from
 * both of its rows) - ligand pairs as pd_vina_refine's intra list, every (ligand row, flexible row), and the flexible rows more
 * than three bonds apart; excl_start [M + 1] / excl_atom [n_excl]: for every flexible row the FIXED atoms (pose indices) within
 * three bonds of it (empty for a ligand row).  All of it float64:
 *   E(y)      (inter + intra) + receptor, every term the pair function of pd_vina_refine: inter over (active ligand row, fixed atom)
 *             and (ligand row, flexible row) pairs, intra over the ligand's pairs, receptor over (flexible row, fixed atom not in
 *             its excl list) and (flexible row, flexible row) pairs; no n_rot factor
 *   move(y,s) s in R^(6+N): the N torsions in table order as pd_vina_refine turns them, then the rotation s[3:6] about the centroid
 *             of the L ligand rows and the translation s[0:3], both of the ligand rows alone
 *   ggrad     [0:3] and [3:6] sum over the ligand rows, [6+k] over the rows of torsion k
 * pd_vina_flex_energy: energy, inter, intra, receptor [P], grad [P][M][3], ggrad [P][6+N] of the poses as they are; any output may
 * be NULL.  pd_vina_flex_refine: pd_vina_refine's minimiser (the same code), stopping rules and outputs in the 6 + N coordinates;
 * x_refined [P][A][3] = x with the movable rows replaced, every other row copied; inter, intra, receptor [P] (may be NULL): the parts
 * of `energy` (one more evaluation at the end, not counted in `evaluations`); moved [P]: RMSD of the L ligand rows, moved_flex [P] (may
 * be NULL): RMSD of the F flexible rows (0 when F == 0).  ws: pd_vina_flex_workspace_numel(P, M, N) = P ((6+N)^2 + 3 M) doubles.  One
 * launch, one block of 256 threads per pose, 6 M doubles of LDS, no atomics, every sum in a fixed order: bit-identical from launch
 * to launch and for a pose alone or inside a batch.  With F == S == 0 it is pd_vina_refine.  NULL required pointers, misaligned
 * pointers, sizes < 1 (F, T, S < 0), max_iters < 0, grad_tol < 0, max_step <= 0 or a short workspace: PD_ERR_ARG; M > 1024, N >
 * PD_VINA_REFINE_MAX_TORSIONS, A > 2^22, P > 65535: PD_ERR_UNSUPPORTED.  A rejected call writes nothing.  The indices inside the
 * tables are the caller's to keep in range.                                                                                    */
int pd_vina_flex_workspace_numel(int P, int M, int N);
int pd_vina_flex_energy(const float* x, const int* mov_idx, const unsigned char* type, const unsigned char* fixed_mask,
                        const unsigned char* active, const int* rot, const unsigned* rot_mask, const int* pair_start,
                        const int* pair_atom, int n_pair, const int* excl_start, const int* excl_atom, int n_excl, double* energy,
                        double* inter, double* intra, double* receptor, double* grad, double* ggrad, int P, int A, int L, int F,
                        int T, int S, void* stream);
int pd_vina_flex_refine(const float* x, const int* mov_idx, const unsigned char* type, const unsigned char* fixed_mask,
                        const unsigned char* active, const int* rot, const unsigned* rot_mask, const int* pair_start,
                        const int* pair_atom, int n_pair, const int* excl_start, const int* excl_atom, int n_excl, int max_iters,
                        double grad_tol, double max_step, double* ws, long long ws_numel, float* x_refined, double* energy_start,
                        double* energy, double* inter, double* intra, double* receptor, int* iterations, int* evaluations,
                        int* status, double* moved, double* moved_flex, double* energy_trace, int P, int A, int L, int F, int T,
                        int S, void* stream);
/* Monte-Carlo global search of P poses, K independent chains each: perturb, minimise locally with the BFGS of pd_vina_refine,
 * Metropolis test, keep the best (vina_refine.hip; ABI 11, additive; the loop every docking program that carries Vina's scoring
 * function runs - here the package's own definition, tests/vina_search_ref.py, not a port of Vina's monte_carlo).  Tables, E, move
 * and the minimiser as pd_vina_refine takes them.  For pose id q = pose0 + p and chain c, n = 6 + T:
 *   start     y = the ligand rows of x[p]; (cur, E_cur) = descend(y) from H = I; best = cur, best_step = 0 - exactly pd_vina_refine's
 *             result for the pose, in every chain
 *   step m    m = 1 .. steps_total.  Philox4x32-10, key (seed lo, seed hi): counter (q, c, m, 0) gives w0 .. w3, counter (q, c, m, 1)
 *             gives w4 as its first word; u_j = (w_j + 0.5) 2^-32 in float64; entity e = (w0 (2 + T)) >> 32 in integers.  s = 0, then
 *             e == 0: s[0:3] = translate_amp (2 u_{1..3} - 1);  e == 1: s[3:6] = rotate_amp (2 u_{1..3} - 1) (rotation vector, radians);
 *             e == 2 + k: s[6+k] = pi (2 u_1 - 1).  (new, E_new) = descend(move(cur, s)) from a fresh H = I.  Accept iff E_new is finite
 *             and (E_new < E_cur or u_4 < exp((E_cur - E_new) / temperature)); temperature (kcal/mol) may be +inf.  On accept cur = new.
 *             Independently: if E_new is finite and E_new < E_best, best = new and best_step = m.
 * One launch runs the steps step0 + 1 .. step0 + n_steps (step0 == 0 also initialises the state with the start descent; step0 +
 * n_steps <= steps_total, which sizes the traces).  The chain state lives in ws between launches, so a search cut into launches of
 * any lengths is bit-identical to one launch; x, the tables, the settings and ws must be the same in all of them.  Outputs, written
 * by every launch: x_chains [P][K][L][3] (fp32: each chain's best, rounded once), energy_chains, energy_start [P][K] (float64: E_best,
 * E after the start), best_step, accepted, evaluations (of E, the start included) [P][K] (int32).  Optional (may be NULL):
 * trace_energy [P][K][steps_total + 1] (float64: E after the start, then E_new of every step), trace_entity, trace_accept,
 * trace_iterations, trace_status [P][K][steps_total] (int32: of step m at index m - 1; iterations and status of its descent).
 * ws: pd_vina_search_workspace_numel(P, K, L, T) = P K ((6+T)^2 + 9 L + 8) doubles - a long long: 7 GB at the limits, a byte count
 * no int holds (negative: the error code).  One block of 256 threads per (pose, chain), 6 L doubles of LDS, no atomics, no allocation, no
 * synchronisation, every sum in the order pd_vina_refine uses: bit-identical from launch to launch, independent of P, K and pose0 +
 * p's place in the batch.  pd_vina_search_select: best_chain [P] (the chain with the lowest energy_chains, the lowest index on a
 * tie), energy [P], x_search [P][A][3] = x with the ligand rows of that chain; one block per pose.  NULL required pointers,
 * misaligned pointers, sizes < 1, pose0 < 0, step0 < 0, n_steps < 0, step0 + n_steps > steps_total, temperature not > 0 (NaN
 * included), an amplitude < 0 or NaN, a short workspace and pd_vina_refine's own rules: PD_ERR_ARG; L > 1024, T >
 * PD_VINA_REFINE_MAX_TORSIONS, A > 2^22, K > 64, P K > 65535: PD_ERR_UNSUPPORTED.  A rejected call writes nothing.             */
long long pd_vina_search_workspace_numel(int P, int K, int L, int T);
int pd_vina_search(const float* x, const int* lig_idx, const unsigned char* type, const unsigned char* rec_mask,
                   const unsigned char* lig_active, const int* rot, const unsigned* rot_mask, const int* intra_start,
                   const int* intra_atom, int n_intra, int max_iters, double grad_tol, double max_step, unsigned long long seed,
                   int pose0, int step0, int n_steps, int steps_total, double temperature, double translate_amp, double rotate_amp,
                   double* ws, long long ws_numel, float* x_chains, double* energy_chains, double* energy_start, int* best_step,
                   int* accepted, int* evaluations, double* trace_energy, int* trace_entity, int* trace_accept,
                   int* trace_iterations, int* trace_status, int P, int K, int A, int L, int T, void* stream);
int pd_vina_search_select(const float* x, const int* lig_idx, const float* x_chains, const double* energy_chains, int* best_chain,
                          double* energy, float* x_search, int P, int K, int A, int L, void* stream);
/* pd_vina_search over pd_vina_flex_refine's tables: the Monte-Carlo search with flexible side chains (vina_flex.hip; ABI 11,
 * additive; tests/flex_search_ref.py is the written definition).  Tables, E = (inter + intra) + receptor, move and the minimiser as
 * pd_vina_flex_refine takes them, M = L + F, N = T + S, n = 6 + N; start, draws, Metropolis test and best as pd_vina_search, with
 * two changes: the entity is e = (w0 (2 + N)) >> 32, and e == 2 + k proposes s[6+k] = pi (2 u_1 - 1) for a ligand torsion (k < T),
 * chi_amp (2 u_1 - 1) for a side-chain torsion (T <= k < N).  The rigid part of a proposal acts on the ligand rows alone; every
 * descent runs in all n coordinates from a fresh H = I.  With F == S == 0 it is pd_vina_search.  step0, n_steps, steps_total and the
 * workspace as there: the chain state (H [n][n], pos, cur, best [M][3], E_cur, E_best, E_start, the counters) lives in ws between
 * launches and a search cut into launches is the same search bit for bit.  Outputs, written by every launch: x_chains [P][K][M][3]
 * (fp32: the movable rows of each chain's best), energy_chains, energy_start [P][K], best_step, accepted, evaluations [P][K]; the
 * five traces of pd_vina_search (may be NULL).  ws: pd_vina_flex_search_workspace_numel(P, K, M, N) = P K (n^2 + 9 M + 8) doubles
 * (13 320 per chain at M = 1024, n = 64; negative: the error code).  One block of 256 threads per (pose, chain), 6 M doubles of LDS,
 * no atomics, every sum in pd_vina_flex_refine's order.
 * pd_vina_flex_search_select (one block per pose, after the last launch, same ws): best_chain [P] = the chain with the lowest E_best
 * in ws (the lowest index on a tie); x_search [P][A][3] = x with the movable rows of that chain's float64 best, rounded once;
 * energy [P] and inter, intra, receptor [P] (may be NULL) from one more evaluation of it (not counted), energy == (inter + intra) +
 * receptor; moved [P], moved_flex [P] (may be NULL): RMSD of the ligand rows and of the flexible rows from x (0 when F == 0).
 * Errors as pd_vina_search and pd_vina_flex_refine, checked in the latter's order (chi_amp < 0 or NaN: PD_ERR_ARG); M > 1024, N >
 * PD_VINA_REFINE_MAX_TORSIONS, A > 2^22, K > 64, P K > 65535: PD_ERR_UNSUPPORTED.  A rejected call writes nothing.             */
long long pd_vina_flex_search_workspace_numel(int P, int K, int M, int N);
int pd_vina_flex_search(const float* x, const int* mov_idx, const unsigned char* type, const unsigned char* fixed_mask,
                        const unsigned char* active, const int* rot, const unsigned* rot_mask, const int* pair_start,
                        const int* pair_atom, int n_pair, const int* excl_start, const int* excl_atom, int n_excl, int max_iters,
                        double grad_tol, double max_step, unsigned long long seed, int pose0, int step0, int n_steps,
                        int steps_total, double temperature, double translate_amp, double rotate_amp, double chi_amp, double* ws,
                        long long ws_numel, float* x_chains, double* energy_chains, double* energy_start, int* best_step,
                        int* accepted, int* evaluations, double* trace_energy, int* trace_entity, int* trace_accept,
                        int* trace_iterations, int* trace_status, int P, int K, int A, int L, int F, int T, int S, void* stream);
int pd_vina_flex_search_select(const float* x, const int* mov_idx, const unsigned char* type, const unsigned char* fixed_mask,
                               const unsigned char* active, const int* rot, const unsigned* rot_mask, const int* pair_start,
                               const int* pair_atom, int n_pair, const int* excl_start, const int* excl_atom, int n_excl,
                               const double* ws, long long ws_numel, int* best_chain, double* energy, double* inter, double* intra,
                               double* receptor, float* x_search, double* moved, double* moved_flex, int P, int K, int A, int L,
                               int F, int T, int S, void* stream);
/* Protein - ligand interaction fingerprint of P poses of one ligand in its receptor: which residues does a pose touch, and how?
 * (plif.hip; ABI 11, additive; per-residue fingerprints in the manner of PLIP and ProLIF, heavy atoms only - the reference has no
 * counterpart.)  Tables, built once per system (physdock_amd/interactions.py): lig_idx [L] the ligand's atoms in a pose;
 * lig_active [L] 0 = the ligand atom takes no part (a hydrogen) and reports 0; type [A] the type byte of pd_vina_score (bit 4
 * hydrophobic, bit 5 donor, bit 6 acceptor; bits 0 - 3 are not looked at); charge [A] bit 0 cation, bit 1 anion; the receptor
 * atoms sorted by residue: res_start [R + 1] ascending from 0, res_atom [N] with N = res_start[R] <= A (distinct pose atoms, never
 * a ligand atom; the atoms of residue s are res_atom[res_start[s] .. res_start[s + 1]), a residue may own none).  thresholds: FOUR
 * floats ON THE HOST, read by the call and passed on as values: contact, hydrophobic, hbond, ionic (A).  Per pose p, over the pairs
 * (active ligand atom i, receptor atom j) with r = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx))), bit k of a byte = kind k:
 *   0 contact         r < thresholds[0]                                      3 hbond_acceptor  i acceptor, j donor,  r < thresholds[2]
 *   1 hydrophobic     both hydrophobic,    r < thresholds[1]                 4 cationic        i cation,   j anion,  r < thresholds[3]
 *   2 hbond_donor     i donor, j acceptor, r < thresholds[2]                 5 anionic         i anion,    j cation, r < thresholds[3]
 *   bits[p][s]          OR over the pairs whose receptor atom lies in residue s (bits 6 and 7 are 0)
 *   ligand_bits[p][i]   OR over the receptor atoms for ligand atom i
 *   min_dist[p][s]      the exact minimum of r over the residue's pairs; +inf without receptor atom or without active ligand atom
 *   counts[p][k]        the number of residues whose byte has bit k
 * ws_bits [P * N] bytes and ws_min [P * N] floats are the workspace (may be NULL when N == 0).  Three launches, no atomics, no
 * allocation, no synchronisation; OR, minimum and integer sums only: bit-identical from launch to launch, independent of P and
 * of a pose's place among the P.  float and int pointers must be 4-byte aligned, sizes positive (N >= 0, N <= A), thresholds
 * finite and not negative (else PD_ERR_ARG); L <= 1024, A <= 2^22, P <= 65535, R <= A (else PD_ERR_UNSUPPORTED).  A rejected
 * call writes nothing.                                                                                                         */
#define PD_PLIF_KINDS 6
#define PD_PLIF_THRESHOLDS 4
int pd_plif_fingerprint(const float* x, const int* lig_idx, const unsigned char* type, const unsigned char* charge,
                        const unsigned char* lig_active, const int* res_start, const int* res_atom, const float* thresholds,
                        unsigned char* ws_bits, float* ws_min, unsigned char* bits, unsigned char* ligand_bits, float* min_dist,
                        int* counts, int P, int A, int L, int R, int N, void* stream);
/* bits [P][R] against one reference row ref_bits [R] (it may be a row of bits), both masked with kind_mask (bit k = kind k counts;
 * 0 .. 63): shared[p] = popcount(bits & ref & mask), n_pose[p] = popcount(bits & mask), n_ref[0] = popcount(ref & mask) (int32,
 * summed over the residues), recovery[p] = shared / n_ref (1 where n_ref == 0), tanimoto[p] = shared / (n_pose + n_ref - shared)
 * (1 where the union is empty) - each ONE fp32 division of two integers (exactly representable up to 2^24).  One block per pose. */
int pd_plif_compare(const unsigned char* bits, const unsigned char* ref_bits, int kind_mask, int* shared, int* n_pose, int* n_ref,
                    float* recovery, float* tanimoto, int P, int R, void* stream);
/* tanimoto [P][P]: the same Tanimoto between every two rows of bits [P][R]; symmetric, the diagonal exactly 1; row p equals
 * pd_plif_compare against row p bit for bit.  One thread per pair, 16 x 16 pairs per block.  Limits and codes as above.          */
int pd_plif_pairwise(const unsigned char* bits, int kind_mask, float* tanimoto, int P, int R, void* stream);
/* Ring interactions of P poses of one ligand in its receptor: pi-stacking, pi-cation and halogen bonds per residue - the kinds
 * pd_plif_fingerprint leaves out (plif_rings.hip, whose header comment holds the full definition; ABI 11, additive; the conditions
 * and default thresholds are PLIP's published ones - the reference has no counterpart).  x, lig_idx, type, charge, lig_active,
 * res_start and res_atom are exactly what pd_plif_fingerprint takes; the receptor's CATION (charge bit 0) and ACCEPTOR (type bit 6)
 * atoms are found through res_atom.  Rings as a CSR over pose atoms: ring g is ring_atom[ring_start[g] .. ring_start[g + 1]) in
 * cyclic order, 3 .. 8 atoms, the ligand's G_l rings first (ring_residue -1), then the receptor's G_r rings IN ASCENDING ORDER OF
 * ring_residue [G_l + G_r], the residue a ring belongs to.  halogen [H][2]: ligand-local indices (X, C).  thresholds: EIGHT doubles
 * ON THE HOST, passed on as values - the five distances stack_dist, stack_offset, pication_dist, pication_offset, halogen_dist (A),
 * then the three cosines of parallel_angle, t_angle, halogen_angle.  In double from the fp32 coordinates: centroid c = mean of the
 * ring's atoms, normal n = sum_i (a_i - c) x (a_{i+1} - c) normalised; a ring whose normal has zero or non-finite length, with a
 * non-finite coordinate, a size outside 3 .. 8 or an atom outside 0 .. A - 1 is degenerate, takes part in nothing and reports n = 0
 * (ring_start is a device array: the call cannot reject a ring size).  Bit k of a byte = kind k:
 *   0 pi_parallel   ligand ring g, receptor ring h: |c_g - c_h| < t[0], min(off_gh, off_hg) < t[1], |n_g . n_h| > t[5]
 *   1 pi_tshaped    the same distance and offset, |n_g . n_h| < t[6]
 *   2 pi_cation     ligand ring g, receptor cation j: |x_j - c_g| < t[2], the offset of x_j on the plane of g < t[3]
 *   3 cation_pi     active ligand cation i, receptor ring h: the same with the roles swapped
 *   4 halogen_bond  active ligand halogen X with its carbon C, receptor acceptor j: |x_X - x_j| < t[4], cos(C - X ... j) < t[7]
 * with off_gh = sqrt(max(0, d^2 - ((c_h - c_g) . n_g)^2)).  Bits 5 - 7 are 0; a NaN fails every comparison.
 *   bits[p][s]               OR over the rings, cations and acceptors of residue s
 *   ligand_bits[p][i]        OR per ligand atom (a ring's byte goes to its atoms, bit 4 to X, bit 3 to the cation; inactive: 0)
 *   ring_bits[p][g]          OR per ligand ring
 *   centroid, normal         [P][G_l + G_r][3] doubles
 *   min_centroid_dist[p][s]  the smallest ligand-ring to residue-ring centroid distance, minimum in double, rounded once; +inf
 *                            when either side has no ring that is not degenerate
 *   counts[p][k]             residues per kind, [P][5]
 * workspace: pd_plif_rings_workspace(P, L, N, G_l, G_r, H) bytes, 8-byte aligned (the function returns PD_ERR_UNSUPPORTED when the
 * size does not fit an int).  Four launches, no atomics, no allocation, no synchronisation; OR, exact minima and integer sums only:
 * bit-identical from launch to launch, independent of P and of a pose's place among the P.  PD_ERR_ARG: a required pointer is NULL
 * (res_atom may be when N == 0; ring_start, ring_atom, ring_residue, centroid and normal when G_l + G_r == 0; ring_bits when G_l ==
 * 0; halogen when H == 0), P, A, L or R not positive, a negative count, N > A, an int or float pointer off 4-byte or a double
 * pointer (thresholds and workspace included) off 8-byte alignment, a negative or non-finite distance, a cosine outside [-1, 1], a
 * short workspace.  PD_ERR_UNSUPPORTED: L > 1024, G_l > 64, G_r > 4096, H > 64, A > 2^22, P > 65535, R > A.  A rejected call writes
 * nothing.                                                                                                                       */
#define PD_PLIF_RING_KINDS 5
#define PD_PLIF_RING_THRESHOLDS 8
int pd_plif_rings(const float* x, const int* lig_idx, const unsigned char* type, const unsigned char* charge,
                  const unsigned char* lig_active, const int* res_start, const int* res_atom, const int* ring_start,
                  const int* ring_atom, const int* ring_residue, int G_l, int G_r, const int* halogen, int H,
                  const double* thresholds, void* workspace, size_t workspace_bytes, unsigned char* bits,
                  unsigned char* ligand_bits, unsigned char* ring_bits, double* centroid, double* normal, float* min_centroid_dist,
                  int* counts, int P, int A, int L, int R, int N, void* stream);
int pd_plif_rings_workspace(int P, int L, int N, int G_l, int G_r, int H);
/* Riding hydrogens of P poses of one ligand in its receptor, and the hydrogen bonds they make with the D - H ... A angle
 * (hydrogens.hip, whose header comment holds the full definition; ABI 11, additive; bond lengths and thresholds are this package's
 * defaults, the bond conditions PLIP's published ones - the reference has no counterpart).  Hydrogen table, H rows, built once per
 * system (physdock_amd/hydrogens.py): parent [H] the pose atom a hydrogen rides on; ref [H][3] pose atoms n1, n2, n3 (-1 unused);
 * mode [H] one of PD_H_*; length [H] (A), angle_a [H], angle_b [H] (radians); side [H] 0 receptor, 1 ligand.  In double from the fp32
 * coordinates, with p the parent, u_i = unit(n_i - p), rounded once to fp32:
 *   PD_H_TRI     H = p + length unit(-(u1 + u2 + u3))
 *   PD_H_BISECT  H = p + length (cos a unit(-(u1 + u2)) + sin a unit(u1 x u2))
 *   PD_H_NERF    bc = unit(p - n1), n = unit((n1 - n2) x bc), m = n x bc; H = p + length (-cos a bc + sin a (cos b m + sin b n))
 *   PD_H_LINEAR  H = p + length unit(p - n1)
 * A hydrogen is not placed (x_h NaN, placed 0) when a vector to be normalised is shorter than 1e-6, a coordinate it reads is not
 * finite, a ref its mode needs is -1 or outside 0 .. A - 1, or its mode is none of the four.  group_h [G][3]: the rows of a rotor
 * group - one OH / SH (row, -1, -1; 12 candidates) or one NH3+ (three rows; 4 candidates), NERF rows sharing parent, n1, n2.
 * Candidate k adds k * 30 degrees to every b; its score is the smallest |A - H| over the group's hydrogens and the finite entries A
 * of the other molecule's part of acc with |A - p| <= d_da; the smallest score wins, a tie goes to the smaller k, without such an
 * acceptor k = 0; with orient == 0, or a row that is not placed, the group keeps its default angles and reports 0.  acc [NA_r +
 * NA_l]: the receptor's acceptor atoms sorted by residue, then the ligand's.
 *   x_h [P][H][3]  placed [P][H]  rotor_choice [P][G]
 * Two launches, no atomics, no allocation; exact minima only: bit-identical from launch to launch, independent of P and of a pose's
 * place among the P.  PD_ERR_ARG: a required pointer is NULL (group_h and rotor_choice may be when G == 0, acc when NA_r + NA_l ==
 * 0), P, A or H not positive, a negative count, G > H, NA_r + NA_l > A, an int or float pointer off 4-byte alignment, d_da negative
 * or not finite.  PD_ERR_UNSUPPORTED: H > 65535, A > 2^22, P > 65535.  A rejected call writes nothing.                            */
#define PD_H_TRI 0
#define PD_H_BISECT 1
#define PD_H_NERF 2
#define PD_H_LINEAR 3
int pd_place_hydrogens(const float* x, const int* parent, const int* ref, const unsigned char* mode, const float* length,
                       const float* angle_a, const float* angle_b, const unsigned char* side, const int* group_h, int G,
                       const int* acc, int NA_r, int NA_l, double d_da, int orient, float* x_h, unsigned char* placed,
                       int* rotor_choice, int P, int A, int H, void* stream);
/* The hydrogen bonds of the placed hydrogens.  polar [HP_l + HP_r]: the rows whose parent is N, O or S, the ligand's first, then the
 * receptor's sorted by the residue of the parent (rh_start [R + 1]: the CSR of that part); polar_slot [H]: a row's place in polar or
 * -1; acc, NA_r, NA_l as above (racc_start [R + 1]: the CSR of the receptor's part); lig_idx [L]; lig_acc_slot [L]: a ligand atom's
 * place in the ligand's part of acc or -1.  thresholds: TWO doubles ON THE HOST - d_da (A) and cos(angle_min).  A placed polar
 * hydrogen H on D and an acceptor A of the other molecule bond iff |D - A| <= t[0] and (D - H) . (A - H) <= t[1] |D - H| |A - H|,
 * in double on x and on the fp32 x_h as stored; a NaN fails.  Bit 0 hbond_donor (the ligand donates), bit 1 hbond_acceptor.
 *   bits[p][s]         bit 0: a ligand hydrogen bonds to an acceptor of residue s; bit 1: a hydrogen of residue s to a ligand acceptor
 *   ligand_bits[p][i]  bit 0: a hydrogen on ligand atom i donates; bit 1: ligand atom i accepts
 *   h_bits[p][h]       the bit of the row's side when it bonds to anything
 *   counts[p][k]       (hydrogen, acceptor) pairs per kind, [P][2]
 * workspace: pd_hydrogen_bonds_workspace(P, HP_l, HP_r, NA_r, NA_l) bytes (at least 8; PD_ERR_UNSUPPORTED when an int cannot hold
 * them), 8-byte aligned: a pair count per polar row and a byte per (row, acceptor of the other side).  Two launches, no atomics, no
 * allocation; OR and integer sums only: bit-identical as above.  PD_ERR_ARG: a required pointer is NULL (polar may be when HP_l +
 * HP_r == 0, acc when NA_r + NA_l == 0), a size not positive, a negative count, NA_r + NA_l > A, misalignment (thresholds and
 * workspace: 8 bytes), d_da negative or not finite, a cosine outside [-1, 1], a short workspace.  PD_ERR_UNSUPPORTED: H > 65535,
 * HP_l + HP_r > H, L > 1024, NA_l > 1024, A > 2^22, P > 65535, R > A.  A rejected call writes nothing.                                */
#define PD_HBOND_KINDS 2
#define PD_HBOND_THRESHOLDS 2
int pd_hydrogen_bonds(const float* x, const float* x_h, const unsigned char* placed, const int* parent, const int* polar, int HP_l,
                      int HP_r, const int* polar_slot, const int* acc, int NA_r, int NA_l, const int* racc_start, const int* rh_start,
                      const int* lig_idx, const int* lig_acc_slot, const double* thresholds, void* workspace, size_t workspace_bytes,
                      unsigned char* bits, unsigned char* ligand_bits, unsigned char* h_bits, int* counts, int P, int A, int H, int L,
                      int R, void* stream);
int pd_hydrogen_bonds_workspace(int P, int HP_l, int HP_r, int NA_r, int NA_l);
/* SD file records of n ligand poses, formatted on the device (sdf.hip; ABI 11, additive; the CTfile V2000 specification, THIS
 * PACKAGE'S definition - tests/sdf_ref.py writes it down - and not RDKit's bytes: no time stamp, no wedge flags, charges only as M  CHG).
 * Tables, built once per ligand (physdock_amd/sdfio.py): tmpl [M] the molblock (title, program line, comment, counts line, one
 * 69-column atom line per atom with 30 blank coordinate columns, bond lines, M  CHG lines, M  END, each with its newline); map [M]:
 * < 0 copies tmpl[i], 30 s + col fills column col (0 .. 29) of template atom s; atom [na] the index into a pose of every template
 * atom; hdr the item headers ">  <name>\n" one behind the other with hdr_start [K + 1]; decimals [K]: d = 0 .. 8 - values[k][p] [K][P]
 * holds the bits of a float32 printed as Python's f"{v:.{d}f}" (nothing padded; "-0.0000", "nan", "inf", "-inf") -, < 0 - an int32
 * printed as str(v).  Record r shows pose p = order[r] (order NULL: p = r; values are indexed by pose) and is
 *   the molblock, column col of atom s holding character col % 10 of f"{v:10.4f}", v = x[p][atom[s]][col / 10];
 *   per item: its header, the value's text, "\n\n";   then "$$$$\n".
 * |v| 10^d is exact in float64 for a float32 v and d <= 8 (24 significand bits, at most 19 for 5^8), so rint of it is the
 * round-half-even of the correctly rounded decimal conversion and every digit comes from that integer; the sign survives rounding to
 * zero.  Counted in *overflow (the caller zeroes and reads it): a coordinate that is not finite or does not fit its 10 columns (after
 * rounding above 99999.9999 or below -9999.9999), written as '*' in every column; a value with |v| 10^d >= 1e15, written as a single
 * '*'; every number of a record whose order[r] is outside 0 .. P-1 (written from pose 0).
 *   out [capacity]     the records one behind the other: a valid SD file as it stands
 *   offsets [n + 1]    int64, record r is out[offsets[r] .. offsets[r + 1]); offsets[n] is the size of the file
 *   vlen [n][K]        workspace: the length of every value's text
 * fixed: the bytes of a record that are not a value's text (M, the headers, two newlines per item, 5 for "$$$$\n"); longest: fixed +
 * the longest text of every value (18 for a float32, 11 for an int32); capacity >= n * longest.  Nothing is written at or behind
 * out[capacity].  Three launches on the stream - measure (skipped when K == 0), an int64 exclusive scan in one block, one thread per
 * byte -, no atomics but the overflow counter, no allocation.  PD_ERR_ARG: a required pointer is NULL (order may be; hdr, hdr_start,
 * decimals, values, vlen may be when K == 0), n outside 1 .. 65535, K outside 0 .. PD_SDF_MAX_ITEMS, a size not positive, fixed <
 * M + 5 + 6 K, longest < fixed + K, capacity < n * longest.                                                                          */
#define PD_SDF_MAX_ITEMS 32
int pd_sdf_format(const float* x, const unsigned char* tmpl, const int* map, const int* atom, const int* order,
                  const unsigned char* hdr, const int* hdr_start, const int* decimals, const int* values, unsigned char* vlen,
                  long long* offsets, unsigned char* out, int* overflow, int n, int P, int A, int M, int K, int fixed, int longest,
                  long long capacity, void* stream);
/* Ligand burial and interface area of P poses of one ligand in its receptor: solvent-accessible surface area by point counting
 * (sasa.hip; ABI 11, additive; Shrake & Rupley 1973, HEAVY ATOMS ONLY - absolute areas are not comparable with all-atom tools, and
 * the default radii and probe have not been validated on real complexes; the reference has no counterpart).  Tables, built once
 * per system (physdock_amd/surface.py): cls [A] one byte per pose atom - 0 ignored (padding, an atom that does not exist, an
 * inactive ligand atom), 1 receptor, 2 ligand; radius [A] (A); unit [n_points][3] the golden spiral in fp32 (t = k + 0.5, z = 1 -
 * 2 t / n, phi = t pi (3 - sqrt 5), u_k = (sqrt(1 - z^2) cos phi, sqrt(1 - z^2) sin phi, z), computed in float64); lig_idx [L] the
 * ligand's atoms in a pose (cls 2 or 0); polar [L] 1 = the ligand atom counts as polar; the receptor atoms (cls 1) sorted by
 * residue, res_start [R + 1] / res_atom [N] as pd_plif_fingerprint takes them; probe (A) by value.  For pose p and atom i of class
 * c != 0, with R_i = radius_i + probe: the point p_ik = x_i + R_i u_k (per coordinate fmaf(R_i, u, x_i)) is covered by atom j iff
 * j != i (by index), cls_j != 0 and fmaf(dz, dz, fmaf(dy, dy, dx * dx)) < R_j * R_j with d = p_ik - x_j; same_k: a covering j has
 * class c, other_k: one has the other class; n_free[i] = #{k: !same_k}, n_bound[i] = #{k: !same_k && !other_k}, n_buried = n_free -
 * n_bound; area(m, i) = (float)m * ((12.566370614359172f * (R_i * R_i)) / (float)n_points) in A^2.
 *   free_points[p][s]      n_free of ligand atom lig_idx[s] (0 for an inactive one)
 *   buried_points[p][a]    n_buried of every pose atom (0 for an ignored atom and for a receptor atom no ligand atom reaches)
 *   per_atom[p][s]         area(n_buried) of ligand atom s
 *   totals[t][p]           PD_SASA_TOTALS rows of P: 0 ligand_free, 1 ligand_bound, 2 ligand_buried (sums of area(n_free), area(n_bound),
 *                          area(n_buried) over the ligand atoms in ascending order), 3 buried_fraction = buried / free (0 where free
 *                          is 0), 4 buried_polar, 5 buried_apolar (ligand_buried split by polar), 6 receptor_buried (sum over the
 *                          receptor atoms in ascending atom order), 7 interface_area = (ligand_buried + receptor_buried) / 2
 *   residue_buried[p][r]   sum of area(n_buried) over the residue's receptor atoms in the order of its run
 *   interface_residues[p]  the number of residues with residue_buried > 0
 * ws_free [P * A] ints is the workspace.  The neighbour list of an atom is walked in pieces of PD_SASA_LIST or more entries: no
 * input is truncated.  Two launches, no atomics, no allocation, no synchronisation; "any", integer sums and float sums in a fixed
 * order: bit-identical from launch to launch, independent of P and of a pose's place among the P.  float and int pointers must be
 * 4-byte aligned, sizes positive (N >= 0, N <= A), probe finite and not negative (else PD_ERR_ARG); n_points <= PD_SASA_MAX_POINTS,
 * L <= 1024, A <= 2^22, P <= 65535, R <= A (else PD_ERR_UNSUPPORTED).  A rejected call writes nothing.                             */
#define PD_SASA_MAX_POINTS 1024
#define PD_SASA_LIST 256
#define PD_SASA_TOTALS 8
int pd_buried_surface(const float* x, const unsigned char* cls, const float* radius, const float* unit, const int* lig_idx,
                      const unsigned char* polar, const int* res_start, const int* res_atom, float probe, int* ws_free,
                      int* free_points, int* buried_points, float* per_atom, float* totals, float* residue_buried,
                      int* interface_residues, int P, int A, int L, int R, int N, int n_points, void* stream);
/* Pocket volume, enclosure and lining residues of P poses of one system on a lattice around the ligand (pocket.hip; ABI 11,
 * additive; the grid method of LIGSITE, Hendlich, Rippmann & Barnickel 1997, and POVME; HEAVY ATOMS ONLY; the default spacing, probe,
 * lining distance, reach and enclosure threshold are this package's own and have not been validated on real complexes; the reference
 * has no counterpart).  Tables, built once per system (physdock_amd/pocket.py): cls [A] and radius [A] as pd_buried_surface takes them,
 * lig_idx [L], the receptor atoms by residue res_start [R + 1] / res_atom [N].  tests/pocket_ref.py is the written definition.
 *   centre     centre == NULL: the float64 mean of the active ligand atoms (cls 2) of the pose, summed in lig_idx order and rounded
 *              once to fp32; else centre[p * centre_stride + 0 .. 2] (centre_stride 0: one centre for all poses, 3: one each).  With
 *              snap != 0 each coordinate c becomes fl32(h * rint(c / h)), evaluated in float64.  centre_used [P][3] is what was used.
 *   lattice    n points per axis, spacing h (fp32); in float64 o = centre - (h (n - 1)) / 2, point (i, j, k) is g = o + (i, j, k) h
 *              and has the linear index (i n + j) n + k
 *   predicates in float64 from the fp32 inputs, d = sqrt((dx dx + dy dy) + dz dz) without fused multiply-add:
 *              solid(g): a receptor atom j has d(g, x_j) < radius_j + probe;  inside(g): an active ligand atom i has d(g, x_i) <
 *              radius_i;  near(g, j): d(g, x_j) < radius_j + lining for a receptor atom j.  (The kernels decide a pair in fp32 only
 *              outside a guard band of 2^-20 (h (n - 1) + threshold) around the threshold - derived in pocket.hip - and evaluate it
 *              in float64 inside: the result is the float64 predicate.)
 *   buried(g)  of the seven directions (1,0,0) (0,1,0) (0,0,1) (1,1,1) (1,1,-1) (1,-1,1) (-1,1,1) the number in which a solid point
 *              lies within steps[d] lattice steps of g in the + sense and in the - sense; leaving the lattice is no hit.  steps is a
 *              HOST array of seven ints, floor(reach / (h |d|)) by the caller.
 *   pocket     not solid and buried >= min_enclosed (0 .. 7).  Pocket points form 6-connected components; a pocket point with inside is
 *              occupied; the site is the union of the components that hold an occupied point.
 *   classes[p][g]        0 solid, 1 free but not pocket, 2 pocket outside the site, 3 site and empty, 4 site and occupied
 *   buried[p][g]         buried(g); 0 for a solid point
 *   counts[p][0 .. 7]    n_solid, n_free (every non-solid point), n_pocket, n_site, n_occupied, n_ligand (non-solid points with
 *                        inside), n_components, n_site_components
 *   truncated[p]         1: a site point lies on a face of the lattice
 *   values[v][p]         PD_POCKET_VALUES rows of P: 0 site_volume = n_site h^3, 1 unfilled_volume = (n_site - n_occupied) h^3, 2
 *                        pocket_volume = n_pocket h^3 (the product in float64, rounded once), 3 filled_fraction = n_occupied / n_site,
 *                        4 ligand_in_site = n_occupied / n_ligand (0 where the divisor is 0), 5 ligand_enclosure = the mean of
 *                        atom_buried / 7 over the ligand atoms that have a point (0 when none has)
 *   atom_class[p][s], atom_buried[p][s]   class and buried of the lattice point nearest ligand atom s, rint((x - o) / h) per axis in
 *                        float64; 255 for an inactive atom and for one outside the lattice
 *   lining_points[p][r]  the site points g with near(g, j) for at least one receptor atom j of residue r; lining_residues[p] the
 *                        number of residues with a count above 0
 *   ok[p]                0: a non-finite coordinate in an atom of class != 0, or a non-finite centre (a ligand without an active atom
 *                        has one).  Then every count is 0, every float NaN (centre_used too), classes, buried, atom_class and
 *                        atom_buried are 255 and truncated is 0.
 * ws: pd_pocket_grid_workspace_numel(P, n, A) = P (2 n^3 + 2 n^2 ceil(n / 32)) ints (labels, marks and the two bit masks; negative:
 * the error code).  Four launches, no allocation, no synchronisation, no floating-point atomics; "any" tests and integer sums only:
 * bit-identical from launch to launch, independent of P and of a pose's place among the P.  PD_ERR_ARG: a required pointer is NULL
 * (centre may be; res_atom when N == 0) or an int / float pointer is off its 4-byte alignment, a size < 1 (N >= 0, N <= A), h not
 * positive and finite, probe or lining negative or not finite, a negative step count, min_enclosed outside 0 .. 7, a centre_stride other
 * than 0 or 3, a short workspace.  PD_ERR_UNSUPPORTED: n outside PD_POCKET_MIN_N .. PD_POCKET_MAX_N, L > 1024, R > 4096, P > 65535, A >
 * 2^22, h (n - 1) > 4096 A.  A rejected call launches nothing.                                                                       */
#define PD_POCKET_MIN_N 8
#define PD_POCKET_MAX_N 48
#define PD_POCKET_COUNTS 8
#define PD_POCKET_VALUES 6
long long pd_pocket_grid_workspace_numel(int P, int n, int A);
int pd_pocket_grid(const float* x, const unsigned char* cls, const float* radius, const int* lig_idx, const int* res_start,
                   const int* res_atom, const float* centre, int centre_stride, int snap, float h, int n, float probe, float lining,
                   const int* steps, int min_enclosed, int* ws, long long ws_numel, float* centre_used, unsigned char* ok,
                   unsigned char* classes, unsigned char* buried, int* counts, unsigned char* truncated, float* values,
                   unsigned char* atom_class, unsigned char* atom_buried, int* lining_points, int* lining_residues, int P, int A, int L,
                   int R, int N, void* stream);
int pd_euler(const float* x_hat, const float* x_den, const float* x_proj, const float* w, float t_hat, float eta, float dt,
             float* x_next, int B, int A, void* stream);
int pd_timestep_embed(const float* tau, float* emb, int n, void* stream);
/* pd_dit_bounds (ABI 5; tightened in ABI 8): rigorous magnitude bounds of a DiT block's activations for the two-part fp16 operand
 * format, from the AdaLN table and the weights - no activation is looked at: tab [nrows][ld] holds per DiT block
 * (shift | 1 + scale | gate) x (attention, transition), C channels each; consts [nblocks][4] = (q bound, k bound, -, -);
 * wstack [nblocks][C + 2 hidden][C] = the block's (linear_v | w1 | w3) rows as its projections use them; vh [nrows][nblocks][2]
 * scratch.  out [nrows][nblocks][8] = (|q|, |k|, |v| = |o|, |y|, |y'|, |h|, 0, 0) upper bounds.  ABI 8: |v| and |h| are per-output-row
 * Cauchy-Schwarz bounds with the step's own modulation inside the norm (sqrt(C) ||W_n o (1 + scale)||_2 + |W_n . shift|), maximised
 * over n - a large AdaLN gain or weight row no longer loosens the bound of every channel (csrc/sampler.hip for the derivation;
 * reference adaptive_layer_norm_zero.py:16-21, attentions.py:241-265, transitions.py:27-30).                                     */
int pd_dit_bounds(const float* tab, int nrows, int ld, int nblocks, int C, int hidden, const float* consts, const float* wstack,
                  float* vh, float* out, void* stream);
/* chirality accept / reject of B poses without leaving the device (replaces the per-pose RDKit rebuild + R/S comparison of
 * redocking.py:264-281,303-317): centres[nc][4] = (centre atom, three neighbour atoms), indices into the A atoms of a pose;
 * sign of the signed volume (n1-c).((n2-c)x(n3-c)) vs ref_sign[nc] (+1 / -1); accept[b] = 1 iff every centre matches.
 * sign_out [B][nc] (optional) returns the signs themselves (used once, on the reference coordinates, to make ref_sign).   */
int pd_chirality(const float* x, const int* centres, const int* ref_sign, int* accept, int* sign_out, int B, int A,
                 int n_centres, void* stream);
/* ligand rows of a pose batch, for the relaxation branch (model.py:252-257):
 * pd_ligand_gather : lig[b,l,:] = x[b, lig_idx[l], :]                      (`x_denoised[:, is_ligand_atom]`)
 * pd_ligand_scatter: dst = src with dst[b,a,:] = lig[b, atom_slot[a], :] where atom_slot[a] >= 0
 *                    (`x_ref = deepcopy(x_denoised); x_ref[:, is_ligand_atom] = relaxed`); atom_slot[A] = ligand slot or -1 */
int pd_ligand_gather(const float* x, const int* lig_idx, float* lig, int B, int A, int L, void* stream);
int pd_ligand_scatter(float* dst, const float* src, const float* lig, const int* atom_slot, int B, int A, int L, void* stream);

/* ---- MMFF94 ligand relaxation on the device (mmff.hip) ----------------------------------------
 * replaces the host loop `get_next_step_pos` (models/model.py:26-52): per sample
 * AllChem.MMFFOptimizeMolecule(ref_mol, mmffVariant="MMFF94", maxIters=mmff_iters, ignoreInterfragInteractions=True)
 * (RDKit: ForceField::minimize -> BFGSOpt::minimize over the MMFF94 contribs).  The molecule arrives as plain term
 * tables (device pointers; int32 atom indices into the ligand, float64 parameters):
 *   bond   [n][2] i,j      | kb, r0
 *   angle  [n][3] i,j,k    | ka, theta0 (deg), linear flag (0/1)            j = central atom
 *   strbnd [n][3] i,j,k    | kbaIJK, kbaKJI, r0_ij, r0_kj, theta0
 *   oop    [n][4] i,j,k,l  | koop                                            j central, l the out-of-plane atom
 *   tors   [n][4] i,j,k,l  | V1, V2, V3
 *   vdw_R / vdw_eps / ele_qq [L][L] symmetric dense pair tables: R*_ij, eps_ij (0: pair excluded), q_i q_j / D with the
 *                            0.75 1-4 factor folded in (0: excluded)
 *   inc_ptr [L+1], inc: atom -> incident bonded terms (CSR); entry = kind << 28 | slot << 24 | term index,
 *                       kind 0..4 in the order above, slot = position of the atom in the term's index row          */
typedef struct pd_mmff_terms {
    int n_atoms, n_bond, n_angle, n_strbnd, n_oop, n_tors;
    const int* bond_idx;   const double* bond_par;
    const int* angle_idx;  const double* angle_par;
    const int* strbnd_idx; const double* strbnd_par;
    const int* oop_idx;    const double* oop_par;
    const int* tors_idx;   const double* tors_par;
    const double* vdw_R;   const double* vdw_eps;  const double* ele_qq;
    const int* inc_ptr;    const int* inc;
} pd_mmff_terms;
/* energy[b] (kcal/mol) and grad[b][L][3] of B conformations pos[b][L][3] (float64; either output may be NULL) */
int pd_mmff_energy_grad(const pd_mmff_terms* terms, const double* pos, double* energy, double* grad, int B, void* stream);
/* x_ref = x [B][A][3] with the rows lig_idx[0..L) replaced by their relaxed coordinates (`x_ref = deepcopy(x_denoised);
 * x_ref[:, is_ligand_atom] = get_next_step_pos(...)`, model.py:253-255); max_iters = mmff_iters.
 * ws: B * (9 L^2 + 24 L) float64 of scratch (inverse Hessian + BFGS vectors per sample)                            */
int pd_mmff_relax(const pd_mmff_terms* terms, const float* x, const int* lig_idx, float* x_ref, double* ws,
                  long long ws_doubles, int B, int A, int max_iters, void* stream);

/* ---- loss terms of the training-time forward (loss.hip; ABI 11) -----------------------------
 * The five terms of PhysDockLoss (models/loss.py:576-625), fp32 in, one fp32 scalar out per term (gradients: next block).  No [B,A,A],
 * [B,T,T] or [T,T,bins] intermediate is written: pairs are formed in registers and reduced per block into `ws`, a second pass
 * adds the partial sums in a fixed order in float64 (the same bits on every call, no floating-point atomics).
 * `ws` holds at least pd_loss_workspace_numel(B, A, T) floats (= max(n (n + 1) / 2 * (B + 1) with n = ceil(A / 64), 2 T B,
 * 2 ceil(T^2 / 256), B)); the launchers may share it when they run on one stream.  Index arrays are int64 (torch.long).
 * pd_loss_smooth_lddt  : smooth_lddt_loss (loss.py:162-181)   mean_b sum_ij m_ij eps(|d_pred - d_gt|) / (1e-9 + sum m_ij),
 *                        m_ij = (d_gt < max_clamp_distance) exists_i exists_j, eps(d) = 1/4 sum_c sigmoid(d - c), c = .5, 1, 2, 4
 * pd_loss_centre_pairs : bond_loss (loss.py:245-318) -> out[0] and key_res_loss (loss.py:535-559) -> out[1] in one pass over the
 *                        centre-atom pairs: mean_b scale_b(sigma) * mean_b sum_ij mask_ij f(diff_ij) / (sum mask + eps)
 * pd_loss_distogram    : distogram_loss (loss.py:78-115); boundaries_sq = linspace(min_bin, max_bin, no_bins - 1) ** 2 from the
 *                        host (the reference's own expression); no_bins <= 63
 * pd_loss_weighted_mse : weighted_mse_loss (loss.py:118-159) after the alignment: x_gt_aligned [B,A,3] is the output of
 *                        pd_kabsch_align(x_denoised, x_exists, x_gt, 0, weights).  As the reference computes it: sigma_data = 16
 *                        whatever the configuration says, scale (t^2 + 16^2) / (16 t)^2 / 3, clamped at 10000               */
int pd_loss_workspace_numel(int B, int A, int T);
int pd_loss_smooth_lddt(const float* x_denoised, const float* x_gt, const float* x_exists, float max_clamp_distance, float* ws,
                        float* out, int B, int A, void* stream);
int pd_loss_centre_pairs(const float* x_denoised, const float* x_gt, const long long* token_id_to_centre_atom_id,
                         const float* token_bonds, const float* is_key_res, const float* is_ligand, const float* t_hat,
                         float sigma_data_bond, float sigma_data_key, float eps, float* ws, float* out, int B, int A, int T,
                         void* stream);
int pd_loss_distogram(const float* p_distogram, const float* x_gt, const float* x_exists,
                      const long long* token_id_to_pseudo_beta_atom_id, const float* boundaries_sq, int no_bins, float* ws,
                      float* out, int A, int T, void* stream);
int pd_loss_weighted_mse(const float* x_denoised, const float* x_gt_aligned, const float* weights, const float* t_hat, float* ws,
                         float* out, int B, int A, void* stream);

/* ---- gradients of the loss terms (loss_grad.hip; additive exports of ABI 11) ----------------
 * d term / d x_denoised [B,A,3] and d distogram_loss / d p_distogram [T,T,no_bins], as torch autograd gives them for the
 * reference's code: |.| has derivative 0 at 0, a zero distance a zero direction, torch.clamp blocks the weighted MSE above 1e4.
 * Same rules as the forward block: no pair tensor, ordered reductions, no floating-point atomics, no allocation or host read.
 * `scale` is a DEVICE pointer to the upstream factor (term weight x upstream gradient x finite flag); a zero scale writes / adds
 * an exact 0 (never 0 * NaN).  accumulate = 0 writes g_x, 1 adds to it.  `ws` holds at least pd_loss_grad_workspace_numel(B, A, T)
 * floats (= max(3 B A + ceil(A / 64), 4 + 3 B T, B + 1)); it is not shared with a forward launch still reading its own.
 * pd_loss_weighted_mse_grad : 2 w_a (x_denoised - x_gt_aligned) mean_b scale_b(16) / (3 (1e-9 + B sum w)) x scale[0]
 * pd_loss_smooth_lddt_grad  : full-row sweep, (1 / B) / (1e-9 + sum m) sum_j 2 m_ij eps'(delta) sign(delta) (x_i - x_j) / d_ij
 * pd_loss_centre_pairs_grad : scale[0] x bond_loss + scale[1] x key_res_loss (both orientations of each mask), added per
 *                             centre atom in token order (two tokens may name one atom); accumulate = 0 zeroes g_x first
 * pd_loss_distogram_grad    : g_p = scale m^3 (softmax(m p) - onehot(bin)) / (1e-9 + sum m), m = exists_i exists_j (written) */
int pd_loss_grad_workspace_numel(int B, int A, int T);
int pd_loss_weighted_mse_grad(const float* x_denoised, const float* x_gt_aligned, const float* weights, const float* t_hat,
                              const float* scale, float* ws, float* g_x, int B, int A, int accumulate, void* stream);
int pd_loss_smooth_lddt_grad(const float* x_denoised, const float* x_gt, const float* x_exists, float max_clamp_distance,
                             const float* scale, float* ws, float* g_x, int B, int A, int accumulate, void* stream);
int pd_loss_centre_pairs_grad(const float* x_denoised, const float* x_gt, const long long* token_id_to_centre_atom_id,
                              const float* token_bonds, const float* is_key_res, const float* is_ligand, const float* t_hat,
                              float sigma_data_bond, float sigma_data_key, float eps, const float* scale, float* ws, float* g_x,
                              int B, int A, int T, int accumulate, void* stream);
int pd_loss_distogram_grad(const float* p_distogram, const float* x_gt, const float* x_exists,
                           const long long* token_id_to_pseudo_beta_atom_id, const float* boundaries_sq, int no_bins,
                           const float* scale, float* ws, float* g_p, int A, int T, void* stream);

/* ---- confidence losses (confidence_loss.hip; additive exports of ABI 11) ---------------------
 * cal_lddt, the token frames and the pLDDT / PDE / PAE losses (models/loss.py:184-207,320-532) with the gradient of each loss to
 * its logits.  Same rules as the two blocks above: fp32, no [A,T], [T,T] or one-hot tensor, ordered reductions, no allocation or
 * host read.  Every target is a hard bin: divisions that feed a bin index are IEEE, so lDDT (a ratio of two exact sums) and the
 * bins equal the reference's wherever no distance sits on a threshold.  Only pose 0 enters the three losses.
 * `ws` holds at least pd_conf_loss_workspace_numel(B, A, T) floats (= 4 + ceil(max(A, T^2) / 64)); the loss launchers may share it
 * on one stream.  g (nullable) is OVERWRITTEN with scale[0] m^3 (softmax(m p) - onehot(bin)) / (1e-9 + sum m); `scale` is a DEVICE
 * pointer (needed only with g); a zero scale or a masked row writes exact zeros.  no_bins <= 64.
 * pd_lddt_atoms      : lddt [B,A] of x_pred [B,A,3] against x_gt over the T token centres; an empty inclusion set gives NaN
 * pd_conf_frames     : frames [T,13] = e1 | e2 | e3 | origin | (cos theta < 0.906308) of x [A,3] (a pose or x_gt)
 * pd_conf_loss_plddt : rows = atoms, m = x_exists, bin = clamp(long(lddt no_bins)) (NaN -> 0); lddt [A] is that of pose 0
 * pd_conf_loss_pairs : rows = token pairs, m = exists_ci exists_cj, bin = clamp(long((e - min_bin) / bin_range no_bins));
 *                      mode 0 (PDE) e = |d_pred - d_gt| of the centres, mode 1 (PAE) e = |R_i^pred (c_j - b_i)^pred -
 *                      R_i^gt (c_j - b_i)^gt| valid_i^gt valid_i^pred (frames of pd_conf_frames; unused and nullable in mode 0) */
int pd_conf_loss_workspace_numel(int B, int A, int T);
int pd_lddt_atoms(const float* x_pred, const float* x_gt, const long long* token_id_to_centre_atom_id, const float* is_dna,
                  const float* is_rna, const float* is_polymer, float* lddt, int B, int A, int T, void* stream);
int pd_conf_frames(const float* x, const long long* frame_atom_0, const long long* frame_atom_1, const long long* frame_atom_2,
                   float* frames, int A, int T, void* stream);
int pd_conf_loss_plddt(const float* p_plddt, const float* lddt, const float* x_exists, int no_bins, const float* scale, float* ws,
                       float* out, float* g_plddt, int A, void* stream);
int pd_conf_loss_pairs(int mode, const float* p_pair, const float* x_pred0, const float* x_gt, const float* x_exists,
                       const long long* token_id_to_centre_atom_id, const float* frames_pred, const float* frames_gt,
                       float min_bin, float bin_range, int no_bins, const float* scale, float* ws, float* out, float* g_pair,
                       int A, int T, void* stream);

/* ---- confidence metrics (metrics.hip; additive exports of ABI 11) ------------------------------
 * The inference-time scores of data/tools/get_metrics.py from the logits of ConfidenceModule, for P stacked logit sets and B poses
 * per call.  fp32; the logits are read once; ordered reductions (two calls give the same bits, and so do two bit-identical
 * rows, for any P), no floating-point atomics, no allocation or host read.  no_bins <= 64 (else PD_ERR_UNSUPPORTED).
 * pd_metrics_plddt  : atom_plddts [P,A] = 100 sum_k softmax(p_plddt [P,A,no_bins])_k (k + 0.5) / no_bins; mean_plddt [P] = the
 *                     plain mean over all A atoms (no mask, as in the reference)
 * pd_metrics_pae_tm : one pass over p_pae [P,T,T,no_bins].  `centres` [no_bins] is a DEVICE table of the bin centres, `weights`
 *                     [T] the residue weights w (s_mask, may be fractional), asym_id [T] int32 (nullable: ipTM = 0, row 0).
 *                     pae [P,T,T] (nullable) = sum_k prob_k centre_k.  With tm_ij = sum_k prob_k / (1 + centre_k^2 / d0^2),
 *                     d0 = 1.24 (max(int(sum w), 19) - 15)^(1/3) - 1.8 formed on the device, and for the pair masks m = 1 (pTM)
 *                     and m = asym_i != asym_j (ipTM): per_alignment_i = sum_j tm_ij m_ij w_i w_j / (1e-8 + sum_j m_ij w_i w_j);
 *                     ptm / iptm [P] = per_alignment at the FIRST maximal row of per_alignment_i w_i, rows [P,2] int32 that row
 *                     (pTM, ipTM), per_alignment [P,2,T] (nullable) all rows.  `ws` holds at least
 *                     pd_metrics_workspace_numel(P, T) floats (= 64 + 2 P T ceil(T / 16)).  P <= 65535.
 * pd_metrics_clash  : get_has_clash per pose of x_pred [B,A,3] over the atoms with a_mask == 1 and polymer != 0 ([A] floats);
 *                     chain [A] int32 is the dense chain index 0 .. n_chain - 1 in ascending asym_id order, n_chain <= 64.
 *                     counts [B,n_chain,n_chain] int32 (workspace, overwritten) = ordered atom pairs closer than 1.1 per chain
 *                     pair.  has_clash [B] int64 = 1 if n > 100 or 2 n > min(N_a, N_c) for a chain pair of the reference's
 *                     loop (a over all but the last, c over all but the first chain with eligible atoms, which pairs a middle
 *                     chain with itself) or, with skip_self_pairs, of a < c.  ranking [B] (nullable) = 0.8 iptm + 0.2 ptm -
 *                     has_clash with (i)ptm read at b * tm_stride (tm_stride 0 or 1).  B <= 65535, A <= 46340. */
int pd_metrics_workspace_numel(int P, int T);
int pd_metrics_plddt(const float* p_plddt, float* atom_plddts, float* mean_plddt, int P, int A, int no_bins, void* stream);
int pd_metrics_pae_tm(const float* p_pae, const float* centres, const float* weights, const int* asym_id, float* ws, float* pae,
                      float* ptm, float* iptm, int* rows, float* per_alignment, int P, int T, int no_bins, void* stream);
int pd_metrics_clash(const float* x_pred, const float* a_mask, const int* chain, const float* polymer, int* counts,
                     const float* ptm, const float* iptm, int tm_stride, long long* has_clash, float* ranking, int B, int A,
                     int n_chain, int skip_self_pairs, void* stream);

/* ---- Gaussian shape and feature overlap (shape_overlap.hip; additive exports of ABI 11) -----------------------------
 * First-order Gaussian overlap (Grant, Gallardo & Pickup 1996) of molecules that need no atom correspondence; float64 from the fp32
 * coordinates, ordered sums, no atomics: bit-identical from launch to launch and whatever else is in the batch.
 * tests/shape_overlap_ref.py is the written definition.  A "side" is n structures of one molecule: L named atoms with the exponents
 * alpha [L] (DEVICE doubles, kappa / R_i^2) and F features in CSR form (feat_start [F+1], feat_atom: indices 0 .. L-1 into the named
 * atoms, feat_kind [F] in 0 .. 5); features are Gaussians of the exponent color_alpha.  The caller guarantees every index is inside
 * its array (physdock_amd/shape.py checks them on the host).  L, F <= 1024, n <= 65535 per side, A <= 2^22.
 * pd_shape_prepare : ws (pd_shape_workspace_numel(n, L, F) = n (3 L + 3 F + 2) doubles) = per structure the atoms [L][3], the
 *                    feature points [F][3] (the mean of the members) and (O_AA, C_AA); both NaN when a named atom is not finite.
 * pd_shape_overlap : sides a (rows) and b (columns) as prepared, with the lengths of their workspaces.  o_ab, c_ab double [n,C],
 *                    shape_tanimoto, color_tanimoto, combo float [n,C]; atom_share double [n,L] (C == 1 only): each row atom's part
 *                    of o_ab.  Every output may be NULL.  pairwise != 0 needs the same side twice: the columns >= row are computed and
 *                    mirrored.  A NaN structure gives NaN in its whole row / column.
 * pd_shape_overlay : L, M <= 256.  Maximises O(move(A, s), B) over rigid motions from five starts (principal axes aligned and turned
 *                    by 180 degrees about none, the first, second, third axis; the pose as it stands) with the minimiser of
 *                    pd_vina_refine at zero torsions.  ws: pd_shape_overlay_workspace_numel(n, C, L) = 5 n C (16 + 3 L) doubles.  Per
 *                    (row, column): transform double [7] = the unit quaternion (w, x, y, z), w >= 0, and t with x' = R x + t;
 *                    x_fit double [L][3] (nullable) = the row's atoms as the minimiser left them; scores float [3]
 *                    (shape, colour, combo at the optimum); overlap, overlap_start (in place) double; best_start, iterations,
 *                    evaluations, status (0 converged / 1 max_iters / 2 line search) int32 of the winning start.
 * PD_ERR_ARG / PD_ERR_UNSUPPORTED before anything is launched for NULL required pointers, sizes out of range or a short workspace. */
long long pd_shape_workspace_numel(int n, int L, int F);
int pd_shape_prepare(const float* x, const int* lig_idx, const double* alpha, const int* feat_start, const int* feat_atom,
                     const int* feat_kind, double color_alpha, double* ws, long long ws_numel, int n, int A, int L, int F, void* stream);
int pd_shape_overlap(const double* ws_a, long long ws_a_numel, const double* alpha_a, const int* kind_a, int n, int L, int Fa,
                     const double* ws_b, long long ws_b_numel, const double* alpha_b, const int* kind_b, int C, int M, int Fb,
                     double color_alpha, int pairwise, double* o_ab, double* c_ab, float* shape_tanimoto, float* color_tanimoto,
                     float* combo, double* atom_share, void* stream);
long long pd_shape_overlay_workspace_numel(int n, int C, int L);
int pd_shape_overlay(const double* ws_a, long long ws_a_numel, const double* alpha_a, const int* kind_a, int n, int L, int Fa,
                     const double* ws_b, long long ws_b_numel, const double* alpha_b, const int* kind_b, int C, int M, int Fb,
                     double color_alpha, int max_iters, double grad_tol, double max_step, double* ws, long long ws_numel,
                     double* transform, double* x_fit, float* scores, double* overlap, double* overlap_start, int* best_start, int* iterations,
                     int* evaluations, int* status, void* stream);

/* ---- Torsion fingerprint and torsion-fingerprint deviation TFD (torsion.hip; additive exports of ABI 11) --------------
 * The ligand's torsion angles per pose and the TFD between poses (after Schulz-Gasch, Schaerfer, Guba & Rarey 2012; the package's own
 * definition: tests/torsion_ref.py and physdock_amd/torsions.py, which builds the tables).  Float64 from the fp32 coordinates, fixed
 * order sums, an exact minimum over the table rows, no atomics: a value depends on its own structures and the tables alone and is
 * bit-identical whatever the batch.  Tables (all on the DEVICE): quads int32 [Q][4], the Q distinct quadruples of ligand atoms
 * 0 .. L-1 (the closure of the base quadruples under the symmetry table; a quadruple and its reverse are one); the fingerprint's T
 * entries as qstart int32 [T+1] (entry t owns the base quadruples qstart[t] .. qstart[t+1]-1 of Nq), w double [T] (weights >= 0 with a
 * positive sum) and inv_max_dev double [T] (1 / max_dev in 1 / degree); image uint16 [Nq][M], m fastest: the id in 0 .. Q-1 of base
 * quadruple qb seen through table row m, image[qb][0] its own id.  The caller guarantees that every index lies inside its array; one
 * that does not is never followed and counts as an angle that does not exist (NaN).
 * pd_torsion_prepare   : x fp32 [n][A][3] gathered through lig_idx int32 [L] (NULL: atoms 0 .. L-1, needs A >= L) -> ws double [n][Q]
 *                        (pd_torsion_workspace_numel(n, Q) = n Q), the IUPAC dihedral of each quadruple in degrees,
 *                        atan2(|b2| b1.(b2 x b3), (b1 x b2).(b2 x b3)) 180 / pi; NaN when a coordinate is not finite or
 *                        |b1 x b2|^2 <= 1e-12 |b1|^2 |b2|^2 (or the same on the other side).  angles_deg (nullable, float [n][Nq]; needs
 *                        image): the angle of every base quadruple rounded once to fp32.
 * pd_torsion_tfd       : rows ws_a [na][Q] against columns ws_b [nb][Q] as prepared.  dev_t = min(1, mean over the entry's quadruples
 *                        of the circular distance of the row's angle at image[qb][0] and the column's at image[qb][m], times
 *                        inv_max_dev[t]); TFD(m) = sum_t w_t dev_t / sum_t w_t, NaN when an angle it names is; D float [na][nb] = the
 *                        float64 min over m rounded once (a NaN never wins; NaN when every m is NaN; exactly 0 when T = 0, where the
 *                        workspaces and tables may be NULL), best_perm (nullable, int32 [na][nb]) the smallest m that attains it or -1.
 *                        symmetric != 0 covers ws_b == ws_a (NULL or ws_a, nb == na): i < j is computed (row i fixed, row j permuted)
 *                        and mirrored, the diagonal is an exact 0, or NaN for a structure one of whose own angles is NaN; best_perm
 *                        must then be NULL.  One 256-thread block per (row, tile of TJ columns), the angles in LDS: TJ = 64 (M <= 4),
 *                        16 (M <= 16), 4 (M <= 64) or 1, quartered until (TJ + 1) (Q | 1) doubles fit 65280 bytes (64 up to Q = 125,
 *                        16 up to 479, 4 up to 1631, 1 up to 4079; for Q = 4080 .. 4096 TJ = 1 and the row stays in global memory).
 * pd_torsion_deviation : rows ws_a [na][Q] against ONE prepared reference ws_ref [Q] at table row rows[i] (int32 [na]; NULL: row 0)
 *                        -> dev float [na][T], the dev_t above: which bond is wrong.  NaN for an entry that names a NaN angle and for
 *                        a row outside 0 .. M-1 (the -1 of best_perm).  T = 0 writes nothing.
 * L <= 1024, T <= 1024, Q <= 4096, Nq <= 9216, M <= 65535, 65535 structures per side: else PD_ERR_UNSUPPORTED.  A NULL required
 * pointer, a misaligned pointer, a size < 1 or a short workspace: PD_ERR_ARG.  A rejected call launches nothing.                    */
int pd_torsion_workspace_numel(int n, int Q);
int pd_torsion_prepare(const float* x, const int* lig_idx, const int* quads, const unsigned short* image, double* ws, long long ws_numel,
                       float* angles_deg, int n, int A, int L, int Q, int Nq, int M, void* stream);
int pd_torsion_tfd(const double* ws_a, const double* ws_b, const int* qstart, const double* w, const double* inv_max_dev,
                   const unsigned short* image, float* D, int* best_perm, int na, int nb, int Q, int T, int Nq, int M, int symmetric,
                   void* stream);
int pd_torsion_deviation(const double* ws_a, const double* ws_ref, const int* rows, const int* qstart, const double* inv_max_dev,
                         const unsigned short* image, float* dev, int na, int Q, int T, int Nq, int M, void* stream);

/* ---- Poses against the trunk's own distogram (distogram_score.hip; additive exports of ABI 11) -------------------------
 * How well does a pose agree with the distances the trunk predicted?  logits fp32 [T][T][no_bins] (PhysDock.predict_distogram) over
 * the pseudo-beta distance of two tokens; the package's own definition: tests/distogram_score_ref.py and physdock_amd/distogram.py,
 * which builds the tables.  Agreement with the trunk is self-consistency, not accuracy, and the defaults of the Python class (contact
 * cutoff, cap on the expected distance, classes) have not been validated.  Float64 from the fp32 inputs, fixed-order sums, no atomics:
 * a pose's values are bit-identical whatever the batch.  Tables on the DEVICE: token_class uint8 [T] (0 inactive, 1 receptor, 2
 * ligand), pb_atom int32 [T] (the pseudo-beta atom of an active token, inside 0 .. A-1), rows int32 [n_rows] (the n_ligand_rows ligand
 * tokens ascending, then - with the receptor class - the n_receptor_tokens receptor tokens ascending), row_of int32 [T] (a ligand
 * token's place in rows).  The caller guarantees that every index lies inside its array.  On the HOST, float64: centres [no_bins] and
 * bounds_sq [no_bins - 1] (the squared bin edges).  contact_bin: the last bin that counts as a contact, -1 for none.
 * pd_distogram_tables    : per token pair lse = log sum exp of its logits (double [T][T]), expected = sum_b softmax_b centres[b] and
 *                          p_contact = sum_{b <= contact_bin} softmax_b (float [T][T], rounded once).
 * pd_distogram_score     : x fp32 [P][A][3].  bin = #{k : d2 > bounds_sq[k]} of every pair of a row, nll = lse - logit[bin].  bins uint8
 *                          [P][n_ligand_rows][T] (255 in the column of an inactive token) and ws double [P][n_rows][8]: per row the sum
 *                          of nll over its interface pairs (a receptor row: over its receptor pairs j > i), over its ligand pairs
 *                          j > i, of |d - expected| where expected <= max_expected, of p_contact over the pairs in contact, and the
 *                          counts of the third, of p_contact >= 0.5, of those in contact, of all in contact.
 * pd_distogram_reduce    : values float [7][P] = nll_interface, nll_ligand, nll_receptor, nll, expected_error, contact_recovery,
 *                          contact_precision (NaN where nothing is counted); token_nll float [P][T] (the mean interface nll of a token
 *                          against the other side, NaN without a partner), n_contacts int32 [P], ok uint8 [P]: a pose with a non-finite
 *                          coordinate at an active pseudo-beta atom has ok = 0, NaN floats, n_contacts 0 and zeroed bins.
 * pd_distogram_potential : V(d) = the linear interpolation of lse - logit over the centres, constant outside them.  potential float
 *                          [P] = its mean over the interface and the ligand pairs; forces float [P][n_ligand_rows][3] = minus the
 *                          gradient on each ligand token's pseudo-beta atom and abs_force float [P][n_ligand_rows] = the sum of the
 *                          absolute values of the contributions (both or neither NULL).  ws double [P][n_ligand_rows][5].
 * 2 <= no_bins <= 64, T <= 4096, P <= 65535: else PD_ERR_UNSUPPORTED.  A NULL required pointer, a misaligned pointer, a size < 1, a
 * short workspace or a non-finite centre / bound: PD_ERR_ARG.  A rejected call launches nothing.                                    */
#define PD_DISTOGRAM_MAX_BINS 64
#define PD_DISTOGRAM_MAX_TOKENS 4096
#define PD_DISTOGRAM_ROW_PARTIALS 8
#define PD_DISTOGRAM_POTENTIAL_PARTIALS 5
#define PD_DISTOGRAM_VALUES 7
int pd_distogram_tables(const float* logits, const double* centres, int contact_bin, double* lse, float* expected, float* p_contact,
                        int T, int no_bins, void* stream);
int pd_distogram_score(const float* x, const int* pb_atom, const unsigned char* token_class, const int* rows, const float* logits,
                       const double* lse, const float* expected, const float* p_contact, const double* bounds_sq, int contact_bin,
                       float max_expected, unsigned char* bins, double* ws, long long ws_numel, int P, int A, int T, int no_bins,
                       int n_ligand_rows, int n_rows, void* stream);
int pd_distogram_reduce(const float* x, const int* pb_atom, const unsigned char* token_class, const int* rows, const int* row_of,
                        const float* logits, const double* lse, unsigned char* bins, const double* ws, long long ws_numel,
                        float* values, float* token_nll, int* n_contacts, unsigned char* ok, int P, int A, int T, int no_bins,
                        int n_ligand_rows, int n_receptor_tokens, int n_rows, void* stream);
int pd_distogram_potential(const float* x, const int* pb_atom, const unsigned char* token_class, const int* rows, const float* logits,
                           const double* lse, const double* centres, double* ws, long long ws_numel, float* potential, float* forces,
                           float* abs_force, int P, int A, int T, int no_bins, int n_ligand_rows, int n_receptor_tokens, void* stream);

/* ---- lDDT of the ligand pocket and pocket RMSDs (pocket_accuracy.hip; additive exports of ABI 11) ----------------------------
 * Did the model draw the right pocket?  x fp32 [P][A][3] against one ground truth; the package's own definition (not OpenStructure's
 * bytes): tests/pocket_accuracy_ref.py and physdock_amd/pocket_accuracy.py, which builds the tables.  Float64 from the fp32
 * coordinates, integer counts, fixed-order sums, no atomics: a pose's values are bit-identical whatever the batch.  Tables on the
 * DEVICE: the Np pocket atoms by (pocket residue, atom) as patom int32 [Np] (pose atom), patom_partner int32 [Np] (the pose atom whose
 * name it may exchange with; itself for none), patom_kind uint8 [Np] (bit 0: CA, bit 1: N / CA / C / O), patom_ref double [Np][3] (the
 * reference coordinates); res_atom_start int32 [Rp+1] (the pocket atoms of each of the Rp pocket residues); the pairs in CSR form over
 * the pocket atoms, pair_start int32 [Np+1], pair_atom int32 (pose atom, ascending per row), pair_dist double; atom_partner int32 [A]
 * (as patom_partner, per pose atom) and atom_slot int32 [A] (the pocket residue 0 .. Rp-1 of a pose atom, -1 outside the pocket);
 * named int32 [n_named], every pose atom a table names, ascending.  The caller guarantees that every index lies inside its array.
 * pd_pocket_accuracy : a pair is conserved at t when | |p_i - p_j| - pair_dist | < thr_t.  Per pocket residue with partners the
 *                      conserved (pair, threshold) entries of its rows are counted as given and with its partners exchanged in the
 *                      pose; swapped int32 [P][Rp] = 1 where the second count is strictly greater.  Then, with all chosen exchanges
 *                      applied on both sides of every pair: conserved int32 [P][4], lddt_lp float [P] = sum conserved / (4 n_pairs),
 *                      residue_lddt float [P][Rp] (both 0 without pairs).  Fit: Horn's quaternion (proper rotations only) of the pose's
 *                      CA atoms on the reference's: quat double [P][4] (w, x, y, z; first non-zero component positive) and t double
 *                      [P][3] with ref ~ R(quat) x + t; rmsd float [P][3] = CA, backbone and all pocket atoms under that transform,
 *                      residue_rmsd float [P][Rp]; exchanges applied.  fit_ok uint8 [P] = 0 with NaN RMSDs and transform for fewer than
 *                      3 CA atoms or a CA set (either side) whose scatter matrix has its middle eigenvalue <= 1e-8 of the largest.
 *                      ok uint8 [P] = 0 for a non-finite coordinate at a named atom: NaN floats, zero integers, fit_ok 0.
 *                      ws: pd_pocket_accuracy_workspace_numel(P, Rp) = 4 P Rp ints, 16-byte aligned.  A row of pairs is walked
 *                      PD_POCKET_ACCURACY_TILE at a time.
 * A <= 4096, Rp <= 1024, P <= 65535: else PD_ERR_UNSUPPORTED.  A NULL required pointer (pair_atom / pair_dist may be NULL when
 * n_pairs == 0), a misaligned pointer, a size < 1, Rp > Np, n_named < Np, Np or n_named > A, a threshold <= 0 or a short workspace:
 * PD_ERR_ARG.  A rejected call launches nothing.                                                                                   */
#define PD_POCKET_ACCURACY_MAX_ATOMS 4096
#define PD_POCKET_ACCURACY_MAX_RESIDUES 1024
#define PD_POCKET_ACCURACY_TILE 256
int pd_pocket_accuracy_workspace_numel(int P, int Rp);
int pd_pocket_accuracy(const float* x, const int* patom, const int* patom_partner, const unsigned char* patom_kind,
                       const double* patom_ref, const int* res_atom_start, const int* pair_start, const int* pair_atom,
                       const double* pair_dist, const int* atom_partner, const int* atom_slot, const int* named, double thr0,
                       double thr1, double thr2, double thr3, int* ws, long long ws_numel, float* lddt_lp, float* residue_lddt,
                       int* conserved, int* swapped, float* rmsd, float* residue_rmsd, double* quat, double* t, unsigned char* ok,
                       unsigned char* fit_ok, int P, int A, int Np, int Rp, int n_pairs, int n_named, void* stream);

/* ---- ligand features from the molecular graph (ligand_features.hip; additive export of ABI 11) ---------------------------------
 * From a library of G ligand graphs to the reference's ligand feature blocks in one launch (the reference: RDKit on the host,
 * PhysDock/data/tools/rdkit.py get_features_from_ref_mol and feature_loader.py:327-352).  The package's own definition, not RDKit's
 * bytes: tests/ligand_features_ref.py and physdock_amd/ligand.py, which builds the tables.  Tables on the DEVICE, CSR over the
 * ligands: atom_start, bond_start int32 [G+1], pair_start int64 [G+1] (prefix sums of L^2); atoms int32 [n_atoms][4] = (atomic number,
 * formal charge, hydrogen count, flags: bit 0 written aromatic, bits 1-2 chirality 0 none / 1 @ / 2 @@); bonds int32 [n_bonds][4] =
 * (i, j local to the ligand, twice the bond order, 0).  Outputs: atom_table int8 [n_atoms][16] = ref_charge, ref_element (Z - 1),
 * ref_is_aromatic, ref_degree, ref_hybridization, ref_implicit_valence, ref_chirality, ref_in_ring_of_3 .. 8, then zeros; pair_table
 * int8 [n_pairs][8] = d_token, token_bonds, bond_type, bond_as_double, bond_in_ring, bond_is_conjugated, bond_is_aromatic, zero;
 * ref_feat float [n_atoms][167] (columns 0 .. 2, ref_pos, are written as zero) and rel_tok_feat float [n_pairs][42] in the reference's
 * column order.  One block per ligand, integers only, no atomics: a ligand's bits do not depend on the library around it.
 * Every ligand needs 1 <= L <= PD_LIGAND_FEATURES_MAX_ATOMS atoms and at most PD_LIGAND_FEATURES_MAX_BONDS bonds; one whose rows leave
 * the arrays is not written and a bond that leaves its ligand is skipped.  A NULL pointer (bonds may be NULL when n_bonds == 0), a
 * misaligned pointer, G < 1, n_atoms < G, n_pairs < n_atoms: PD_ERR_ARG; G > 65535 or sizes beyond G ligands of the largest size:
 * PD_ERR_UNSUPPORTED.  A rejected call launches nothing.                                                                          */
#define PD_LIGAND_FEATURES_MAX_ATOMS 128
#define PD_LIGAND_FEATURES_MAX_BONDS 512
int pd_ligand_features(const int* atom_start, const int* bond_start, const long long* pair_start, const int* atoms, const int* bonds,
                       signed char* atom_table, signed char* pair_table, float* ref_feat, float* rel_tok_feat, int G, int n_atoms,
                       int n_bonds, long long n_pairs, void* stream);

/* ---- aromaticity of ligand graphs (aromaticity.hip; additive export of ABI 11) -------------------------------------------------
 * Perceive aromatic rings in Kekule input, kekulise aromatic input, or both in turn, for a library of G ligands in one launch (the
 * reference: RDKit perceives on read).  The package's own definition, not RDKit's bytes: tests/aromaticity_ref.py.  The tables are
 * those of pd_ligand_features (atom_start, bond_start int32 [G+1], atoms int32 [n_atoms][4], bonds int32 [n_bonds][4]) and atoms_out,
 * bonds_out have the same layout, so they go straight into pd_ligand_features.  o2 is twice the bond order, 3 = aromatic; neighbours
 * are visited in ascending atom index.
 *   mode 0 kekulise: an atom NEEDS a double bond when it has a bond with o2 == 3, its element is in the organic subset (B C N O P S
 *     F Cl Br I with the normal valences 3; 4; 3, 5; 2; 3, 5; 2, 4, 6; 1) and, with used = (sum of o2 over its other bonds) / 2 +
 *     (number of its aromatic bonds) + hydrogen count + shift (shift = -charge for N, O, P, S, else |charge|), the smallest normal
 *     valence v >= used exists and v - used == 1.  The result is the lexicographically first perfect matching of the needing atoms
 *     over aromatic bonds: the lowest unmatched needing atom tries its unmatched needing aromatic neighbours in ascending order, each
 *     try one step, with backtracking.  Matched bonds get o2 = 4, every other aromatic bond 2, bit 0 of every atom's flags is cleared.
 *   mode 1 perceive: candidate rings are the chordless cycles of 5 .. 7 atoms; a bond is cyclic when it is no bridge.  An atom with a
 *     bond of o2 > 4 or more than one double bond contributes nothing; with one double bond 1 if that bond is cyclic, 0 if the atom is
 *     a carbon and the partner N, O or S, else nothing; without one 2 for N, P (charge 0, neighbours + hydrogens == 3), 2 for O, S, Se
 *     (charge 0, == 2), 2 for C (charge -1, == 3), 0 for C (charge +1) or B (charge 0) with == 3, else nothing.  A ring through an atom
 *     with a bond of o2 == 3 is skipped.  A ring is aromatic when all its atoms contribute and the sum is 4n + 2: its bonds get o2 = 3,
 *     its atoms flag bit 0; every other atom's bit 0 is cleared.  Rings are judged independently on the input orders.
 *   mode 2 normalise: kekulise, then perceive.
 * atoms_out: the input rows with bit 0 of the flags rewritten.  bonds_out: the input rows with column 2 rewritten and column 3 = bit 0
 * "in a perceived aromatic ring" | bit 1 "chosen double by the matching".  status int32 [G]: 0 done; 1 no matching exists; 2 a try
 * would have been step max_steps + 1; with 1 or 2 the ligand's rows are copied through unchanged.  counts int32 [G][4]: aromatic rings
 * found, aromatic atoms and aromatic bonds in the rows written, matching steps.  One block per ligand, integers only, no atomics: a
 * ligand's bits do not depend on the library around it.  Limits as for pd_ligand_features; a ligand whose rows leave the arrays is
 * not written (nor its status and counts) and a bond that leaves its ligand is copied through and otherwise skipped.  A NULL pointer
 * (bonds and bonds_out may be NULL when n_bonds == 0), an output that is its input, a misaligned pointer, n_ligands < 1, n_atoms <
 * n_ligands, a mode outside 0 .. 2, max_steps < 0: PD_ERR_ARG; n_ligands > 65535 or more atoms than that many ligands of the largest
 * size: PD_ERR_UNSUPPORTED.  A rejected call launches nothing.                                                                    */
int pd_aromaticity(const int* atom_start, const int* bond_start, const int* atoms, const int* bonds, int* atoms_out, int* bonds_out,
                   int* status, int* counts, int n_ligands, int n_atoms, int n_bonds, int mode, int max_steps, void* stream);

/* ---- double-bond stereo of every pose (bond_stereo.hip; additive export of ABI 11) ---------------------------------------------
 * Is each stated double bond cis or trans in the pose, and how far is it twisted?  (PoseBusters' double-bond stereo check; the
 * counterpart of pd_chirality.)  The package's own definition: tests/bond_stereo_ref.py.  x fp32 [n_poses][n_atoms][3]; quads int32
 * [n_entries][6] = (a, b, c, d, a2, d2), atom indices into the pose: b=c the double bond, a and a2 the substituents of b, d and d2
 * those of c, a2 / d2 = -1 for none; expect uint8 [n_entries] (1 cis, 2 trans) or NULL to label only; max_twist in degrees.
 *   dihedral fp32 [n_poses][n_entries]  the IUPAC dihedral a-b-c-d in degrees: b1 = b - a, b2 = c - b, b3 = d - c, m = b1 x b2, n = b2 x b3,
 *            phi = atan2(|b2| (b1 . n), m . n), in float64 from the fp32 coordinates, every product and sum rounded on its own, the
 *            result rounded once to fp32; NaN for a coordinate that is not finite or |m|^2, |n|^2 < 1e-12
 *   twist    fp32 [n_poses][n_entries]  min(|phi|, 180 - |phi|), the largest over the pairs (a, d), (a2, d), (a, d2), (a2, d2) that
 *            exist (so a pyramidal end shows), rounded once to fp32; NaN when one of them is not defined
 *   state    uint8 [n_poses][n_entries] 0 undefined (dihedral NaN), 1 cis (m . n > 0), 2 trans (m . n < 0), 3 perpendicular (== 0)
 *   per pose (each may be NULL): n_wrong int32 = entries with state != expect (without expect: undefined entries), n_twisted int32 =
 *            entries with twist > max_twist or NaN, max_twist_seen fp32 = the largest twist, NaN if any is NaN, ok int32 = n_wrong == 0
 * One launch, one 64-lane wave per pose, lane k takes entries k, k + 64, ...; integer sums and an exact maximum over fixed trees, no
 * atomics: the bits are the same from launch to launch and for a pose alone or in a batch.  An index outside [0, n_atoms) (other
 * than -1 for a2 / d2) makes its entry undefined and is not followed.  NULL x, quads, dihedral, twist or state, a count < 1, a
 * misaligned pointer, max_twist < 0 or NaN: PD_ERR_ARG; n_entries > 1024 or n_poses > 65535: PD_ERR_UNSUPPORTED.  A rejected call
 * launches nothing.                                                                                                               */
int pd_bond_stereo(const float* x, const int* quads, const unsigned char* expect, float max_twist, float* dihedral, float* twist,
                   unsigned char* state, int* n_wrong, int* n_twisted, float* max_twist_seen, int* ok, int n_poses, int n_atoms,
                   int n_entries, void* stream);

/* ---- circular fingerprints of ligand graphs and their comparison (fingerprint.hip; additive exports of ABI 11) -----------------
 * Which ligands of a library are near-duplicates, which are closest to a known binder, which diverse few should be docked first?
 * Morgan / ECFP-like fingerprints after Rogers & Hahn 2010 and Tanimoto similarity - the package's own definition, not RDKit's bytes:
 * tests/fingerprint_ref.py.  Hash arithmetic mod 2^32: fmix(h): h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >>
 * 16;  push(h, v) = fmix(h * 0x01000193 + v + 0x9E3779B9).
 *
 * pd_morgan_fingerprint: the tables of pd_ligand_features (atom_start, bond_start int32 [G+1], atoms int32 [n_atoms][4] = Z, charge,
 * h_count, flags; bonds int32 [n_bonds][4] = i, j, o2, -), one launch, one block per ligand.  id_0(a) = push chained from 0 over Z,
 * heavy degree, h_count, charge, in-ring (a bond of the atom is no bridge), flags & 1 - or atom_invariants[a] (uint32 [n_atoms]) when
 * that pointer is not NULL.  id_r(a), r = 1 .. radius: push chained from 0 over r, id_{r-1}(a) and the neighbours' pairs (o2, id_{r-1})
 * in ascending order, o2 then id.  env_r(a), a set of the ligand's bonds: env_0 empty, env_r(a) = env_{r-1}(a) | union over neighbours
 * b of (env_{r-1}(b) | {bond a-b}).  Every radius-0 feature is kept; (a, r), r >= 1, exactly when no feature (a', r'), r' >= 1, with the
 * same bond set has a smaller (r', id, a'); every atom iterates to the last radius.  A kept feature sets bit id & (n_bits - 1).
 *   bits uint32 [G][n_bits / 32] (bit k = bit k % 32 of word k / 32), ids uint32 [n_atoms][radius + 1], kept uint8 [n_atoms][radius + 1],
 *   n_features int32 [G] (kept features), popcount int32 [G]
 * Integers only, no atomics but an LDS OR into the bit row: a ligand's bits do not depend on the library around it.  Limits as for
 * pd_ligand_features; a ligand whose rows leave the arrays is not written and a bond that leaves its ligand is skipped.  A NULL pointer
 * (bonds may be NULL when n_bonds == 0, atom_invariants always), a misaligned pointer, n_ligands < 1, n_atoms < n_ligands, a radius
 * outside 0 .. PD_FINGERPRINT_MAX_RADIUS, n_bits other than 512, 1024, 2048, 4096: PD_ERR_ARG; n_ligands > 65535 or more atoms than
 * that many ligands of the largest size: PD_ERR_UNSUPPORTED.
 *
 * pd_fingerprint_tanimoto: a uint32 [n][n_words], b uint32 [m][n_words] -> sim fp32 [n][m] and, when not NULL, common int32 [n][m].
 * With c = popcount(a & b) and u = popcount(a) + popcount(b) - c the value is the IEEE fp32 quotient (float)c / (float)u; an empty
 * union gives 1, as pd_plif_pairwise does.
 * pd_fingerprint_nearest: for each row of a the k rows of b of the largest similarity -> index int32 [n][k], similarity fp32 [n][k],
 * common int32 [n][k], best first; ordered by the exact fraction (c1 u2 against c2 u1; an empty union as 1 / 1), the smaller column
 * on a tie; exclude_self = 1 skips column i for row i.  n x m is never stored.  1 <= k <= PD_FINGERPRINT_MAX_K, k <= m - exclude_self.
 * pd_fingerprint_maxmin: the MaxMin diverse subset (Ashton et al. 2002): picks[0] = first, then the unpicked row whose largest
 * similarity to the picked rows is smallest (the largest min of 1 - T), exact fractions, the smallest index on a tie -> picks int32
 * [n_pick], max_similarity fp32 [n_pick] (that largest similarity; NaN for the first).  1 + 2 (n_pick - 1) launches, the next pick stays
 * on the device.  ws: pd_fingerprint_maxmin_workspace_numel(n) int32.
 * All three: 1 <= n_words <= PD_FINGERPRINT_MAX_WORDS; rows up to 65535 * 16 (else PD_ERR_UNSUPPORTED); a NULL or misaligned pointer,
 * a count < 1, k, n_pick or first out of range, a short workspace: PD_ERR_ARG.  A rejected call launches nothing.               */
#define PD_FINGERPRINT_MAX_RADIUS 4
#define PD_FINGERPRINT_MAX_WORDS 128
#define PD_FINGERPRINT_MAX_K 16
int pd_morgan_fingerprint(const int* atom_start, const int* bond_start, const int* atoms, const int* bonds,
                          const unsigned* atom_invariants, unsigned* bits, unsigned* ids, unsigned char* kept, int* n_features,
                          int* popcount, int n_ligands, int n_atoms, int n_bonds, int radius, int n_bits, void* stream);
int pd_fingerprint_tanimoto(const unsigned* a, const unsigned* b, float* sim, int* common, int n, int m, int n_words, void* stream);
int pd_fingerprint_nearest(const unsigned* a, const unsigned* b, int* index, float* similarity, int* common, int n, int m, int n_words,
                           int k, int exclude_self, void* stream);
int pd_fingerprint_maxmin_workspace_numel(int n);
int pd_fingerprint_maxmin(const unsigned* bits, int* ws, int ws_numel, int* picks, float* max_similarity, int n, int n_words, int n_pick,
                          int first, void* stream);

/* ---- substructure search over a ligand library (substructure.hip; additive exports of ABI 11) -----------------------------------
 * Which ligands contain a query pattern, how often and on which atoms?  The package's own definition, not RDKit's:
 * tests/substructure_ref.py; physdock_amd/smarts.py reads the queries from a stated subset of SMARTS.
 *
 * The ligands are the tables of pd_ligand_features (or atoms / bonds as pd_aromaticity returned them).  Per atom: heavy degree,
 * aromatic (flags & 1, or a bond with o2 = 3), ring (a bond of the atom is no bridge).  Per bond one of ten states, 2 * (0 single, 1
 * double, 2 triple, 3 aromatic, 4 other) + (1 when the bond is no bridge).  The Q queries are packed as
 *   q_atom_start int32 [Q+1]              prefix sums of the query atoms (1 .. PD_SUBSTRUCT_MAX_QUERY_ATOMS each)
 *   q_op_start   int32 [n_query_atoms+1]  prefix sums of the ops of every query atom (1 .. PD_SUBSTRUCT_MAX_OPS each)
 *   q_ops        int32 [n_ops]            code | argument << 8, postfix over a stack of truth values (PD_SUBSTRUCT_OP_*); the value
 *                                         of an atom program is the top of the stack at its end
 *   q_bond_start int32 [Q+1]              prefix sums of the query bonds (0 .. PD_SUBSTRUCT_MAX_QUERY_BONDS each)
 *   q_bonds      int32 [n_query_bonds][4] (lo, hi, mask, -): lo < hi query atoms of that query, sorted by hi; bit s of mask allows
 *                                         state s.  Every query atom but the first is the hi of a bond; its parent is the lowest lo
 *   atom_classes int32 [n_atoms] or NULL  the word PD_SUBSTRUCT_OP_CLASS reads: bit k, inner pattern k anchors on this atom
 * An embedding maps the query atoms injectively to the atoms of one ligand, every program true and every query bond on a ligand bond
 * of an allowed state.  The search is depth-first in the order of the query atoms: atom 0 on every atom that passes its program,
 * ascending (an anchor), atom k on the free neighbours of its parent's image that pass program k, ascending.  One candidate is one
 * step; an anchor that has spent max_steps when a candidate is due stops with what it found.
 *
 * pd_substructure_search, one launch for G ligands x Q queries:
 *   n_embeddings, n_unique, status int32 [G][Q]: the embeddings found (saturating at 2^31 - 1); those that are the lexicographically
 *   smallest embedding onto their own atom set; 0 done, 2 a budget ran out (1 is reserved: not written)
 *   atom_hits, anchor_hits uint32 [n_atoms][ceil(Q / 32)], bit q % 32 of word q / 32: the atom lies in an embedding of query q / is
 *   the image of its atom 0
 * pd_substructure_matches, for the one query `query` of `query_atoms` atoms: matches int32 [G][max_matches][query_atoms], the first
 * embeddings of every ligand in the order above (unique_only = 1: the first unique ones) as atom indices local to the ligand, the
 * rest -1; n_written int32 [G].
 * Integers only, no atomics but a commuting LDS OR: bit-identical from launch to launch and independent of a ligand's place in the
 * library.  A ligand or a query whose rows leave the arrays or break the limits is not written.  PD_ERR_ARG: a NULL or misaligned
 * required pointer (bonds may be NULL when n_bonds == 0, q_bonds when n_query_bonds == 0, atom_classes always), n_ligands or
 * n_queries < 1, n_atoms < n_ligands, max_steps < 0, table sizes that no n_queries patterns within the limits have, query outside
 * 0 .. n_queries - 1, query_atoms outside 1 .. PD_SUBSTRUCT_MAX_QUERY_ATOMS, max_matches outside 1 .. PD_SUBSTRUCT_MAX_MATCHES,
 * unique_only other than 0 or 1.  PD_ERR_UNSUPPORTED: n_ligands > 65535, n_queries > 1024, more atoms than that many ligands of the
 * largest size.  A rejected call launches nothing.                                                                               */
#define PD_SUBSTRUCT_MAX_QUERY_ATOMS 32
#define PD_SUBSTRUCT_MAX_QUERY_BONDS 64
#define PD_SUBSTRUCT_MAX_OPS 32
#define PD_SUBSTRUCT_MAX_MATCHES 256
#define PD_SUBSTRUCT_OP_TRUE 0               /* the argument is unused                                     */
#define PD_SUBSTRUCT_OP_Z 1                  /* Z == argument                                              */
#define PD_SUBSTRUCT_OP_AROMATIC 2
#define PD_SUBSTRUCT_OP_ALIPHATIC 3
#define PD_SUBSTRUCT_OP_DEGREE 4             /* heavy degree == argument                                   */
#define PD_SUBSTRUCT_OP_H_COUNT 5
#define PD_SUBSTRUCT_OP_CONNECTIVITY 6       /* degree + h_count == argument                               */
#define PD_SUBSTRUCT_OP_RING 7
#define PD_SUBSTRUCT_OP_CHARGE 8             /* charge == argument - 128                                   */
#define PD_SUBSTRUCT_OP_CLASS 9              /* bit `argument` of the atom's class word                    */
#define PD_SUBSTRUCT_OP_NOT 10
#define PD_SUBSTRUCT_OP_AND 11
#define PD_SUBSTRUCT_OP_OR 12
#define PD_SUBSTRUCT_OP_ELEMENT_ALIPHATIC 13 /* Z == argument and not aromatic                             */
#define PD_SUBSTRUCT_OP_ELEMENT_AROMATIC 14  /* Z == argument and aromatic                                 */
int pd_substructure_search(const int* atom_start, const int* bond_start, const int* atoms, const int* bonds, const int* q_atom_start,
                           const int* q_op_start, const int* q_ops, const int* q_bond_start, const int* q_bonds,
                           const int* atom_classes, int* n_embeddings, int* n_unique, int* status, unsigned* atom_hits,
                           unsigned* anchor_hits, int n_ligands, int n_atoms, int n_bonds, int n_queries, int n_query_atoms, int n_ops,
                           int n_query_bonds, int max_steps, void* stream);
int pd_substructure_matches(const int* atom_start, const int* bond_start, const int* atoms, const int* bonds, const int* q_atom_start,
                            const int* q_op_start, const int* q_ops, const int* q_bond_start, const int* q_bonds,
                            const int* atom_classes, int* matches, int* n_written, int n_ligands, int n_atoms, int n_bonds,
                            int n_queries, int n_query_atoms, int n_ops, int n_query_bonds, int query, int query_atoms, int max_matches,
                            int unique_only, int max_steps, void* stream);

/* ---- canonical numbering, certificate and identity key of ligand graphs (canonical.hip; additive exports of ABI 11) ---------------
 * Are two records the same molecule, and what is its one spelling?  The package's own definition, not InChI and not RDKit's
 * canonical SMILES: tests/canonical_ref.py.  push and fmix are the hash functions of pd_morgan_fingerprint.
 *
 * The ligands are the tables of pd_ligand_features (or atoms / bonds as pd_aromaticity returned them) and
 *   isotopes      int32 [n_atoms]         0 .. 65535
 *   chiral_order  int32 [n_atoms][4]      of a marked atom its neighbours in the written order, local to the ligand, -1 a hydrogen,
 *                                         padded with -2; an order of fewer than 3 or more than 4 entries is an empty row
 *   stereo_start  int32 [G+1], stereo int32 [n_stereo][8]   rows (a, b, c, d, kind, a2, d2, -) of smiles.parse_smiles, up to
 *                                         PD_CANONICAL_MAX_STEREO per ligand
 *   cert_start    int32 [G+1]             prefix sums of 3 + 2 n + m + s words per ligand
 * inv(a) = (Z, charge, h_count, isotope, flags & 1).  A colouring gives every atom the number of atoms with a strictly smaller key;
 * the root colours by inv; one round colours by (colour, sum mod 2^32 over the bonds (a, b) of push(push(0, o2), colour[b])); refine
 * repeats rounds until the number of colours stops growing; individualise(v) colours by (colour, a != v) and refines.  Depth-first
 * from the refined root: at a colouring that is not discrete the members of the cell of the smallest colour with more than one atom
 * are tried in ascending index, except a terminal atom when an earlier member is terminal on the same neighbour with the same o2.
 * Every refine is one step; a step that is due when max_steps are spent ends the search with status 2.  A discrete colouring is a
 * leaf; its certificate is the words n, m; per label Z | (charge + 128) << 8 | h_count << 16 | aromatic << 24 and isotope | parity <<
 * 16; the bonds lo << 16 | hi << 8 | o2 in labels, ascending; s; the stereo rows b << 23 | c << 16 | a << 9 | d << 2 | kind in labels
 * (b < c, a and d the lowest-label substituents, kind flipped for every end that names the other one), ascending.  parity: 0 without
 * a mark, with h_count >= 2, an empty chiral_order row or two terminal neighbours of equal inv and o2; else the mark (1 @, 2 @@),
 * exchanged when the row in labels has an odd number of inversions.  The smallest certificate wins, the first found on a tie.
 *   labels, order int32 [n_atoms]  (order the inverse of labels within the ligand; the input order when no leaf was reached)
 *   classes int32 [n_atoms]        the refined root colouring: topological symmetry classes
 *   cert uint32 [n_cert_words], key uint32 [G][2] (push chained over the certificate from the seeds 0 and 1)
 *   status (0 done, 2 out of steps; 1 is reserved), steps, leaves, canonical (1 exactly when status is 0) int32 [G]
 * pd_canonical_first: first_of int32 [G], the smallest j < g with status 0, an equal key and a certificate equal word for word, else
 * g; a ligand whose status is not 0 is its own first and nobody else's.
 * Integers only, no atomics: bit-identical from launch to launch and independent of a ligand's place in the library.  A ligand whose
 * rows leave the arrays or break the limits is not written.  PD_ERR_ARG: a NULL or misaligned required pointer (bonds may be NULL
 * when n_bonds == 0, stereo when n_stereo == 0), n_ligands < 1, n_atoms < n_ligands, max_steps < 1, n_cert_words other than
 * 3 n_ligands + 2 n_atoms + n_bonds + n_stereo.  PD_ERR_UNSUPPORTED: n_ligands > 65535, more atoms than that many ligands of the
 * largest size, 2^31 words or more.  A rejected call launches nothing.                                                         */
#define PD_CANONICAL_MAX_STEREO 64
int pd_canonical_form(const int* atom_start, const int* bond_start, const int* atoms, const int* bonds, const int* isotopes,
                      const int* chiral_order, const int* stereo_start, const int* stereo, const int* cert_start, int* labels,
                      int* order, int* classes, unsigned* cert, unsigned* key, int* status, int* steps, int* leaves, int* canonical,
                      int n_ligands, int n_atoms, int n_bonds, int n_stereo, long long n_cert_words, int max_steps, void* stream);
int pd_canonical_first(const unsigned* key, const int* status, const int* cert_start, const unsigned* cert, int* first_of,
                       int n_ligands, long long n_cert_words, void* stream);

/* ---- hipGraph helpers (api.hip): capture the host-deterministic step loop once, replay it */
int pd_graph_begin(void* stream);
int pd_graph_end(void* stream, void** exec_out);
int pd_graph_launch(void* exec, void* stream);
int pd_graph_destroy(void* exec);

/* ---- library management ------------------------------------------------------------- */
int pd_abi_version(void);
int pd_gemm_args_size(void);  /* sizeof(pd_gemm_args) / sizeof(pd_attn_args) as compiled: a binding checks its own struct  */
int pd_attn_args_size(void);  /* mirror against these before the first call (a short struct would be read past its end)   */
int pd_init(void);            /* sets per-kernel LDS limits; call once before graph capture */
int pd_attention_occupancy(void);   /* diagnostic: resident attention blocks per CU (runtime's figure) */

#ifdef __cplusplus
}
#endif
#endif
