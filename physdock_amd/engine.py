"""Kernel orchestration for the conditioning trunk and the AF3DiT denoiser.

This module owns no arithmetic: every number is produced by a launcher of
libphysdock_hip.so (ops.py).  It mirrors, call for call, the module tree of the reference
(layers/diffusion_conditioning.py, layers/transformers.py, primitives/*.py) but with the
algebraic levers of SURVEY §7 applied:

* norms are folded into the GEMM that consumes them (row statistics + A-tile transform),
* q/k/v(/g) projections are one GEMM, SwiGLU / sigmoid-gated pairs are one GEMM,
* pair biases are written directly in the attention kernel's fragment layout; the DiT's 18
  step- and sample-invariant bias projections are hoisted out of the loop (one GEMM over
  ``ap`` and one over ``z`` per call),
* AdaLN (shift, 1+scale, gate) tables for all steps are two GEMMs per call.
"""
from __future__ import annotations

import math

import torch

from . import ops
from ._lib import ACT_RELU, ACT_SIGMOID, ACT_SILU, LOG2E
from .ops import LN, OUT_BIASFRAG, OUT_OPM, OUT_TRANSPOSED, RMS


def off(t, n):
    """device address of element n of tensor t (fp32 / int32 alike: 4-byte elements)"""
    return t.data_ptr() + 4 * n


class Workspace:
    """Named, shape-keyed scratch buffers (torch tensors used as raw device memory)."""

    def __init__(self, device):
        self.device = device
        self.bufs = {}

    def get(self, name, *shape, dtype=torch.float32, zero=False):
        key = (name, tuple(shape), dtype)
        t = self.bufs.get(key)
        if t is None:
            t = (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=self.device)
            self.bufs[key] = t
        return t

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in self.bufs.values())


class Engine:
    def __init__(self, packed, config, device):
        self.P = packed            # PackedWeights
        self.cfg = config
        self.device = device
        self.ws = Workspace(device)
        self.lane = 0              # sample lane (concurrent stream) whose private DiT scratch is in use
        #: DiT families ("atom" / "token") whose launches were taken off the two-part fp16 format by check_dit_bounds (their bounds
        #: turned out too loose for these weights): they run on bf16 x 6, which needs no bound.  Lives with the engine = the weights.
        self.f16_off = set()
        self.probe = None          # check_dit_bounds: records (operand, observed magnitudes, bound) at three sites of dit_block
        self.bound_report = {}     # family -> operand -> dict(amax_ratio, typical_ratio): the last check_dit_bounds result
        self._bounds_checked = set()
        self._bounds_failed = {}
        dc = config.model.diffusion_conditioning
        self.inf, self.eps = float(dc.inf), float(dc.eps)

    # ------------------------------------------------------------------ small helpers
    def gemm(self, A, W, Y, M, N, K, **kw):
        """ops.gemm with the pre-split (3 x bf16) copy of a weight operand attached when W is a packed weight matrix, so
        that eligible shapes run on the bf16 matrix pipe at fp32 accuracy (csrc/gemm_split.hip).  Activation x activation
        contractions (raw addresses, k-major / batched operands) stay on the fp32 MFMA."""
        w3 = None
        if isinstance(W, torch.Tensor) and W.dim() == 2 and W.shape[0] == N and K % 4 == 0 and kw.get("batch", 1) == 1 \
                and not kw.get("a_kmajor") and not kw.get("w_kmajor") and N % 64 == 0 \
                and (kw.get("out_mode", 0) == 0 or (kw.get("out_mode") == OUT_TRANSPOSED and kw.get("glu"))):
            w3 = self.P.w3(W, K)
        rowmajor_or_glut = kw.get("out_mode", 0) == 0 or (kw.get("out_mode") == OUT_TRANSPOSED and kw.get("glu"))
        if kw.get("a_amax") is None and w3 is not None and ops.F16_GEMM and ops.F16_NORM_BOUND and rowmajor_or_glut \
                and kw.get("stats") is not None and not kw.get("pro_rows_per_group") \
                and all(v is None or isinstance(v, torch.Tensor) for v in (kw.get("pro_w"), kw.get("pro_b"))):
            # a norm prologue with STATIC gain / shift bounds its own output for any input: |x^_k| <= sqrt(K) after RMSNorm or
            # LayerNorm, so |x^ w + b| <= sqrt(K) max|w| + max|b| (an activation in the prologue only shrinks it) - the trunk's
            # normalised projections take the two-part fp16 format on this bound
            kw["a_amax"] = self.P.norm_bound(kw.get("pro_w"), kw.get("pro_b"), K)
        if kw.get("a_amax") is not None and w3 is not None and ops.F16_GEMM and rowmajor_or_glut:
            # the caller knows an upper bound of |A'|: two-part fp16 operands (three MFMA products instead of six)
            kw["W2"] = self.P.w2(W, K)
        else:
            kw.pop("a_amax", None)
            if kw.pop("A2", None) is not None:
                raise RuntimeError("a pre-split fp16 A operand was prepared for a launch that cannot take it")
        ksw = None
        if kw.get("batch", 1) == 1 and kw.get("out_mode", 0) == 0 and M <= 8192 and K >= 256 and not kw.get("a_kmajor"):
            # few rows x long K (token-level projections at a handful of samples): scratch that lets pd_gemm cut K
            ksw = self.ws.get("gemm_ksplit", 9 << 20)
        return ops.gemm(A, W, Y, M, N, K, W3=w3, ksplit_ws=ksw, **kw)

    def trunk_attn_bounds(self, prefix, norm_weight):
        """static |q|, |k|, |v| bounds of a trunk attention (None: keep the bf16 x 6 kernel)"""
        if not (ops.F16_ATTN and ops.F16_TRUNK_ATTN and ops.SPLIT_ATTN):
            return None
        return self.P.attn_static_bounds(prefix, norm_weight)

    _PS_MEMO = {}

    def attn_prescale(self, qk, nbatch, nq, nk, H, ws=None, strides=None):
        """power of two to fold into the out_scale of the bias producer of an attention launch, or 0.0: non-zero exactly when
        pd_attention would run this launch on the pipelined fp16-format kernel (variant 3000 +), which takes the bias tile - times the
        product of its q and k operand scales - as the initial value of the score accumulator.  qk: host (|q|, |k|) bounds or None."""
        if qk is None or not (ops.PIPE_ATTN and ops.F16_ATTN and ops.SPLIT_ATTN):
            return 0.0
        # strides: the (batch, sequence) strides in floats the REAL launch addresses q / k / v with - the pipelined kernel's
        # 32-bit buffer offsets bound them (pd_attention_pipe_ok), so the probe must see them, and the real pre-scale too (its
        # magnitude limit); the library refuses a pre-scaled bias on any other kernel (PD_ERR_ARG) should the two ever disagree
        st = tuple(strides) if strides is not None else (max(nq, nk) * H * 32, H * 32)
        key = (float(qk[0]), float(qk[1]), nbatch, nq, nk, H, ws is not None and ws.numel(), st,
               ops.PIPE_ATTN, ops.F16_ATTN, ops.SPLIT_ATTN)
        r = Engine._PS_MEMO.get(key)
        if r is None:
            d = 1 << 20
            r = ops.attn_bias_prescale(qk[0], qk[1])
            v = ops.attention(d, d, d, d, nq=nq, nk=nk, nbatch=nbatch, nheads=H, q_strides=st, k_strides=st,
                              v_strides=st, o_strides=(nq * H * 32, H * 32), bias=d, bias_nk=nq, ws=ws,
                              f16_amax=(qk[0], qk[1], 1.0), bias_prescale=r, query_only=True)
            if v < 3000:
                r = 0.0
            Engine._PS_MEMO[key] = r
        return r

    def trunk_prescale(self, prefix, norm_weight, nbatch, nq, nk, H, strides=None):
        """attn_prescale of a trunk attention (static bounds from the projection weights)"""
        if self.trunk_attn_bounds(prefix, norm_weight) is None:
            return 0.0
        return self.attn_prescale(self.P.attn_static_bounds_host(prefix, norm_weight)[:2], nbatch, nq, nk, H, self.attn_ws(nbatch, nq, nk, H),
                                  strides=strides)

    @staticmethod
    def o_bound(bounds):
        """device address of the v bound inside a (q, k, v) bound vector = bound of the attention output (a convex combination of v rows)"""
        return None if (bounds is None or not (ops.F16_GEMM and ops.F16_TRUNK_GEMM and ops.SPLIT_GEMM)) else bounds.data_ptr() + 8

    def lws(self, name, *shape, dtype=torch.float32):
        """lane-private scratch: concurrent sample lanes never share a DiT intermediate"""
        return self.ws.get(f"{name}@{self.lane}", *shape, dtype=dtype)

    def stats(self, x, M, C, mode, eps, name="stats", kmajor=False, ldx=None):
        st = self.ws.get(f"{name}@{self.lane}", M, 2)
        ops.rowstats(x, st, M, C, mode=mode, eps=eps, kmajor=kmajor, ldx=ldx)
        return st

    def stats_buf(self, M, name="stats"):
        """[M, 2] scratch for row statistics the consuming GEMM fills or computes itself (ops.gemm(stats_inline=))"""
        return self.ws.get(f"{name}@{self.lane}", M, 2)

    def attn_ws(self, nbatch, nq, nk, nheads):
        """scratch for key-split attention launches (None when the launch fills the chip by itself)"""
        n = ops.attn_split_ws_numel(nbatch, nq, nk, nheads)
        return self.lws("attn_split", n) if n else None

    def lin(self, x, wname, M, out=None, **kw):
        """plain Linear by packed-weight name; returns the output tensor"""
        W, b, N, K, ldw = self.P.linear(wname)
        if out is None:
            out = self.ws.get("lin:" + wname, M, N)
        lda = kw.pop("lda", K)
        self.gemm(x, W, out, M, N, K, lda=lda, ldw=ldw, bias=b, **kw)
        return out

    # ------------------------------------------------------------------ shared blocks
    def pair_bias(self, prefix, z, T1, T2, C, mask, norm_w, out, transpose=False, norm="norm_z", st_out=None, prescale=0.0):
        """bias[h, q, k] = (W_z . RMSNorm(z))[h] + maskbias -> fragment layout (x log2 e).  One streaming pass over z
        (pd_pair_bias) that also leaves the row statistics in `st_out` for the projection GEMM that shares the norm;
        shapes the kernel does not cover go through rowstats + GEMM."""
        P = self.P
        W, _, H, K, ldw = P.linear(prefix + ".linear_z")
        osc = LOG2E * (prescale if prescale > 0 else 1.0)      # prescale: see attn_prescale (a power of two: exact)
        if ops.pair_bias(z, P.bias_w(prefix, norm), out, T1, T2, C, H, stats_out=st_out, maskadd=mask, maskval=-self.inf,
                         out_scale=osc, transpose=transpose, mode=RMS, eps=self.eps, only_if_faster=True):
            return H
        st = st_out if st_out is not None else self.ws.get(f"stats_pb@{self.lane}", T1 * T2, 2)
        ops.rowstats(z, st, T1 * T2, C, mode=RMS, eps=self.eps)
        self.gemm(z, W, out, T1 * T2, H, C, ldw=ldw, stats=st, pro_w=norm_w, out_mode=OUT_BIASFRAG, T1=T1, T2=T2,
                  frag_transpose=transpose, maskadd=mask, maskval=-self.inf, out_scale=osc)
        return H

    def attention_pair_bias(self, prefix, s, nbatch, N, C, bias, norm_name="norm_s", nk=None, bias_prescale=0.0):
        """s += (W_o . Attn(RMSNorm(s)) + b_o) * (W_g RMSNorm(s) + b_g)   (attentions.py:32-53,76-97)"""
        P = self.P
        rows = nbatch * N
        H = C // 32
        W, b = P.qkvg(prefix)
        qkvg = self.ws.get("qkvg", rows, 4 * C)
        self.gemm(s, W, qkvg, rows, 4 * C, C, stats=self.stats_buf(rows), stats_inline=(RMS, self.eps),
                  pro_w=P[f"{prefix}.{norm_name}.weight"], bias=b)
        o = self.ws.get("attn_o", rows, C)
        st4 = (N * 4 * C, 4 * C)
        ops.attention(off(qkvg, 0), off(qkvg, C), off(qkvg, 2 * C), o, nq=N, nk=nk or N, nbatch=nbatch, nheads=H,
                      q_strides=st4, k_strides=st4, v_strides=st4, o_strides=(N * C, C), bias=bias, bias_nk=N,
                      ws=self.attn_ws(nbatch, N, nk or N, H), f16_amax=(bnd := self.trunk_attn_bounds(prefix, P[f"{prefix}.{norm_name}.weight"])),
                      bias_prescale=bias_prescale)
        Wo, bo, _, _, ldw = P.linear(prefix + ".linear_o")
        self.gemm(o, Wo, s, rows, C, C, ldw=ldw, bias=bo, mul=off(qkvg, 3 * C), ldmul=4 * C, res=s, a_amax=self.o_bound(bnd))

    def transition(self, prefix, x, rows, C):
        """x += W2(silu(W1 RMSNorm(x)) * W3 RMSNorm(x))                    (transitions.py:15-18)"""
        P = self.P
        W13, hidden = P.glu(prefix + ".feed_forward")
        W2, _, _, _, ldw = P.linear(prefix + ".feed_forward.w2")
        nw = P[prefix + ".ffn_norm.weight"]
        f16 = ops.F16_GEMM and ops.F16_TRUNK_GEMM and ops.SPLIT_GEMM
        hb = P.glu_hidden_bound(prefix + ".feed_forward", nw) if f16 else None
        # pair rows (C = 128, hidden = 384, >= 32768 of them): the whole transition in ONE launch - RMS statistics, SwiGLU, down-
        # projection, residual, the hidden activations never leave the CU (the DiT's atom-transition kernel with rms = 1, a zero
        # shift and a unit gate; static bounds of y and h from the weights)
        if f16 and ops.FUSED_TRANSITION and ops.FUSED_TRUNK_TRANSITION and W13.shape[1] == C and ldw == hidden \
                and ops.transition_f16(x, rows, C, hidden, shift=ops.const_vec(0.0, C), scale1p=nw, gate=ops.const_vec(1.0, C),
                                       W13=P.w2(W13, C), W2=P.w2(W2, hidden), y_amax=P.norm_bound(nw, None, C), h_amax=hb,
                                       eps=self.eps, rms=True):
            return
        h = self.ws.get("ffn_h", rows, hidden)
        self.gemm(x, W13, h, rows, 2 * hidden, C, stats=self.stats_buf(rows), stats_inline=(RMS, self.eps), pro_w=nw, glu=1)
        self.gemm(h, W2, x, rows, C, hidden, ldw=ldw, res=x, a_amax=hb)

    def triangle_update(self, prefix, z, T, C, mask, transpose):
        """z += TriangleUpdate(z)                                          (attentions.py:157-171)"""
        P = self.P
        M = T * T
        st = self.stats(z, M, C, RMS, self.eps)
        nw = P[prefix + ".norm_in.weight"]
        Wqk, bqk = P.tri_qk(prefix)                       # packed [qx|q|kx|k] -> 64 outputs (q 32 | k 32)
        qk = self.ws.get("tri_qk", 64, M)
        self.gemm(z, Wqk, qk, M, 128, C, stats=st, pro_w=nw, bias=bqk, glu=2, rowscale=mask,
                 out_mode=OUT_TRANSPOSED, ldy=M)
        Wg, bg, _, _, ldw = P.linear(prefix + ".linear_g")
        Wz, bz, _, _, ldwz = P.linear(prefix + ".linear_z")
        wout = P[prefix + ".norm_out.weight"]
        # one launch for everything behind the einsum (pd_tri_tail) when the shapes are the model's (C = 128, 32 einsum channels)
        fused = ops.FUSED_TRI_TAIL and ops.F16_GEMM and ops.F16_TRUNK_GEMM and ops.SPLIT_GEMM and C == 128 and ldw == C and ldwz == 32 \
            and Wg.shape[0] == C and Wz.shape == (C, 32)
        g = None
        if not fused:
            g = self.ws.get("tri_g", M, C)
            self.gemm(z, Wg, g, M, C, C, ldw=ldw, stats=st, pro_w=nw, bias=bg, act=ACT_SIGMOID)
        o = self.ws.get("tri_o", 32, M)
        Tr = self.Tr          # the sum over j runs over REAL tokens only (padded j never enter a reduction)
        f16mul = False
        if (ops.F16_TRI_MUL is True or (ops.F16_TRI_MUL == "row" and not transpose)) and ops.F16_GEMM and ops.F16_TRUNK_GEMM \
                and ops.SPLIT_GEMM and Wqk.shape[0] == 128:
            bq = P.tri_qk_bounds(prefix, nw)         # static bounds of |q|, |k|: the einsum takes the two-part fp16 format
            f16mul = ops.tri_mul(off(qk, 0), off(qk, 32 * M), o, T, Tr, 32, M, transpose=transpose, q_amax=bq.data_ptr(), k_amax=bq.data_ptr() + 4)
        if f16mul:
            pass
        elif not transpose:   # o[c,i,I] = sum_j q[c,i,j] k[c,I,j]
            self.gemm(off(qk, 0), off(qk, 32 * M), o, T, T, Tr, lda=T, ldw=T, ldy=T, batch=32, sA=M, sW=M, sY=M)
        else:               # o[c,a,b] = sum_j k[c,j,a] q[c,j,b]
            self.gemm(off(qk, 32 * M), off(qk, 0), o, T, T, Tr, lda=T, ldw=T, ldy=T, batch=32, sA=M, sW=M, sY=M,
                     a_kmajor=True, w_kmajor=True)
        if fused and ops.tri_tail(z, o, M, C, 32, w_in=nw, w_out=wout, eps=self.eps, Wg=P.w2(Wg, C), bg=bg, Wz=P.w2(Wz, 32), bz=bz,
                                  zn_amax=P.norm_bound(nw, None, C), on_amax=P.norm_bound(wout, None, 32)):
            return
        if g is None:
            g = self.ws.get("tri_g", M, C)
            self.gemm(z, Wg, g, M, C, C, ldw=ldw, stats=st, pro_w=nw, bias=bg, act=ACT_SIGMOID)
        st2 = self.stats(o, M, 32, RMS, self.eps, "stats_tri", kmajor=True, ldx=M)
        self.gemm(o, Wz, z, M, C, 32, a_kmajor=True, lda=M, ldw=ldwz, stats=st2, pro_w=wout,
                 bias=bz, mul=g, ldmul=C, res=z)

    def triangle_attention(self, prefix, z, T, C, mask, transpose):
        """z += TriangleAttention(z)                                       (attentions.py:194-217)"""
        P = self.P
        M = T * T
        H = C // 32
        nw = P[prefix + ".norm.weight"]
        # bias first: its streaming pass over z also produces the row statistics of the shared norm
        st = self.ws.get(f"stats@{self.lane}", M, 2)
        bias = self.ws.get("tri_bias", ops.bias_frag_numel(H, T, T), zero=True)
        # (strides of the widest projection layout, q|k|v|g: the fused-tail q|k|v form only shrinks them)
        ps = self.trunk_prescale(prefix, nw, T, T, self.Tr, H, strides=(4 * C, T * 4 * C) if transpose else (T * 4 * C, 4 * C))
        bnd = self.trunk_attn_bounds(prefix, nw)
        Wo, bo, _, _, ldw = P.linear(prefix + ".linear_o")
        # round 6: when the attention projects q | k | v inside its blocks (csrc/tri_attn.hip) the bias pass over z also writes the
        # normalised rows, scaled and split, in that kernel's fragment order (33.5 MB at T = 256, read by the four head blocks of a row)
        zn_amax = math.sqrt(C) * 1.0001
        want_in_block = (bnd is not None and ops.F16_GEMM and ops.F16_TRUNK_GEMM and ops.SPLIT_GEMM and C == 128 and ldw == C and H == 4
                         and ops.FUSED_TRI_ATTN and ps > 0.0 and T <= 256 and T % 4 == 0)
        z2 = None
        if want_in_block:
            z2 = self.ws.get("tri_z2", ops.tri_z2_numel(T), dtype=torch.float16, zero=True)
            if not ops.pair_bias_split(z, P.bias_w(prefix, "norm"), bias, T, z2, stats_out=st, maskadd=mask, maskval=-self.inf,
                                       out_scale=LOG2E * ps, transpose=transpose, eps=self.eps, zn_amax=zn_amax):
                z2 = None
        if z2 is None:
            self.pair_bias(prefix, z, T, T, C, mask, nw, bias, transpose=transpose, norm="norm", st_out=st, prescale=ps)
        # With the fused tail (pd_tri_tail mode 1: gate projection + linear_o + gate + residual in one launch) the projection in
        # front is q|k|v only and the gate tensor never exists
        f16 = bnd is not None and ops.F16_GEMM and ops.F16_TRUNK_GEMM and ops.SPLIT_GEMM and C == 128 and ldw == C
        fused = f16 and ops.FUSED_TRI_ATTN_TAIL
        o = self.ws.get("attn_o", M, C)
        # round 6: the q | k | v projection INSIDE the attention block (csrc/tri_attn.hip): q | k | v never exist in HBM.  Needs the
        # pre-scaled bias of the fp16-format kernels and T <= 256; the gate is then projected by the fused tail or on its own
        in_block = (z2 is not None
                    and ops.tri_attention(z2, P.qkv_folded_w2(prefix, nw), bias, o, T, self.Tr, C, H, transpose=transpose,
                                          bias_prescale=ps, bias_nk=T, qkv_amax=bnd, zn_amax=zn_amax))
        if z2 is not None and not in_block:
            raise RuntimeError("pd_tri_attention refused a shape pd_pair_bias_split accepted")
        nq = 3 if fused else 4
        qkvg = None
        if not in_block:
            if fused:
                W, b, _, _ = P.qkv_g(prefix)
                qkvg = self.ws.get("qkv3", M, 3 * C)
            else:
                W, b = P.qkvg(prefix)
                qkvg = self.ws.get("qkvg", M, 4 * C)
            self.gemm(z, W, qkvg, M, nq * C, C, stats=st, pro_w=nw, bias=b)
            if not transpose:
                st4, sto = (T * nq * C, nq * C), (T * C, C)
            else:
                st4, sto = (nq * C, T * nq * C), (C, T * C)
            ops.attention(off(qkvg, 0), off(qkvg, C), off(qkvg, 2 * C), o, nq=T, nk=self.Tr, nbatch=T, nheads=H,
                          q_strides=st4, k_strides=st4, v_strides=st4, o_strides=sto, bias=bias, bias_nk=T,
                          f16_amax=bnd, bias_prescale=ps)
        Wg, bg = P[prefix + ".linear_g.weight"], P[prefix + ".linear_g.bias"]
        if fused and ops.tri_tail(z, o, M, C, C, w_in=nw, w_out=None, eps=self.eps, Wg=P.w2(Wg, C), bg=bg, Wz=P.w2(Wo, C), bz=bo,
                                  zn_amax=P.norm_bound(nw, None, C), on_amax=self.o_bound(bnd), mode=1):
            return
        if fused or in_block:   # no gate tensor yet: the gate as its own projection, then the three-operand epilogue
            gt = self.ws.get("tri_g", M, C)
            self.gemm(z, Wg, gt, M, C, C, stats=st, pro_w=nw, bias=bg)
            self.gemm(o, Wo, z, M, C, C, ldw=ldw, bias=bo, mul=gt, ldmul=C, res=z, a_amax=self.o_bound(bnd))
            return
        self.gemm(o, Wo, z, M, C, C, ldw=ldw, bias=bo, mul=off(qkvg, 3 * C), ldmul=4 * C, res=z, a_amax=self.o_bound(bnd))

    def triangle_block(self, prefix, z, T, C, mask, maskT):
        """layers/transformers.py:48-54.  The reference transposes z for the column variants but NOT the mask
        (attentions.py:158-162,195,208), i.e. pair (i,j) of the original layout sees mask[j,i]: `maskT`."""
        self.triangle_update(prefix + ".triangle_row_update", z, T, C, mask, False)
        self.triangle_update(prefix + ".triangle_col_update", z, T, C, maskT, True)
        self.triangle_attention(prefix + ".triangle_row_attention", z, T, C, mask, False)
        self.triangle_attention(prefix + ".triangle_col_attention", z, T, C, maskT, True)
        self.transition(prefix + ".pair_transition", z, T * T, C)

    def atom_transformer(self, prefix, a, ap, A, Ca, Cap, ap_mask, no_blocks):
        """AtomTransformer (layers/transformers.py:25-36): a is updated in place through the blocks' residuals"""
        P = self.P
        abias = self.ws.get("atom_bias", ops.bias_frag_numel(Ca // 32, A, A), zero=True)
        for b in range(no_blocks):
            blk = f"{prefix}.blocks.{b}"
            ps = self.trunk_prescale(blk + ".attention", P[blk + ".attention.norm_s.weight"], 1, A, self.Ar, Ca // 32, strides=(A * 4 * Ca, 4 * Ca))
            self.pair_bias(blk + ".attention", ap, A, A, Cap, ap_mask, P[blk + ".attention.norm_z.weight"], abias, prescale=ps)
            self.attention_pair_bias(blk + ".attention", a, 1, A, Ca, abias, nk=self.Ar, bias_prescale=ps)
            self.transition(blk + ".transition", a, A, Ca)

    def pairformer(self, prefix, s, z, T, Cs, Cz, z_mask, z_maskT, no_blocks):
        """Pairformer (layers/transformers.py:124-146): s and z are updated in place"""
        P = self.P
        sbias = self.ws.get("single_bias", ops.bias_frag_numel(Cs // 32, T, T), zero=True)
        for b in range(no_blocks):
            blk = f"{prefix}.blocks.{b}"
            self.triangle_block(blk, z, T, Cz, z_mask, z_maskT)
            ps = self.trunk_prescale(blk + ".attention", P[blk + ".attention.norm_s.weight"], 1, T, self.Tr, Cs // 32, strides=(T * 4 * Cs, 4 * Cs))
            self.pair_bias(blk + ".attention", z, T, T, Cz, z_mask, P[blk + ".attention.norm_z.weight"], sbias, prescale=ps)
            self.attention_pair_bias(blk + ".attention", s, 1, T, Cs, sbias, nk=self.Tr, bias_prescale=ps)
            self.transition(blk + ".transition", s, T, Cs)
            if self.trunk_probe is not None:
                self.trunk_probe(f"pairformer.{b}.s", s.view(T, Cs))
                self.trunk_probe(f"pairformer.{b}.z", z.view(T, T, Cz))

    # ------------------------------------------------------------------ conditioning trunk
    trunk_probe = None    # diagnostics: callable(name, tensor view) invoked after every trunk block (tests/test_trunk_pins_gpu.py)

    def conditioning(self, batch, s_pool=None):
        """DiffusionConditioning.forward (diffusion_conditioning.py:232-238) -> a, ap, s, z (workspace tensors).

        `s_pool` (diagnostics / parity budget only): a replacement for the pooled atom activations, the output of the reference's
        `TokenEmbedder.downscale` (:168-176).  The reference pools by cumsum over all atoms + diff, whose fp32 prefixes (|C| up
        to 1800 for pooled sums of ~4) carry a rounding that no implementation can reproduce unless its inputs are bit-identical
        (tools/pool_noise_cpu.py); injecting the reference's own pooled tensor separates that from everything else."""
        P, ws, eps = self.P, self.ws, self.eps
        dc = self.cfg.model.diffusion_conditioning
        Ca, Cap, Cs, Cm, Cz = dc.c_a, dc.c_ap, dc.c_s, dc.c_m, dc.c_z
        A = batch["ref_pos"].shape[0]
        T = batch["target_feat"].shape[0]
        S = batch["msa_feat"].shape[0]
        a2t = batch["atom_id_to_token_id"]
        # padded counts size every row dimension; REAL counts bound every reduction (attention keys, the
        # triangle-multiplication sum), so padding is exactly inert - also for fully masked query rows, which
        # the reference's -1e9 mask turns into a uniform softmax over the real keys (tensor_utils.py:642-646)
        self.Ar, self.Tr = batch.get("_A_real", A), batch.get("_T_real", T)
        ap_mask = batch["ap_mask"]
        z_mask = batch["z_mask"]
        z_maskT = z_mask.t().contiguous()          # layout copy of an input mask (see triangle_block)
        pre = "diffusion_conditioning"

        # ---------------- AtomEmbedder (:110-128)
        ae = pre + ".atom_embedder"
        a = ws.get("a", A, Ca)
        self.lin(batch["ref_feat"], ae + ".linear_c", A, out=a, lda=batch["ref_feat"].shape[1])
        cl = self.lin(a, ae + ".linear_c_l", A, pro_act=ACT_RELU)
        cm = self.lin(a, ae + ".linear_c_m", A, pro_act=ACT_RELU)
        ap = ws.get("ap", A * A, Cap)
        ops.check(ops._lib.init().pd_atom_pair_init(
            ops.ptr(batch["ref_pos"]), ops.ptr(batch["ref_space_uid"]), ops.ptr(cl), ops.ptr(cm),
            ops.ptr(P[ae + ".linear_p.weight"]), ops.ptr(P[ae + ".linear_d.weight"]), ops.ptr(P[ae + ".linear_v.weight"]),
            ops.ptr(ap), A, Cap, ops.stream()), "pd_atom_pair_init")
        # ap += FFN(ap) (no norm): one fused pass for the model's shapes (c_ap = 16 -> 128 -> 16); otherwise two GEMMs,
        # chunked over rows so that the hidden tile stays cache-sized
        W13, hidden = P.glu(ae + ".ffn")
        rc = ops._lib.init().pd_atom_pair_ffn(ops.ptr(ap), ops.ptr(P[ae + ".ffn.w1.weight"]), ops.ptr(P[ae + ".ffn.w3.weight"]),
                                              ops.ptr(P[ae + ".ffn.w2.weight"]), A * A, Cap, hidden, ops.stream())
        if rc == -3:         # PD_ERR_UNSUPPORTED: shapes outside the fused kernel
            W2, _, _, _, ldw2 = P.linear(ae + ".ffn.w2")
            chunk = min(A * A, 1 << 20)
            h = ws.get("ap_ffn_h", chunk, hidden)
            for r0 in range(0, A * A, chunk):
                rows = min(chunk, A * A - r0)
                self.gemm(off(ap, r0 * Cap), W13, h, rows, 2 * hidden, Cap, glu=1)
                self.gemm(h, W2, off(ap, r0 * Cap), rows, Cap, hidden, ldw=ldw2, res=off(ap, r0 * Cap), ldres=Cap)
        else:
            ops.check(rc, "pd_atom_pair_ffn")
        self.atom_transformer(ae + ".atom_transformer", a, ap, A, Ca, Cap, ap_mask, dc.no_blocks_atom)
        if self.trunk_probe is not None:
            self.trunk_probe("atom_embedder.a", a.view(A, Ca))
            self.trunk_probe("atom_embedder.ap", ap.view(A, A, Cap))

        # ---------------- TokenEmbedder (:178-202)
        te = pre + ".token_embedder"
        u = self.lin(a, te + ".linear_a", A, act=ACT_SILU)
        tok_start = batch["_tok_start"]
        s = ws.get("s", T, Cs)
        L = ops._lib.init()
        ops.check(L.pd_segment_pool(ops.ptr(u), ops.ptr(tok_start), None, ops.ptr(s), 1, A, T, Cs, ops.stream()), "pool")
        if self.trunk_probe is not None:
            self.trunk_probe("s_pool", s.view(T, Cs))
        if s_pool is not None:
            s.view(T, Cs)[:s_pool.shape[0]].copy_(s_pool.to(device=s.device, dtype=s.dtype))
        self.lin(batch["target_feat"], te + ".linear_target_feat", T, out=s, lda=batch["target_feat"].shape[1], res=s)
        self.lin(batch["key_res_feat"], te + ".linear_key_res_feat", T, out=s, lda=batch["key_res_feat"].shape[1], res=s)
        self.lin(batch["pocket_res_feat"], te + ".linear_pocket_res_feat", T, out=s, lda=1, res=s)
        si = self.lin(s, te + ".linear_s_i", T)
        sj = self.lin(s, te + ".linear_s_j", T)
        z = ws.get("z", T * T, Cz)
        ops.check(L.pd_pair_init_z(ops.ptr(si), ops.ptr(sj), ops.ptr(P.relpos_T()), ops.ptr(P[te + ".linear_bonds.weight"]),
                                   ops.ptr(batch["asym_id"]), ops.ptr(batch["sym_id"]), ops.ptr(batch["entity_id"]),
                                   ops.ptr(batch["residue_index"]), ops.ptr(batch["rel_tok_feat"]),
                                   ops.ptr(batch["token_bonds_feature"]), ops.ptr(z), T, Cz, ops.stream()), "pair_init_z")
        sm = self.lin(s, te + ".linear_s_input", T)
        m = ws.get("m", S * T, Cm)
        self.lin(batch["msa_feat"], te + ".linear_msa_feat", S * T, out=m, lda=batch["msa_feat"].shape[2], res=sm,
                 res_row_mod=T)

        Hm = Cm // 32
        mbias = ws.get("msa_bias", ops.bias_frag_numel(Hm, T, T), zero=True)
        for b in range(dc.no_blocks_evoformer):
            blk = f"{te}.evoformer.blocks.{b}"
            # MSA row attention with pair bias (attentions.py:76-97)
            ps = self.trunk_prescale(blk + ".msa_row_attention", P[blk + ".msa_row_attention.norm_m.weight"], S, T, self.Tr, Hm, strides=(T * 4 * Cm, 4 * Cm))
            self.pair_bias(blk + ".msa_row_attention", z, T, T, Cz, z_mask, P[blk + ".msa_row_attention.norm_z.weight"], mbias, prescale=ps)
            self.attention_pair_bias(blk + ".msa_row_attention", m, S, T, Cm, mbias, norm_name="norm_m", nk=self.Tr, bias_prescale=ps)
            self.msa_column_attention(blk + ".msa_col_attention", m, S, T, Cm)
            self.transition(blk + ".msa_transition", m, S * T, Cm)
            self.outer_product_mean(blk + ".opm", m, z, S, T, Cm, Cz)
            self.triangle_block(blk, z, T, Cz, z_mask, z_maskT)
            if self.trunk_probe is not None:
                self.trunk_probe(f"evoformer.{b}.m", m.view(S, T, Cm))
                self.trunk_probe(f"evoformer.{b}.z", z.view(T, T, Cz))

        # ---------------- TemplatePairEmbedder (:38-50)
        tp = te + ".template_pair_embedder"
        tmask = ws.get("templ_mask", T * T)
        D = batch["templ_feat"].shape[-1]
        ops.check(L.pd_template_mask(ops.ptr(z_mask), ops.ptr(batch["templ_feat"]), ops.ptr(batch["asym_id"]), ops.ptr(tmask),
                                     T, D, ops.stream()), "template_mask")
        uu = ws.get("templ_u", T * T, Cz)
        st = self.stats(z, T * T, Cz, RMS, 1e-6)
        self.lin(z, tp + ".linear_in", T * T, out=uu, stats=st, pro_w=P[tp + ".norm_in.weight"])
        self.lin(batch["templ_feat"], tp + ".linear_templ_feat", T * T, out=uu, res=uu)
        tmaskT = tmask.reshape(T, T).t().contiguous().reshape(-1)
        for b in range(2):
            self.triangle_block(f"{tp}.triangleformer.blocks.{b}", uu, T, Cz, tmask, tmaskT)
        st = self.stats(uu, T * T, Cz, RMS, eps)
        tpo = self.lin(uu, tp + ".linear_out", T * T, stats=st, pro_w=P[tp + ".norm_out.weight"], pro_act=ACT_RELU)
        ops.check(L.pd_axpby(ops.ptr(z), ops.ptr(z), 1.0, ops.ptr(tpo), ops.ptr(batch["t_mask"]), 1.0, T * T * Cz,
                             ops.stream()), "axpby")
        if self.trunk_probe is not None:      # the embedder's own output (the addend), as the reference module returns it
            self.trunk_probe("template.z", tpo.view(T, T, Cz) * batch["t_mask"].to(tpo.dtype).reshape(-1)[0])

        # ---------------- single representation + Pairformer
        s2 = ws.get("s2", T, Cs)
        self.lin(m, te + ".linear_m", T, out=s2)                  # m[0] = first T rows
        self.lin(s, te + ".linear_s", T, out=s2, res=s2)
        s = s2
        self.pairformer(te + ".pairformer", s, z, T, Cs, Cz, z_mask, z_maskT, dc.no_blocks_pairformer)

        # ---------------- tail (:236-237)
        st = self.stats(s, T, Cs, RMS, eps)
        ta = self.lin(s, pre + ".linear_s", T, stats=st, pro_w=P[pre + ".norm_s.weight"])
        ops.check(L.pd_gather_rows_add(ops.ptr(a), ops.ptr(ta), ops.ptr(a2t), A, Ca, ops.stream()), "gather_rows_add")
        st = self.stats(z, T * T, Cz, RMS, eps)
        zt = self.lin(z, pre + ".linear_z", T * T, stats=st, pro_w=P[pre + ".norm_z.weight"])
        ops.check(L.pd_pair_gather_add(ops.ptr(ap), ops.ptr(zt), ops.ptr(a2t), A, T, Cap, ops.stream()), "pair_gather_add")
        return a, ap, s, z

    # ------------------------------------------------------------------ confidence head
    def confidence(self, batch, s_in, z_in, x_pred, dims, pre="confidence_module"):
        """ConfidenceModule.forward (layers/confidence_module.py:56-88) -> p_pae [T,T,c_pae], p_pde [T,T,c_pde],
        p_plddt [A,c_plddt] (fresh tensors).  s_in [T,c_s], z_in [T*T,c_z] and x_pred [A,3] (the first predicted pose) are
        read only; `dims` carries c_a c_ap c_s c_z no_blocks_heads no_blocks_atom."""
        P, ws = self.P, self.ws
        Ca, Cap, Cs, Cz = dims["c_a"], dims["c_ap"], dims["c_s"], dims["c_z"]
        T, A = s_in.shape[0], x_pred.shape[0]
        self.Ar, self.Tr = batch.get("_A_real", A), batch.get("_T_real", T)
        z_mask = batch["z_mask"]
        z_maskT = z_mask.t().contiguous()
        L = ops._lib.init()
        sp = ops.stream()
        # z = z + linear_s_i(s)[:, None] + linear_s_j(s)[None, :] + linear_d(one_hot(d))                     (:68-72)
        si = self.lin(s_in, pre + ".linear_s_i", T)
        sj = self.lin(s_in, pre + ".linear_s_j", T)
        z = ws.get("conf_z", T * T, Cz)
        WdT = P._c(("conf_WdT", pre), lambda: P[pre + ".linear_d.weight"].t().contiguous())
        ops.check(L.pd_confidence_pair_init(ops.ptr(z_in), ops.ptr(si), ops.ptr(sj), ops.ptr(WdT), ops.ptr(x_pred),
                                            ops.ptr(batch["token_id_to_centre_atom_id"]), ops.ptr(z), T, Cz, sp), "confidence_pair_init")
        s = ws.get("conf_s", T, Cs)
        s.copy_(s_in)
        self.pairformer(pre + ".pairformer", s, z, T, Cs, Cz, z_mask, z_maskT, dims["no_blocks_heads"])      # (:74)
        zs = ws.get("conf_zs", T * T, Cz)
        ops.check(L.pd_pair_symmetrize(ops.ptr(z), ops.ptr(zs), T, Cz, sp), "pair_symmetrize")               # (:75)
        n_pae = P[pre + ".linear_pae.weight"].shape[0]
        n_pde = P[pre + ".linear_pde.weight"].shape[0]
        p_pae = self.lin(zs, pre + ".linear_pae", T * T, out=torch.empty(T * T, n_pae, device=self.device))  # (:76-77)
        p_pde = self.lin(zs, pre + ".linear_pde", T * T, out=torch.empty(T * T, n_pde, device=self.device))
        # a = linear_s_a(s)[atom_id_to_token_id];  ap = linear_z_a(|x_i - x_j|)                              (:79-80)
        ta = self.lin(s, pre + ".linear_s_a", T)
        a0 = ws.get("conf_a0", A, Ca)
        a0.zero_()
        ops.check(L.pd_gather_rows_add(ops.ptr(a0), ops.ptr(ta), ops.ptr(batch["atom_id_to_token_id"]), A, Ca, sp), "gather_rows_add")
        ap = ws.get("conf_ap", A * A, Cap)
        ops.check(L.pd_atom_dist_embed(ops.ptr(x_pred), ops.ptr(P[pre + ".linear_z_a.weight"]), ops.ptr(P[pre + ".linear_z_a.bias"]),
                                       ops.ptr(ap), A, Cap, sp), "atom_dist_embed")
        a = ws.get("conf_a", A, Ca)
        a.copy_(a0)
        self.atom_transformer(pre + ".atom_transformer", a, ap, A, Ca, Cap, batch["ap_mask"], dims["no_blocks_atom"])
        ops.check(L.pd_axpby(ops.ptr(a), ops.ptr(a0), 1.0, ops.ptr(a), None, 1.0, A * Ca, sp), "axpby")      # a + AT(a) (:82-84)
        n_pl = P[pre + ".linear_plddt.weight"].shape[0]
        p_plddt = self.lin(a, pre + ".linear_plddt", A, out=torch.empty(A, n_pl, device=self.device))         # (:86)
        return p_pae.reshape(T, T, n_pae), p_pde.reshape(T, T, n_pde), p_plddt

    def rows_batchable(self, x, wname, out, rows, n):
        """May the plain Linear `wname` over n stacked groups of `rows` rows run as ONE launch and still give every group the bits
        of its own launch?  Yes when the library picks the same kernel for both row counts (pd_gemm_variant) and a group consists
        of whole row tiles of that kernel: pd_gemm sends a ragged row remainder to its general kernel, so a group that ends inside
        a tile would see its last rows on another kernel than alone.  Long-K launches of few rows may be K-split (Engine.gemm),
        which depends on the row count: those stay one launch per group."""
        if n == 1:
            return True
        W, b, N, K, ldw = self.P.linear(wname)
        if K >= 256:
            return False
        v1, vn = (self.gemm(x, W, out, m, N, K, lda=K, ldw=ldw, bias=b, query_only=True) for m in (rows, n * rows))
        tile = 64 if (v1 % 1000) // 100 == 3 else 128
        return v1 >= 0 and v1 == vn and rows % tile == 0

    def lin_groups(self, x, wname, out, rows, n):
        """Linear `wname` over x [n * rows, K] -> out [n * rows, N]: one launch where rows_batchable, else one per group"""
        if self.rows_batchable(x, wname, out, rows, n):
            self.lin(x, wname, n * rows, out=out)
            return 1
        N, K = out.shape[-1], x.shape[-1]
        for q in range(n):
            self.lin(off(x, q * rows * K), wname, rows, out=off(out, q * rows * N))
        return n

    def confidence_poses(self, batch, s_in, z_in, x, dims, chunk, sink, pre="confidence_module"):
        """ConfidenceModule.forward for every pose of x [P,A,3] (ConfidenceModule.forward_poses / score_poses): per pose the bits of
        `confidence(batch, s_in, z_in, x[p])`.  The logits of at most `chunk` poses exist at a time, in workspace buffers that are
        reused from chunk to chunk and from call to call; `sink(p0, n, p_pae [n,T*T,c_pae], p_pde [n,T*T,c_pde], p_plddt
        [n,A,c_plddt])` consumes each chunk (views of those buffers: it must copy or reduce them before it returns).
        Once per call: linear_s_i / linear_s_j of s, the transposed pair mask, the packed linear_d table.  Once per chunk: the
        entry z of all its poses from ONE read of z_in, s_i, s_j (pd_confidence_pair_init_poses), the atom-pair distance
        embedding (pd_atom_dist_embed_poses), z + z^T, the two pair heads and linear_plddt over the chunk's rows (lin_groups).
        Per pose: the Pairformer and AtomTransformer stacks, on the trunk's entry points as `confidence` runs them, and the
        linear_s_a gather (it reads s AFTER the Pairformer, which depends on the pose through z)."""
        P, ws = self.P, self.ws
        Ca, Cap, Cs, Cz = dims["c_a"], dims["c_ap"], dims["c_s"], dims["c_z"]
        T, A, NP = s_in.shape[0], x.shape[1], x.shape[0]
        self.Ar, self.Tr = batch.get("_A_real", A), batch.get("_T_real", T)
        z_mask = batch["z_mask"]
        z_maskT = z_mask.t().contiguous()
        L = ops._lib.init()
        sp = ops.stream()
        si = self.lin(s_in, pre + ".linear_s_i", T)
        sj = self.lin(s_in, pre + ".linear_s_j", T)
        WdT = P._c(("conf_WdT", pre), lambda: P[pre + ".linear_d.weight"].t().contiguous())
        n_pae, n_pde, n_pl = (P[f"{pre}.linear_{k}.weight"].shape[0] for k in ("pae", "pde", "plddt"))
        chunk = max(1, min(int(chunk), NP))
        z = ws.get("confp_z", chunk, T * T, Cz)
        zs = ws.get("confp_zs", chunk, T * T, Cz)
        s = ws.get("confp_s", chunk, T, Cs)
        a0 = ws.get("confp_a0", chunk, A, Ca)
        a = ws.get("confp_a", chunk, A, Ca)
        ap = ws.get("confp_ap", chunk, A * A, Cap)
        p_pae = ws.get("confp_pae", chunk, T * T, n_pae)
        p_pde = ws.get("confp_pde", chunk, T * T, n_pde)
        p_plddt = ws.get("confp_plddt", chunk, A, n_pl)
        a2t, ctr = batch["atom_id_to_token_id"], batch["token_id_to_centre_atom_id"]
        for p0 in range(0, NP, chunk):
            n = min(chunk, NP - p0)
            xc = x[p0:p0 + n]
            ops.check(L.pd_confidence_pair_init_poses(ops.ptr(z_in), ops.ptr(si), ops.ptr(sj), ops.ptr(WdT), ops.ptr(xc), ops.ptr(ctr),
                                                      ops.ptr(z), T, Cz, n, 3 * A, sp), "confidence_pair_init_poses")     # (:68-72)
            s[:n].copy_(s_in[None].expand(n, T, Cs))
            for q in range(n):
                self.pairformer(pre + ".pairformer", s[q], z[q], T, Cs, Cz, z_mask, z_maskT, dims["no_blocks_heads"])     # (:74)
            ops.check(L.pd_pair_symmetrize_poses(ops.ptr(z), ops.ptr(zs), T, Cz, n, sp), "pair_symmetrize_poses")         # (:75)
            self.lin_groups(zs, pre + ".linear_pae", p_pae, T * T, n)                                                      # (:76-77)
            self.lin_groups(zs, pre + ".linear_pde", p_pde, T * T, n)
            a0[:n].zero_()
            for q in range(n):                                                                                             # (:79)
                ta = self.lin(s[q], pre + ".linear_s_a", T)
                ops.check(L.pd_gather_rows_add(ops.ptr(a0[q]), ops.ptr(ta), ops.ptr(a2t), A, Ca, sp), "gather_rows_add")
            ops.check(L.pd_atom_dist_embed_poses(ops.ptr(xc), ops.ptr(P[pre + ".linear_z_a.weight"]), ops.ptr(P[pre + ".linear_z_a.bias"]),
                                                 ops.ptr(ap), A, Cap, n, 3 * A, sp), "atom_dist_embed_poses")             # (:80)
            a[:n].copy_(a0[:n])
            for q in range(n):
                self.atom_transformer(pre + ".atom_transformer", a[q], ap[q], A, Ca, Cap, batch["ap_mask"], dims["no_blocks_atom"])
            ops.check(L.pd_axpby(ops.ptr(a), ops.ptr(a0), 1.0, ops.ptr(a), None, 1.0, n * A * Ca, sp), "axpby")           # (:82-84)
            self.lin_groups(a, pre + ".linear_plddt", p_plddt, A, n)                                                       # (:86)
            sink(p0, n, p_pae[:n], p_pde[:n], p_plddt[:n])

    @staticmethod
    def confidence_pose_bytes(T, A, dims, n_pae=64, n_pde=64, n_pl=50):
        """workspace bytes confidence_poses needs per pose of a chunk (the buffers listed there)"""
        return 4 * (T * T * (2 * dims["c_z"] + n_pae + n_pde) + T * dims["c_s"] + A * (2 * dims["c_a"] + n_pl) + A * A * dims["c_ap"])

    def msa_column_attention(self, prefix, m, S, T, C):
        """m += MSAColumnAttention(m): attention along the MSA-row axis, no bias (attentions.py:117-136)"""
        P = self.P
        rows = S * T
        H = C // 32
        st = self.stats(m, rows, C, RMS, self.eps)
        W, b = P.qkvg(prefix)
        qkvg = self.ws.get("qkvg", rows, 4 * C)
        self.gemm(m, W, qkvg, rows, 4 * C, C, stats=st, pro_w=P[prefix + ".norm_m.weight"], bias=b)
        o = self.ws.get("attn_o", rows, C)
        st4 = (4 * C, T * 4 * C)
        ops.attention(off(qkvg, 0), off(qkvg, C), off(qkvg, 2 * C), o, nq=S, nk=S, nbatch=T, nheads=H,
                      q_strides=st4, k_strides=st4, v_strides=st4, o_strides=(C, T * C), bias=None,
                      f16_amax=(bnd := self.trunk_attn_bounds(prefix, P[prefix + ".norm_m.weight"])))
        Wo, bo, _, _, ldw = P.linear(prefix + ".linear_o")
        self.gemm(o, Wo, m, rows, C, C, ldw=ldw, bias=bo, mul=off(qkvg, 3 * C), ldmul=4 * C, res=m, a_amax=self.o_bound(bnd))

    def outer_product_mean(self, prefix, m, z, S, T, Cm, Cz):
        """z += RMSNorm(W_o . sum_s q_s (x) k_s + b)                       (outer_product_mean.py:23-31)"""
        P = self.P
        rows = S * T
        st = self.stats(m, rows, Cm, RMS, self.eps)
        nw = P[prefix + ".norm_in.weight"]
        q = self.lin(m, prefix + ".linear_q", rows, stats=st, pro_w=nw)
        k = self.lin(m, prefix + ".linear_k", rows, stats=st, pro_w=nw)
        outer = self.ws.get("opm_outer", T * T, 1024)
        self.gemm(q, k, outer, T * 32, T * 32, S, a_kmajor=True, w_kmajor=True, lda=T * 32, ldw=T * 32,
                 out_mode=OUT_OPM, T2=T)
        raw = self.lin(outer, prefix + ".linear_o", T * T)
        ops.rownorm(raw, z, T * T, Cz, res=z, w=P[prefix + ".norm_out.weight"], mode=RMS, eps=self.eps)

    # ------------------------------------------------------------------ denoiser
    def prepare_dit(self, a, ap, s, z, batch, tau, per_sample=False, B=0):
        """Per-call, step-invariant preparation: hoisted pair biases (attentions.py:246,254 executed once
        instead of 18 x steps times) and the AdaLN tables of every step (adaptive_layer_norm_zero.py:19)."""
        P, ws = self.P, self.ws
        dt = self.cfg.model.dit
        Ca, Cs = dt.c_a, dt.c_s
        A, T = a.shape[0], s.shape[0]
        # --- hoisted biases (times the product of the q, k operand scales when the step loop's launches - B samples - take the
        # pipelined attention kernel: attn_prescale)
        Ar, Tr = batch.get("_A_real", A), batch.get("_T_real", T)
        f16 = ops.SPLIT_GEMM and ops.F16_GEMM
        ps_a = self.attn_prescale(P.dit_qk_bounds_host("atom"), B, A, Ar, Ca // 32, self.attn_ws(B, A, Ar, Ca // 32), strides=(A * 3 * Ca, 3 * Ca)) if (B and f16 and "atom" not in self.f16_off) else 0.0
        ps_t = self.attn_prescale(P.dit_qk_bounds_host("token"), B, T, Tr, Cs // 32, self.attn_ws(B, T, Tr, Cs // 32), strides=(T * 3 * Cs, 3 * Cs)) if (B and f16 and "token" not in self.f16_off) else 0.0
        osc_a, osc_t = LOG2E * (ps_a or 1.0), LOG2E * (ps_t or 1.0)
        na, nt = P.dit_bias("atom")[2], P.dit_bias("token")[2]
        fa = ws.get("dit_atom_bias", ops.bias_frag_numel(na, A, A), zero=True)
        ft = ws.get("dit_token_bias", ops.bias_frag_numel(nt, T, T), zero=True)
        self._dit_biases(ap, z, batch, A, T, fa, ft, osc_a, osc_t)
        tab_a, tab_t, bnd = self._dit_tables(tau, per_sample)
        return {"atom_bias": fa, "token_bias": ft, "tab_atom": tab_a, "tab_token": tab_t, "bnd_atom": bnd["atom"],
                "bnd_token": bnd["token"], "ps_atom": ps_a, "ps_token": ps_t, "B": B}

    def _dit_biases(self, ap, z, batch, A, T, fa, ft, osc_a, osc_t):
        """the hoisted atom / token pair biases of the DiT blocks of one system, in fragment layout (x log2 e x the pre-scale)"""
        P = self.P
        dt = self.cfg.model.dit
        Cap, Cz = dt.c_ap, dt.c_z
        Wa, ba_, na = P.dit_bias("atom")                  # [2*nb_atom*H, Cap] with LN affine folded
        if not (Wa.shape[1] == Cap and ops.pair_bias(ap, Wa, fa, A, A, Cap, na, c2=ba_, maskadd=batch["ap_mask"],
                                                      maskval=-self.inf, out_scale=osc_a, mode=LN, eps=1e-5,
                                                      only_if_faster=True)):
            st = self.stats(ap, A * A, Cap, LN, 1e-5, "stats_pb")
            self.gemm(ap, Wa, fa, A * A, na, Cap, stats=st, bias=ba_, out_mode=OUT_BIASFRAG, T1=A, T2=A,
                      maskadd=batch["ap_mask"], maskval=-self.inf, out_scale=osc_a)
        Wt, bt_, nt = P.dit_bias("token")
        st = self.stats(z, T * T, Cz, LN, 1e-5, "stats_pb")
        self.gemm(z, Wt, ft, T * T, nt, Cz, stats=st, bias=bt_, out_mode=OUT_BIASFRAG, T1=T, T2=T,
                  maskadd=batch["z_mask"], maskval=-self.inf, out_scale=osc_t)

    def _dit_tables(self, tau, per_sample=False):
        """AdaLN tables of every step and the magnitude bounds derived from them: functions of the noise levels only"""
        P, ws = self.P, self.ws
        dt = self.cfg.model.dit
        Ca, Cs = dt.c_a, dt.c_s
        n = tau.shape[0]
        L = ops._lib.init()
        # --- AdaLN tables: t = MLP(sincos(tau)); table = Linear(silu(t)) with 1 folded into the scale bias
        emb = ws.get("t_emb", n, 256)
        ops.check(L.pd_timestep_embed(ops.ptr(tau), ops.ptr(emb), n, ops.stream()), "timestep_embed")
        t1 = self.lin(emb, "dit.time_embedder.timestep_embedder.linear_1", n, act=ACT_SILU)
        t = self.lin(t1, "dit.time_embedder.timestep_embedder.linear_2", n)
        Wta, bta = P.adaln("atom")
        Wtt, btt = P.adaln("token")
        tab_a = ws.get("adaln_atom", n, Wta.shape[0])
        tab_t = ws.get("adaln_token", n, Wtt.shape[0])
        self.gemm(t, Wta, tab_a, n, Wta.shape[0], 256, bias=bta, pro_act=ACT_SILU)
        self.gemm(t, Wtt, tab_t, n, Wtt.shape[0], 256, bias=btt, pro_act=ACT_SILU)
        # --- magnitude bounds of every block's activations at every step, from the tables alone (two-part fp16 operand format)
        bnd = {}
        for kind, tab, C in (("atom", tab_a, Ca), ("token", tab_t, Cs)):
            consts = P.dit_bound_consts(kind)
            nb = consts.shape[0]
            out = ws.get("dit_bounds_" + kind, n, nb, 8)
            wstack, hidden = P.dit_bound_weights(kind)
            vh = ws.get("dit_bounds_vh_" + kind, n, nb, 2)
            ops.check(L.pd_dit_bounds(ops.ptr(tab), n, tab.shape[1], nb, C, hidden, ops.ptr(consts), ops.ptr(wstack), ops.ptr(vh),
                                      ops.ptr(out), ops.stream()), "dit_bounds")
            if per_sample:                  # rows = samples of ONE launch (training-time forward): the launch needs the largest
                out.copy_(out.amax(0, keepdim=True).expand_as(out))
            bnd[kind] = out
        return tab_a, tab_t, bnd

    def prepare_dit_many(self, cond_of, batches, tau, B):
        """prepare_dit for G systems of one padded shape sampled together (PhysDock.sample_diffusion_many).  cond_of(g) -> the
        (a, ap, s, z) of system g, consumed before the next one is asked for (the trunk's outputs are shape-keyed workspace buffers):
        its hoisted biases go into slot g of stacked [G][fragments] buffers, its a / s into stacked [G][A][c_a] / [G][T][c_s]
        buffers (prep["a"] / prep["s"]).  The AdaLN tables and bounds depend on the schedule only and are built once.  The pre-scale
        is decided for the launch that really runs: G B batches, the group's largest real key count."""
        P, ws = self.P, self.ws
        dt = self.cfg.model.dit
        Ca, Cs = dt.c_a, dt.c_s
        G = len(batches)
        A, T = batches[0]["ref_pos"].shape[0], batches[0]["target_feat"].shape[0]
        Ar = max(b.get("_A_real", A) for b in batches)
        Tr = max(b.get("_T_real", T) for b in batches)
        nb = G * B
        f16 = ops.SPLIT_GEMM and ops.F16_GEMM
        ps_a = self.attn_prescale(P.dit_qk_bounds_host("atom"), nb, A, Ar, Ca // 32, self.attn_ws(nb, A, Ar, Ca // 32), strides=(A * 3 * Ca, 3 * Ca)) if (B and f16 and "atom" not in self.f16_off) else 0.0
        ps_t = self.attn_prescale(P.dit_qk_bounds_host("token"), nb, T, Tr, Cs // 32, self.attn_ws(nb, T, Tr, Cs // 32), strides=(T * 3 * Cs, 3 * Cs)) if (B and f16 and "token" not in self.f16_off) else 0.0
        osc_a, osc_t = LOG2E * (ps_a or 1.0), LOG2E * (ps_t or 1.0)
        na, nt = P.dit_bias("atom")[2], P.dit_bias("token")[2]
        ga, gt = ops.bias_frag_numel(na, A, A), ops.bias_frag_numel(nt, T, T)
        fa = ws.get("dit_atom_bias_g", G, ga, zero=True)
        ft = ws.get("dit_token_bias_g", G, gt, zero=True)
        a_g = ws.get("grp:a", G, A, Ca)
        s_g = ws.get("grp:s", G, T, Cs)
        for g, b in enumerate(batches):
            a, ap, s, z = cond_of(g)
            self._dit_biases(ap, z, b, A, T, fa[g], ft[g], osc_a, osc_t)
            a_g[g].copy_(a.reshape(A, Ca))
            s_g[g].copy_(s.reshape(T, Cs))
        tab_a, tab_t, bnd = self._dit_tables(tau)
        return {"atom_bias": fa, "token_bias": ft, "tab_atom": tab_a, "tab_token": tab_t, "bnd_atom": bnd["atom"],
                "bnd_token": bnd["token"], "ps_atom": ps_a, "ps_token": ps_t, "B": nb, "G": G, "gstride_atom": ga, "gstride_token": gt,
                "a": a_g, "s": s_g}

    def dit_block(self, prefix, x, B, N, C, bias, tab, tab_off, tab_ld, per_sample, nk, bnd=None, bias_prescale=0.0, rows_alloc=0,
                  gkw=None):
        """DiTBlock (transformers.py:155-159; attentions.py:241-265; transitions.py:27-30).
        tab: AdaLN table row(s) [shift | 1+scale | gate] x (attention, transition) for this block.
        rows_alloc: rows x is allocated with (>= B N, see af3_dit): every row-wise launch of the block then covers that many rows -
        whole 64-row tiles - and the rows past B N hold garbage nobody reads (the attention addresses rows by (sample, position)).
        gkw: the group fields of a launch over several systems (af3_dit(grp=)): bias set and real key count per run of samples."""
        P, eps = self.P, self.eps
        rows = rows_alloc or B * N
        H = C // 32
        grp = dict(pro_rows_per_group=N, pro_gstride=tab_ld) if per_sample else {}
        mgrp = dict(mul_rows_per_group=N if per_sample else rows, mul_gstride=tab_ld if per_sample else 0)
        # wide rows (token DiT, C = 512) in chip-filling launches: AdaLN-normalise and split the activations ONCE
        # (pd_norm_split) instead of in every column block of the projection that consumes them (12 / 22 of them)
        W13, hidden = P.glu(prefix + ".transition.feed_forward")
        # magnitude bounds of this block's GEMM operands (pd_dit_bounds: [q, k, v = o, y, y', h]) -> two-part fp16 operands
        f16 = ops.SPLIT_GEMM and ops.F16_GEMM and bnd is not None
        b_o, b_y, b_y2, b_h = (bnd + 8, bnd + 12, bnd + 16, bnd + 20) if f16 else (None,) * 4
        # wide rows (token DiT, C = 512) in chip-filling launches: AdaLN-normalise and split the activations ONCE
        # (pd_norm_split / pd_norm_split2) instead of in every column block of the projection that consumes them (12 / 22 of them)
        # (narrow atom rows, C = 128, keep the in-kernel prologue: ops.PRESPLIT_MIN_C_F16)
        presplit = ops.SPLIT_GEMM and ops.PRESPLIT_GEMM and C >= (ops.PRESPLIT_MIN_C_F16 if f16 else 256) and C % 32 == 0 \
            and ops.presplit_supported(rows, 3 * C, C, hn=True, f16=f16) and ops.presplit_supported(rows, 2 * hidden, C, glu=1, f16=f16)
        a3 = a2 = None
        if presplit and f16:
            a2 = self.lws("dit_a2", 2, rows, C, dtype=torch.float16)
        elif presplit:
            a3 = self.lws("dit_a3", 3, rows, C, dtype=torch.bfloat16)
        ng = dict(rows_per_group=N if per_sample else 0, gstride=tab_ld if per_sample else 0)

        def norm_split(w_off, amax):
            kw_ = dict(mode=LN, eps=eps, b=off(tab, w_off), w=off(tab, w_off + C), **ng)
            if a2 is not None:
                ops.norm_split2(x, a2, rows, C, amax, **kw_)
                return dict(A2=a2)
            ops.norm_split(x, a3, rows, C, **kw_)
            return dict(A3=a3)
        qkv = self.lws("dit_qkv", rows, 3 * C)
        hn = dict(hn_w=P.headnorm(prefix + ".attention"), hn_cols=2 * C, hn_split=C, hn_eps=eps)
        st3 = (N * 3 * C, 3 * C)
        # bnd: device address of this (step, block)'s magnitude bounds: chip-filling attention launches then take the two-part
        # fp16 operand format too - and write their output already split for linear_o (no split VALU in that GEMM's staging)
        akw = dict(nq=N, nk=nk, nbatch=B, nheads=H, q_strides=st3, k_strides=st3, v_strides=st3, o_strides=(N * C, C), bias=bias,
                   bias_nk=N, ws=self.attn_ws(B, N, nk, H), f16_amax=bnd, bias_prescale=bias_prescale, **(gkw or {}))
        # (K = 512 rows in chip-filling launches: the wide-rows kernel normalises and splits a block's rows inside the projection -
        #  no pre-split copy for q | k | v at all; asked of the library)
        wrows = bool(f16 and ops.F16_ROWS and ops.F16_WIDE_ROWS and C == 512 and ops.rows_inline_supported(
            rows, 3 * C, C, hn=True, per_group_rows=N if per_sample else 0, gstride=tab_ld if per_sample else 0))
        qkv_presplit = bool(presplit and ops.PRESPLIT_QKV and not wrows)
        # k | v leave the projection already scaled and split for that attention kernel (bounds bnd[1], bnd[2]): only when BOTH
        # launches are the fp16-format kernels - asked of the library, never assumed
        kv2 = None
        # the kernel pd_attention picks depends on the launch shape only: asked once per block (kv2 and o_split both need it)
        unsplit_f16 = bool(f16 and ops.F16_ATTN and ops.SPLIT_ATTN and ops.unsplit_f16_attention(
            ops.attention(off(qkv, 0), off(qkv, C), off(qkv, 2 * C), None, query_only=True, **akw)))
        if unsplit_f16 and ops.KV_PRESPLIT and self.probe is None \
                and ops.kv2_supported(rows, C, a2=qkv_presplit and a2 is not None, per_group_rows=N if per_sample else 0):
            kv2 = self.lws("dit_kv2", rows, 4 * C, dtype=torch.float16)      # per row: k then v, groups of (4 high, 4 low) parts
            hn.update(Y2=kv2, y2_amax=bnd + 4, y2_col0=C)
            akw.update(KV2=kv2, kv2_strides=(N * 4 * C, 4 * C))
        if qkv_presplit:
            self.gemm(x, P.qkv(prefix + ".attention"), qkv, rows, 3 * C, C, a_amax=b_y, **norm_split(tab_off, b_y), **hn)
        else:
            self.gemm(x, P.qkv(prefix + ".attention"), qkv, rows, 3 * C, C, stats=self.stats_buf(rows), stats_inline=(LN, eps),
                      pro_b=off(tab, tab_off), pro_w=off(tab, tab_off + C), a_amax=b_y, **hn, **grp)
        if self.probe is not None and kv2 is None and f16:
            self.probe(prefix, "v", qkv[:B * N, 2 * C:], bnd + 8)
        Wo, bo, _, _, ldw = P.linear(prefix + ".attention.linear_o")
        # (the attention kernel lays its split output out as [2][B N][C]: it is the projection's A2 only when no padding rows follow)
        o_split = unsplit_f16 and ops.ATTN_SPLIT_OUT and self.probe is None and C % 32 == 0 and ldw == C and rows == B * N \
            and ops.presplit_supported(rows, C, C, f16=True, gate=True, per_group_rows=N if per_sample else 0, gstride=tab_ld if per_sample else 0)
        if o_split:
            o2 = self.lws("dit_o2", 2, rows, C, dtype=torch.float16)
            ops.attention(off(qkv, 0), off(qkv, C), off(qkv, 2 * C), None, O2=o2, **akw)
            self.gemm(x, Wo, x, rows, C, C, ldw=ldw, bias=bo, mul=off(tab, tab_off + 2 * C), res=x, a_amax=b_o, A2=o2, **mgrp)
        else:
            o = self.lws("dit_o", rows, C)
            ops.attention(off(qkv, 0), off(qkv, C), off(qkv, 2 * C), o, **akw)
            if self.probe is not None and f16:
                self.probe(prefix, "o", o[:B * N], bnd + 8)
            self.gemm(o, Wo, x, rows, C, C, ldw=ldw, bias=bo, mul=off(tab, tab_off + 2 * C), res=x, a_amax=b_o, **mgrp)
        t2 = tab_off + 3 * C
        W2, _, _, _, ldw = P.linear(prefix + ".transition.feed_forward.w2")
        if f16 and ops.FUSED_TRANSITION and self.probe is None and not presplit and W13.shape[1] == C and ldw == hidden \
                and ops.transition_f16(x, rows, C, hidden, shift=off(tab, t2), scale1p=off(tab, t2 + C), gate=off(tab, t2 + 2 * C),
                                       W13=P.w2(W13, C), W2=P.w2(W2, hidden), y_amax=b_y2, h_amax=b_h, eps=eps,
                                       rows_per_group=N if per_sample else 0, gstride=tab_ld if per_sample else 0):
            return                       # atom rows: statistics + SwiGLU + down-projection + gate + residual in one launch
        h = self.lws("dit_h", rows, hidden)
        wrows_glu = bool(f16 and ops.F16_ROWS and ops.F16_WIDE_ROWS and ops.F16_WIDE_ROWS_GLU and C == 512 and ops.rows_inline_supported(
            rows, 2 * hidden, C, glu=1, per_group_rows=N if per_sample else 0, gstride=tab_ld if per_sample else 0))
        if presplit and not wrows_glu:
            self.gemm(x, W13, h, rows, 2 * hidden, C, glu=1, a_amax=b_y2, **norm_split(t2, b_y2))
        else:
            self.gemm(x, W13, h, rows, 2 * hidden, C, stats=self.stats_buf(rows), stats_inline=(LN, eps), pro_b=off(tab, t2),
                      pro_w=off(tab, t2 + C), glu=1, a_amax=b_y2, **grp)
        if self.probe is not None and f16:
            self.probe(prefix, "h", h[:B * N], bnd + 20)
        self.gemm(h, W2, x, rows, C, hidden, ldw=ldw, mul=off(tab, t2 + 2 * C), res=x, a_amax=b_h, **mgrp)

    def check_dit_bounds(self, batch, a, s, prep, plan, B, sigma_data=16.0):
        """First-call guard of the two-part fp16 operand format (round 5): run the denoiser on THIS system,
        THESE weights and the call's own AdaLN tables at three noise levels (first, middle, last step; inputs = ground-truth
        coordinates + t^ N(0, 1), the operating point of a trained denoiser) with every bounded operand materialised in fp32, and
        compare what the launches would see with the bounds pd_dit_bounds derived:
          * observed max > bound: the bound is VIOLATED (an overflow waiting to happen) -> FloatingPointError, always;
          * bound / (typical magnitude) > 2^17, or bound / observed max > 2^12: the bound holds but is so loose that ordinary
            elements fall below the low part's precision floor (csrc/common.h: 2^-40 of the bound) -> the family ("atom" /
            "token") is taken off the fp16 format for this engine (bf16 x 6 needs no bound), with a warning.
        "Typical magnitude" = root mean square over the rows' median |x| would be costlier; the rms of the operand is used.
        Returns the set of families switched off by THIS check (the caller then re-prepares the call).  Not part of any
        captured graph; costs three eager denoiser passes once per (weights, noise schedule)."""
        import warnings
        # (while self.probe is set, dit_block materialises v, o and h as fp32 tensors: no pre-split k | v, no split attention output, no
        #  fused atom transition - a per-ENGINE switch: replicas of a StreamPool run their checks while other replicas sample)
        hooks_were_off = getattr(ops._TLS, "no_hooks", False)
        ops._TLS.no_hooks = True             # (test / profiling hooks see the product launches only; per host thread, no global is touched)
        rec = []

        def probe(prefix, name, t, bound_addr):
            tf = t.float()
            rec.append((prefix, name, tf.abs().amax(), tf.pow(2).mean().sqrt(), bound_addr))
        A = a.shape[0]
        gen = torch.Generator(device=self.device).manual_seed(1234)
        # (screening-time batches may carry a zero / placeholder x_gt: the per-residue reference conformer positions are then the
        #  representative geometry the check has - ADVICE r5)
        x0 = batch["x_gt"] if float(batch["x_gt"].abs().max()) > 0 else batch["ref_pos"]
        xg = x0 - (x0 * batch["a_mask"][:, None]).sum(0, keepdim=True) / batch["a_mask"].sum().clamp_min(1)
        steps = sorted({0, len(plan) // 2, len(plan) - 1})
        x_hat = self.ws.get("probe_xhat", B, A, 3)
        x_den = self.ws.get("probe_xden", B, A, 3)
        bnd_of = {}
        self.probe = probe
        try:
            for i in steps:
                x_hat.copy_(xg[None] + plan[i]["t_hat"] * torch.randn(B, A, 3, device=self.device, generator=gen))
                n0 = len(rec)
                self.af3_dit(batch, x_hat, x_den, a, s, prep, B, plan[i], row=i)
                for j in range(n0, len(rec)):
                    bnd_of[j] = i
        finally:
            self.probe = None
            ops._TLS.no_hooks = hooks_were_off
        if not rec:
            return set()
        amax = torch.stack([r[2] for r in rec]).cpu()
        rms = torch.stack([r[3] for r in rec]).cpu()
        # the bounds live in the per-call tables: read them back through their addresses' offsets
        tabs = {"atom": prep["bnd_atom"], "token": prep["bnd_token"]}
        report, off_now = {}, set()
        for j, (prefix, name, _, _, addr) in enumerate(rec):
            fam = "token" if ".token_dit." in prefix else "atom"
            tb = tabs[fam]
            idx = (addr - tb.data_ptr()) // 4
            bound = float(tb.reshape(-1)[idx])
            m, r = float(amax[j]), float(rms[j])
            if not (m <= bound * 1.001):
                raise FloatingPointError(f"fp16-format operand bound VIOLATED at {prefix} ({name}, step {bnd_of[j]}): observed max {m:.4g} > "
                                         f"bound {bound:.4g} - the engine's bounds do not describe these weights (rebuild the engine; "
                                         f"ops.F16_GEMM = False to confirm)")
            e = report.setdefault(fam, {}).setdefault(name, {"amax_ratio": 0.0, "typical_ratio": 0.0, "where": None})
            ra, rt = bound / max(m, 1e-30), bound / max(r, 1e-30)
            if rt > e["typical_ratio"]:
                e["typical_ratio"], e["where"] = rt, f"{prefix} step {bnd_of[j]}"
            e["amax_ratio"] = max(e["amax_ratio"], ra)
        for fam, ops_ in report.items():
            for name, e in ops_.items():
                if e["typical_ratio"] > 2.0 ** 17 or e["amax_ratio"] > 2.0 ** 12:
                    off_now.add(fam)
                    warnings.warn(f"physdock_amd: the static bound of the {fam}-level DiT operand '{name}' is 2^{math.log2(e['typical_ratio']):.1f} "
                                  f"above its typical magnitude (2^{math.log2(e['amax_ratio']):.1f} above its maximum) at {e['where']}: the {fam} "
                                  f"blocks run on the bf16 x 6 kernels for these weights (no bound needed, ~1.3x slower)")
        self.bound_report = report
        self.f16_off |= off_now
        return off_now

    def af3_dit(self, batch, x_hat, x_den, a, s, prep, B, scal, row=0, per_sample=False, grp=None):
        """AF3DiT.forward (transformers.py:235-262) for one noise level.
        scal: dict(c_in, c_skip, c_out) floats, or per-sample device arrays when per_sample.
        grp (PhysDock.sample_diffusion_many): dict(G, B, nk_atom, nk_token) - G systems of grp["B"] samples each, B = G grp["B"] in
        all.  a [G][A][Ca] and s [G][T][Cs] are then stacked, batch["_tok_start"] [G][T + 1] and batch["atom_id_to_token_id"] [G][A]
        too, nk_atom / nk_token device int32 [G] the real counts, batch["_A_real"] / ["_T_real"] their maxima, batch["_pool_tpb"]
        the minimum, prep from prepare_dit_many.  Every row-wise launch runs once over the G B samples; the per-system inputs go
        through the grouped entry points."""
        P, ws = self.P, self.ws
        dt = self.cfg.model.dit
        Ca, Cs = dt.c_a, dt.c_s
        A, T = a.shape[-2], s.shape[-2]
        Ar, Tr = batch.get("_A_real", A), batch.get("_T_real", T)
        Ha, Hs = Ca // 32, Cs // 32
        G, Bg = (grp["G"], grp["B"]) if grp is not None else (1, B)
        gka = gkt = None
        if grp is not None:
            if per_sample or G * Bg != B:
                raise ValueError("a grouped denoiser pass takes G x B samples on one schedule")
            gka = dict(group_samples=Bg, bias_gstride=prep["gstride_atom"], nk_group=grp["nk_atom"])
            gkt = dict(group_samples=Bg, bias_gstride=prep["gstride_token"], nk_group=grp["nk_token"])
        L = ops._lib.init()
        sp = ops.stream()
        # Sample-major activations [B N, C] are allocated - and run through every row-wise launch - in whole 64-row tiles: a ragged
        # system (T = 227 -> 228 tokens at 20 samples = 4 560 rows) otherwise leaves every projection a row remainder, and the remainder
        # launches (<= 63 rows on the general kernel, 22 - 50 us each) cost more than the projections themselves.  Rows past B N are
        # never initialised and never read by anything that mixes rows (attention / pooling address rows by (sample, position)).
        RA = B * A if per_sample else -(-(B * A) // 64) * 64
        RT = B * T if per_sample else -(-(B * T) // 64) * 64
        ba = self.lws("dit_ba", RA, Ca)
        cin_b = ops.ptr(scal["c_in"]) if per_sample else None
        if grp is not None:
            ops.check(L.pd_precond_g(ops.ptr(x_hat), scal["c_in"], None, ops.ptr(P["dit.linear_x.weight"]),
                                     ops.ptr(P["dit.linear_x.bias"]), ops.ptr(a), ops.ptr(ba), G, Bg, A, Ca, sp), "precond_g")
        else:
            ops.check(L.pd_precond(ops.ptr(x_hat), 0.0 if per_sample else scal["c_in"], cin_b, ops.ptr(P["dit.linear_x.weight"]),
                                   ops.ptr(P["dit.linear_x.bias"]), ops.ptr(a), ops.ptr(ba), B, A, Ca, sp), "precond")
        tab_a, tab_t = prep["tab_atom"], prep["tab_token"]
        lda_, ldt_ = tab_a.shape[1], tab_t.shape[1]
        fa_stride = ops.bias_frag_numel(Ha, A, A)
        ft_stride = ops.bias_frag_numel(Hs, T, T)
        nb_a, nb_t = dt.no_blocks_atom, dt.no_blocks_dit
        bnd_a = None if "atom" in self.f16_off else prep["bnd_atom"]
        bnd_t = None if "token" in self.f16_off else prep["bnd_token"]

        def boff(t, n):                       # address of a bound row, or None for a family that runs without bounds (bf16 x 6)
            return None if t is None else off(t, n)
        if (prep["ps_atom"] or prep["ps_token"]) and prep["B"] != B:
            raise RuntimeError("prepare_dit pre-scaled the hoisted biases for a different sample count")
        psa, pst = prep["ps_atom"], prep["ps_token"]
        for b in range(nb_a):
            self.dit_block(f"dit.atom_dit_encoder.blocks.{b}", ba, B, A, Ca, off(prep["atom_bias"], b * fa_stride),
                           tab_a, row * lda_ + b * 6 * Ca, lda_, per_sample, Ar, bnd=boff(bnd_a, (row * 2 * nb_a + b) * 8), bias_prescale=psa,
                           rows_alloc=RA, gkw=gka)
        bs = self.lws("dit_bs", RT, Cs)
        Wd, bd, _, Kd, ldwd = P.linear("dit.linear_downscale")
        tpb = batch.get("_pool_tpb", 0)
        rc = -3
        if ops.FUSED_POOL and ops.SPLIT_GEMM and ops.F16_GEMM and tpb > 0 and Kd == Ca and ldwd == Ca:
            # linear_downscale + SiLU + token mean + s in one launch: u [B A, 512] (268 MB at the benchmark shape) is never written
            w2p, w2i = P.w2(Wd, Kd)
            if grp is not None:
                rc = L.pd_downscale_pool_g(ops.ptr(ba), w2p.data_ptr(), ops.ptr(w2i), ops.ptr(bd), ops.ptr(batch["_tok_start"]), ops.ptr(s),
                                           ops.ptr(bs), G, Bg, A, T, Ca, Cs, tpb, sp)
            else:
                rc = L.pd_downscale_pool(ops.ptr(ba), w2p.data_ptr(), ops.ptr(w2i), ops.ptr(bd), ops.ptr(batch["_tok_start"]), ops.ptr(s), ops.ptr(bs),
                                         B, A, T, Ca, Cs, tpb, sp)
        if rc == -3:            # PD_ERR_UNSUPPORTED (other widths, a token of more than 64 atoms): projection, then the segment mean
            u = self.lws("dit_u", RA, Cs)
            self.lin(ba, "dit.linear_downscale", RA, out=u, act=ACT_SILU)
            if grp is not None:
                ops.check(L.pd_segment_pool_g(ops.ptr(u), ops.ptr(batch["_tok_start"]), ops.ptr(s), ops.ptr(bs), G, Bg, A, T, Cs, sp), "pool_g")
            else:
                ops.check(L.pd_segment_pool(ops.ptr(u), ops.ptr(batch["_tok_start"]), ops.ptr(s), ops.ptr(bs), B, A, T, Cs, sp), "pool")
        else:
            ops.check(rc, "downscale_pool")
        for b in range(nb_t):
            self.dit_block(f"dit.token_dit.blocks.{b}", bs, B, T, Cs, off(prep["token_bias"], b * ft_stride),
                           tab_t, row * ldt_ + b * 6 * Cs, ldt_, per_sample, Tr, bnd=boff(bnd_t, (row * nb_t + b) * 8), bias_prescale=pst,
                           rows_alloc=RT, gkw=gkt)
        us = self.lws("dit_us", RT, Ca)
        self.lin(bs, "dit.linear_upscale", RT, out=us)
        if grp is not None:
            ops.check(L.pd_unpool_add_g(ops.ptr(ba), ops.ptr(us), ops.ptr(batch["atom_id_to_token_id"]), G, Bg, A, T, Ca, sp), "unpool_g")
        else:
            ops.check(L.pd_unpool_add(ops.ptr(ba), ops.ptr(us), ops.ptr(batch["atom_id_to_token_id"]), B, A, T, Ca, sp), "unpool")
        for b in range(nb_a):
            self.dit_block(f"dit.atom_dit_decoder.blocks.{b}", ba, B, A, Ca,
                           off(prep["atom_bias"], (nb_a + b) * fa_stride), tab_a, row * lda_ + (nb_a + b) * 6 * Ca, lda_,
                           per_sample, Ar, bnd=boff(bnd_a, (row * 2 * nb_a + nb_a + b) * 8), bias_prescale=psa, rows_alloc=RA, gkw=gka)
        cs_b = ops.ptr(scal["c_skip"]) if per_sample else None
        co_b = ops.ptr(scal["c_out"]) if per_sample else None
        ops.check(L.pd_denoise(ops.ptr(ba), ops.ptr(x_hat), ops.ptr(P["dit.norm_r.weight"]), ops.ptr(P["dit.norm_r.bias"]),
                               ops.ptr(P["dit.linear_r.weight"]), self.eps, 0.0 if per_sample else scal["c_skip"],
                               0.0 if per_sample else scal["c_out"], cs_b, co_b, ops.ptr(x_den), B, A, Ca, sp), "denoise")
        return x_den
