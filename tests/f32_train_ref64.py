"""TEST HELPER (not a test, never shipped): plain float64 restatements of the fp32 TRAINING kernels -- csrc/fp32_train.hip (RMSNorm,
SwiGLU, SiLU and ReLU backward, LoRA dropout, column sums, LayerNorm parameter gradients, transpose, row gather, the two-launch
GQA attention backward) and csrc/f32_ca.hip (the cross-attention projector's forward, its lse form and its backward) -- on the exact
fp32 input values, each with a first-order bound E for every element it returns, the case lists, the seeded inputs and the runs
(`run_*`) that tests/test_f32_train_ref64_cpu.py (through F32TrainTorch, a plain-torch fp32 restatement under HipOps' method names)
and tests/test_gpu_f32_train_f64.py (through HipOps) share.  Nothing is shared with the kernels.

RULES (those of tests/f32_ref64.py).  e = 2^-24, LIMIT = 1.0: every element is held to |got - ref| <= E, and has the reference's
value exactly where E = 0 (copies, zeros owed to padding, selections, the exact profiles).  An fp32 +, -, *, / : e relative;
rsqrtf 4 e; logf of S >= 1: 4 e |log S| + 2 e; expf(d): 2 e + e |d| wherever it stands (the contraction finding of f32_ref64.py's
header), and where d is itself an fp32 difference that subtraction's own e |d| beside it: 2 e + 2 e |d|.  A fixed-order sum of
terms t_i carries depth . e . sum |t_i|, depth the longest chain of fp32 additions a term passes in THAT kernel; an MFMA chain of n
terms the any-order bound n e sum |t_i| (n - 1 additions and the product).  Bounds of cancelling results are absolute.

    rmsnorm_bwd    ss = sum x^2, dot = sum (w dy) x: ceil(D / 1024) serial adds per thread + 6 shuffle levels + 16 waves = depth;
                   ss carries one product (depth + 1), dot two (depth + 2): E_dot = (depth + 2) e sum |w dy x|;
                   rs = rsqrtf(ss / D + eps): rel_rs = e ((depth + 1) / 2 + 5);  k = rs rs rs / D dot:
                   E_k = |k| (3 rel_rs + 4 e) + rs^3 / D E_dot;  g = rs (w dy) - x k, a cancelling difference, absolutely:
                   E = |rs w dy| (rel_rs + 2 e) + |x| E_k + e |x k| + e |g|;  accumulate: + e |dx + g|.  A zero row: ss = dot = k = 0
                   exactly, rs = rsqrtf(eps).  eps is the fp32 value the entry point receives.
    sigmoid        sg = 1 / (1 + t), t = expf(-g): t carries 2 e + e |g|, which weighs t / (1 + t) = 1 - sg in the quotient; the
                   addition and the division:  E_sg = sg (2 e + (1 - sg) (2 e + e |g|)), and 2^-126 absolute where |g| > 80 (expf
                   leaves the fp32 range at 88.7; 1 / t leaves the normal range at 87.3);  A = 1 - sg: E_A = E_sg + e A, absolute
                   (at g = 45 sg rounds to 1 and A to 0);  C = 1 + g A: E_C = |g| E_A + e |g A| + e |C|
    swiglu_bwd     dg = ((d u) sg) C: P = d u sg, E_P = |d u| E_sg + 2 e |P|, E_dg = |P| E_C + |C| E_P + e |dg|;
                   du = (d g) sg: E_du = |d g| E_sg + 2 e |du|
    silu           forward x sg: |x| E_sg + e |y|;  backward (dy sg) C: P = dy sg, E_P = |dy| E_sg + e |P|, E = |P| E_C + |C| E_P + e |out|
    relu_bwd       a selection: dy where y > 0, else +0: exact
    lora_dropout   the integer mask of oracle/lora_oracle.py (element index m C + c, never the pitched one) and ONE fp32 product by
                   fl32(1 / (1 - p)): the bits of torch's fp32 product (p = 0: a copy, p = 0.5: exactly 2 x); accumulate: e |out + v|
    colsum         R - 1 serial additions: (R - 1) e sum |x|; the integer profile exact
    layernorm_bwd_params   dgamma = sum_r d ((x - mean) rstd): three roundings per term + R - 1 additions: (R + 2) e sum |d x^|;
                   dbeta: (R - 1) e sum |d|.  mean, rstd are INPUTS.
    transpose      an exact permutation, +0 for R <= r < Rpad; columns >= Rpad and rows >= C of dst untouched
    gather_rows    copies, +0 rows behind a negative index: exact
    attn_bwd       first launch (one workgroup per query and KV head).  s_j = scale sum_d q_d k_jd: 16 serial products per lane + 3
                   shuffle levels + the product + the scale = 21: Es_j = 21 e scale sum |q k|;  dP_j = sum_d do_d v_jd, the same dot:
                   E_dP = 21 e sum |do v|;  e_j = expf(s_j - m): delta_j = 2 e + 2 e |s_j - m| + Es_j relative;
                   l = sum e_j: depth_l = ceil(nk / 256) serial + 6 levels + 4 waves;  P_j = e_j (1 / l):
                   rho_j = delta_j + sum_i P_i delta_i + e (depth_l + 2);
                   lse = m + logf(l): E_lse = e |lse| + 4 e |log l| + 2 e + e depth_l + sum_j P_j delta_j;
                   delta = sum_j P_j dP_j, the same summation: E_delta = sum_j (|P dP| (rho_j + e + e depth_l) + P_j E_dP_j);
                   c_j = dP_j - delta: E_c = E_dP + E_delta + e |c|, absolute;  dS_j = P_j c_j scale:
                   E_dS = scale (P E_c + |P c| (rho_j + 2 e));  dQ = sum_j dS_j k_j: the wave's quarter serial (ceil(nk / 4)) + 4
                   partials (3 additions) + the product: E_dQ = sum_j (E_dS_j + e (ceil(nk / 4) + 4) |dS_j|) |k_j|.
                   Second launch (one workgroup per key and KV head) reads lse and delta: p_i = expf(s_i - lse_i):
                   rel2_i = 2 e + 2 e |s_i - lse_i| + Es_i + E_lse_i;  dS'_i = p_i (dP_i - delta_i) scale:
                   E_dS' = scale (P E_c + |P c| (rel2 + 2 e));  over the nq = S - j queries and all REP heads of the group, the
                   wave's quarter serial: depth_kv = ceil(nq / 4) REP + 4:  E_dV = sum (P (rel2 + e depth_kv)) |do|,
                   E_dK = sum (E_dS' + e depth_kv |dS'|) |q|.  Rows before kstart: +0 in dQ, dK, dV, lse and delta.  The query at
                   s = kstart has one key: P = 1, delta = dP, dS = 0: dQ is 0 exactly.
    ca_attn        s_j = (sum_d q_d k_jd) / denom on v_mfma_f32_16x16x4_f32 (the dh / PARTS ranges added in part order: dh - 1
                   additions in some order): Es_j = (dh + 1) e sum |q k| / denom.  Online softmax, the running l and O rescaled
                   once per key tile, T tiles per split, Z splits merged in order.  Every exponential's argument a key passes
                   (its own s_j - m_tile, the rescales m_old - m_new, the merge's m_z - M) is an fp32 difference and they telescope to
                   d_j = s_j - M: 2 e |d_j|.  depth = KT (the tile's P K product, any order) + 2 T (rescale: a product and an
                   addition per tile) + 2 (T + 1) (expf's constant: its own, T - 1 rescales, the merge) + Z + 1 (the merge's
                   product and additions) + 1 (acc / L):  rel_j = Es_j + 2 e |d_j| + e depth;
                   E_out = sum_j P_j |k_j| (rel_j + sum_i P_i rel_i) + 2^-126 (2 sum_j |k_j| + 2 V) (a probability or product
                   below the normal range); lse = M + logf(L), L >= 1: E_lse = e |lse| + 4 e |log L| + 2 e + sum_j P_j rel_j.
                   V = 1: p = 1, l = 1, weight 1: out has the table row's bits; on the integer profile the score is exact in any
                   order and lse has the bits of its fp32 quotient by denom.  Padding keys k >= V are masked (-inf), not scored 0.
    ca_attn_bwd    held twice.  On operands that are HANDED in (out, lse: the fp32 roundings of the float64 forward), where the
                   forward's error does not enter; and in the chain, handed the forward kernel's own out and lse against the float64
                   gradient of the definition, where E_out enters delta (+ sum |dout| E_out) and E_lse the argument of expf
                   (rel_p + E_lse).  delta_r = sum_c dout out over the head: dh / TPR serial + log2 TPR levels + the product,
                   TPR = 512 / rows per tile: E_dl = (dh / TPR + log2 TPR + 1) e sum |dout out|;  p_j = expf(s_j - lse):
                   rel_p = 2 e + 2 e |s_j - lse| + Es_j;  dP_j = sum_d dout_d k_jd: dh e sum |dout k|;  c_j = dP_j - delta:
                   E_c = E_dP + E_dl + e |c| absolute (a near-one-hot row has P (dP - delta) of 1e-8 of an ordinary row: no
                   pooled scale is needed);  dS_j = p_j c_j / denom: E_dS = (p E_c + |p c| (rel_p + 2 e)) / denom;
                   dq = sum_j dS_j k_j: KT any-order in the tile + T tiles + Z splits:
                   E_dq = sum_j (E_dS_j + e (KT + T + Z) |dS_j|) |k_j| + 2^-126 sum_j 2 (|c_j| / denom + 1) (|k_j| + 1)

GUARDS.  Every output and workspace starts as NaN; every operand has NaN guard rows behind it and NaN in the gap of a pitch greater
than its width; everything outside what a call owes must keep its bits (the runs assert it); calls that take a workspace run twice,
equal bits.  The references run on whatever device `dev` puts the inputs on (the GPU file computes them in float64 on the device)."""
import collections
import math

import torch

from f32_ref64 import (GUARD, LIMIT, TINY, Ref, bits, case_id, cdiv, check, e, gen, ident, nan, old_metric, operand, output, owed,  # noqa: F401
                       same_bits, untouched, vec, worst_of)
from oracle.lora_oracle import lora_keep_scale

F64, F32, I32, I64 = torch.float64, torch.float32, torch.int32, torch.int64
HD = 128
EPS = 1e-6
EPS32 = float(torch.tensor(EPS, dtype=F32))                       # what the entry point receives


def row_scales(M):
    return 2.0 ** torch.linspace(-10, 10, M).round()


def f64(t, dev=ident):
    return dev(t).to(F64)


def cpu(t):
    return t.detach().cpu()


# ------------------------------------------------------------------------------------------------ F32TrainTorch: the fp32 restatement
def sigmoid32(x):
    return 1 / (1 + torch.exp(-x))


class F32TrainTorch:
    """plain torch fp32 on the CPU under HipOps' method names and signatures (a test helper: the CPU file and the mutants run
    through it).  Each method follows its kernel's definition, not its thread map; outputs are written into the caller's views,
    workspaces are ignored.  The small `_` hooks are what the mutants of the CPU file override."""
    name = "f32traintorch"

    # ---- rmsnorm_bwd
    def _rms_d(self, D):
        return float(D)

    def _rms_dot_w(self, w):
        return w

    def f32_rmsnorm_bwd(self, dy, x, w, dx, M, D, eps, accumulate):
        xv, dv, wv = x[:M, :D], dy[:M, :D], w[:D]
        ss = (xv * xv).sum(-1, keepdim=True)
        dot = (self._rms_dot_w(wv) * dv * xv).sum(-1, keepdim=True)
        rs = torch.rsqrt(ss / D + eps)
        k = rs * rs * rs / self._rms_d(D) * dot
        g = rs * (wv * dv) - xv * k
        dx[:M, :D] = dx[:M, :D] + g if accumulate else g

    # ---- pointwise
    def _sigmoid(self, x):
        return sigmoid32(x)

    def _swiglu_du(self, d, g, u, sg):
        return d * g * sg

    def f32_swiglu_bwd(self, dact, gu, dgu, M, I):
        g, u, d = gu[:M, :I], gu[:M, I:2 * I], dact[:M, :I]
        sg = self._sigmoid(g)
        dgu[:M, :I] = d * u * sg * (1 + g * (1 - sg))
        dgu[:M, I:2 * I] = self._swiglu_du(d, g, u, sg)

    def f32_silu(self, x, out, dy=None):
        sg = self._sigmoid(x)
        out.copy_(x * sg if dy is None else dy * sg * (1 + x * (1 - sg)))

    def f32_relu_bwd(self, y, dy, out):
        out.copy_(torch.where(y > 0, dy, torch.zeros_like(dy)))

    def _mask_scale(self, rng, sid, M, Cn, ldx, p):
        return lora_keep_scale((int(rng[0]), int(rng[1])), sid, (M, Cn), p)

    def f32_lora_dropout(self, x, out, M, Cn, p, rng, sid, accumulate=False):
        v = x[:M, :Cn] * self._mask_scale(rng, sid, M, Cn, x.stride(0), p)
        out[:M, :Cn] = out[:M, :Cn] + v if accumulate else v

    # ---- reductions and copies
    def _colsum_rows(self, R):
        return R

    def f32_colsum(self, x, out, R, Cn):
        out[:Cn] = x[:self._colsum_rows(R), :Cn].sum(0)

    def f32_layernorm_bwd_params(self, dy, x, mean, rstd, dgamma, dbeta, R, D):
        d = dy[:R, :D]
        dgamma[:D] = (d * ((x[:R, :D] - mean[:R, None]) * rstd[:R, None])).sum(0)
        dbeta[:D] = d.sum(0)

    def f32_transpose(self, src, dst, R, Cn, Rpad):
        dst[:Cn, :R] = src[:R, :Cn].t()
        dst[:Cn, R:Rpad] = 0

    def f32_gather_rows(self, dx, rows, out, n, D):
        for r in range(n):
            out[r, :D] = dx[int(rows[r]), :D] if int(rows[r]) >= 0 else torch.zeros(D)

    # ---- attention backward
    mutant = None                                                # attn_bwd / ca mutants: a name the methods below look at

    def f32_attn_bwd(self, qkv, dout, kstart, dqkv, lse_ws, delta_ws, B, S, H, G, scale):
        rep, mut = H // G, self.mutant
        x, do = qkv[:B * S].view(B, S, H + 2 * G, HD), dout[:B * S].view(B, S, H, HD)
        dx = dqkv[:B * S].view(B, S, H + 2 * G, HD)
        lse, dl = lse_ws[:B * H * S].view(B, H, S), delta_ws[:B * H * S].view(B, H, S)
        dx.zero_(), lse.zero_(), dl.zero_()
        ar = torch.arange(S)
        for b in range(B):
            lo = int(kstart[b]) + (1 if mut == "kstart off by one" else 0)
            if lo >= S:
                continue
            allow = (ar[None, :] <= ar[:, None]) & (ar[None, :] >= lo) & (ar[:, None] >= lo)
            if mut == "newest key dropped" and S - lo >= 3:
                allow[S - 2, S - 2] = False                      # one query loses its newest key
            live = allow.any(-1)
            for h in range(H):
                g = h // rep
                q, k, v, d = x[b, :, h], x[b, :, H + g], x[b, :, H + G + g], do[b, :, h]
                s = ((q @ k.t()) * scale).masked_fill(~allow, -math.inf)
                s[~live] = 0
                ls = torch.logsumexp(s, -1)
                P = torch.where(allow, torch.exp(s - ls[:, None]), torch.zeros_like(s))
                dP = d @ v.t()
                delta = (P * dP).sum(-1)
                lse[b, h], dl[b, h] = torch.where(live, ls, torch.zeros(S)), delta
            for h in range(H):
                g = h // rep
                q, k, v, d = x[b, :, h], x[b, :, H + g], x[b, :, H + G + g], do[b, :, h]
                hd = h + 1 - 2 * (h % 2) if (mut == "delta from the neighbouring head" and rep > 1) else h
                s = (q @ k.t()) * scale
                P = torch.where(allow, torch.exp(s - lse[b, h][:, None]), torch.zeros_like(s))
                dS = P * (d @ v.t() - dl[b, min(hd, H - 1)][:, None]) * (1.0 if mut == "dS without scale" else scale)
                dx[b, :, h] = dS @ k
                dx[b, :, H + G + g] += P.t() @ d
                if not (mut == "one head left out of dK" and h == g * rep + rep - 1):
                    dx[b, :, H + g] += dS.t() @ q

    # ---- cross-attention
    def _ca_heads(self, q, table, R, H):
        V, D = table.shape
        return q[:R, :D].reshape(R, H, D // H).transpose(0, 1), table.view(V, H, D // H).transpose(0, 1), D // H

    def _ca_scores(self, qh, kh, dh, R, H):
        """[H, R, V] scores and the additive mass of the softmax denominator that is not a key (0 unless a mutant adds some)"""
        V, mut = kh.shape[1], self.mutant
        s = (qh @ kh.transpose(1, 2)) / float(torch.tensor(dh ** 0.5, dtype=F32))
        if mut == "key V - 1 masked":
            s[:, :, V - 1] = -math.inf
        if mut == "last split left out":
            D = dh * H
            splits, per = ca_plan(R, V, D, H)
            s[:, :, (splits - 1) * per * ca_kt(dh):] = -math.inf
        pad = (cdiv(V, ca_kt(dh)) * ca_kt(dh) - V) if mut == "padding keys unmasked" else 0
        return s, pad

    def _ca_forward(self, q, table, R, H):
        qh, kh, dh = self._ca_heads(q, table, R, H)
        s, pad = self._ca_scores(qh, kh, dh, R, H)
        m = s.amax(-1, keepdim=True).clamp_min(0.0) if pad else s.amax(-1, keepdim=True)
        p = torch.exp(s - m)
        L = p.sum(-1, keepdim=True) + pad * torch.exp(-m)          # an unmasked padding key scores 0 and holds a zero value row
        o = (p @ kh) / L
        return o.transpose(0, 1).reshape(R, -1), (m + torch.log(L))[:, :, 0].t()

    def f32_ca_attn(self, q, table, out, R, H, ws=None):
        out[:R, :table.shape[1]] = self._ca_forward(q, table, R, H)[0]

    def f32_ca_attn_lse(self, q, table, out, lse, R, H, ws=None):
        o, ls = self._ca_forward(q, table, R, H)
        out[:R, :table.shape[1]], lse[:R, :H] = o, ls

    def f32_ca_attn_bwd(self, q, table, out, dout, lse, dq, R, H, ws=None):
        V, D = table.shape
        qh, kh, dh = self._ca_heads(q, table, R, H)
        denom = float(torch.tensor(dh ** 0.5, dtype=F32))
        oh, gh = (t[:R, :D].reshape(R, H, dh).transpose(0, 1) for t in (out, dout))
        if self.mutant == "delta from the wrong head" and H > 1:
            oh = oh.roll(1, 0)
        delta = (gh * oh).sum(-1, keepdim=True)
        P = torch.exp((qh @ kh.transpose(1, 2)) / denom - lse[:R, :H].t()[:, :, None])
        dS = P * (gh @ kh.transpose(1, 2) - delta) / (1.0 if self.mutant == "denom applied once" else denom)
        dq[:R, :D] = (dS @ kh).transpose(0, 1).reshape(R, D)


# ------------------------------------------------------------------------------------------------ rmsnorm_bwd
Rmsb = collections.namedtuple("Rmsb", "M D profile acc")
RMSB_DS = (1, 64, 1023, 1024, 1025, 2049, 3584)
RMSB_CASES = ([Rmsb(M, D, "scales", acc) for D in RMSB_DS for M in (1, 3) for acc in (0, 1)]
              + [Rmsb(3, D, "outlier", acc) for D in (1023, 1025, 3584) for acc in (0, 1)]
              + [Rmsb(3, D, "zero_row", acc) for D in (64, 1023, 2049) for acc in (0, 1)])


def rmsb_inputs(c):
    """scales: x rows x 2^-10 .. 2^10 and dy rows the other way round; outlier: one column of x and dy x 2^10; zero_row: the middle
    row of x zero and every third w zero"""
    g = gen(101, c.M, c.D)
    x, dy, w, dx0 = (torch.randn(*s, generator=g) for s in ((c.M, c.D), (c.M, c.D), (c.D,), (c.M, c.D)))
    if c.profile == "scales":
        x *= row_scales(c.M)[:, None]
        dy *= row_scales(c.M).flip(0)[:, None]
    elif c.profile == "outlier":
        x[:, min(1, c.D - 1)] *= 1024.0
        dy[:, min(1, c.D - 1)] *= 1024.0
    else:
        x[c.M // 2] = 0
        w[::3] = 0
    return dict(x=x, dy=dy, w=w, dx0=dx0, case=c)


def rmsb_reference(d, dev=ident):
    c = d["case"]
    x, dy, w, dx0 = (f64(d[k], dev) for k in ("x", "dy", "w", "dx0"))
    D, depth = c.D, cdiv(c.D, 1024) + 6 + 16
    ss = (x * x).sum(-1, keepdim=True)
    rs = torch.rsqrt(ss / D + EPS32)
    rel_rs = e * ((depth + 1) / 2 + 5)
    t = w * dy * x
    dot, E_dot = t.sum(-1, keepdim=True), (depth + 2) * e * t.abs().sum(-1, keepdim=True)
    k = rs ** 3 / D * dot
    E_k = k.abs() * (3 * rel_rs + 4 * e) + rs ** 3 / D * E_dot
    t1, t2 = rs * (w * dy), x * k
    ref = t1 - t2
    E = t1.abs() * (rel_rs + 2 * e) + x.abs() * E_k + e * t2.abs() + e * ref.abs()
    if c.acc:
        ref = dx0 + ref
        E = E + e * ref.abs()
    return Ref({"dx": (cpu(ref), cpu(E))}, {})


def run_rmsb(ops, d, dev=ident, sync=lambda: None):
    c = d["case"]
    full, dxv = output(c.M, c.D, None, dev, init=d["dx0"] if c.acc else None)      # accumulate = 0: onto NaN (overwritten, never read)
    ops.f32_rmsnorm_bwd(operand(d["dy"], None, dev), operand(d["x"], None, dev), vec(d["w"], dev), dxv, c.M, c.D, EPS, c.acc)
    sync()
    return {"dx": owed(full, c.M, c.D, f"rmsnorm_bwd {case_id(c)}")}


# ------------------------------------------------------------------------------------------------ swiglu_bwd, silu, relu_bwd
G_GRID = [-45.0, 0.0, -0.0, 45.0, 80.0, -80.0, 100.0, -100.0] + [float(v) for v in range(-80, 81, 5)]
Swib = collections.namedtuple("Swib", "M I")
SWIB_CASES = [Swib(1, 1), Swib(1, 255), Swib(1, 256), Swib(1, 257), Swib(3, 85), Swib(2, 129)]
SILU_NS = (1, 255, 256, 257)


def point_inputs(n, seed):
    """g: the grid (+-0, +-45, +-80, +-100, -80 .. 80 in steps of 5) first, then 8 N(0, 1) clamped to +-40; d: N(0, 1) x 2^-10 .. 2^10
    per element; u: N(0, 1) with every 7th element x 2^10.  On the grid |u| and |d| are at least 1, so that no product with
    sigmoid(-80) = 1.8e-35 leaves the normal range (beyond 80 the 2^-126 allowance stands)."""
    gg = gen(103, n, seed)
    g = (torch.randn(n, generator=gg) * 8).clamp_(-40, 40)
    u, d = torch.randn(n, generator=gg), torch.randn(n, generator=gg)
    d *= 2.0 ** torch.randint(-10, 11, (n,), generator=gg).to(F32)
    u[::7] *= 1024.0
    k = min(n, len(G_GRID))
    g[:k] = torch.tensor(G_GRID[:k])
    u[:k] = torch.sign(u[:k]) * (1 + u[:k].abs())
    d[:k] = torch.sign(d[:k]) * (1 + d[:k].abs()).clamp_max(8.0)
    return g, u, d


def sig_ref(g):
    """(sg, A = 1 - sg, C = 1 + g A, E_sg, E_C) in float64"""
    sg, A = torch.sigmoid(g), torch.sigmoid(-g)
    E_sg = sg * (2 * e + A * (2 * e + e * g.abs())) + TINY * (g.abs() > 80).to(F64)
    E_A = E_sg + e * A
    C = 1 + g * A
    return sg, A, C, E_sg, g.abs() * E_A + e * (g * A).abs() + e * C.abs()


def swib_inputs(c):
    g, u, d = point_inputs(c.M * c.I, c.M)
    return dict(gu=torch.cat([g.view(c.M, c.I), u.view(c.M, c.I)], 1), dact=d.view(c.M, c.I), case=c)


def swib_reference(d, dev=ident):
    c = d["case"]
    gu, dd = f64(d["gu"], dev), f64(d["dact"], dev)
    g, u = gu[:, :c.I], gu[:, c.I:]
    sg, A, C, E_sg, E_C = sig_ref(g)
    P = dd * u * sg
    E_P = (dd * u).abs() * E_sg + 2 * e * P.abs()
    dg, du = P * C, dd * g * sg
    E_dg = P.abs() * E_C + C.abs() * E_P + e * dg.abs()
    E_du = (dd * g).abs() * E_sg + 2 * e * du.abs()
    return Ref({"dgu": (cpu(torch.cat([dg, du], 1)), cpu(torch.cat([E_dg, E_du], 1)))}, {})


def run_swib(ops, d, dev=ident, sync=lambda: None):
    c = d["case"]
    full, dv = output(c.M, 2 * c.I, None, dev)
    ops.f32_swiglu_bwd(operand(d["dact"], None, dev), operand(d["gu"], None, dev), dv, c.M, c.I)
    sync()
    return {"dgu": owed(full, c.M, 2 * c.I, f"swiglu_bwd {case_id(c)}")}


def silu_inputs(n):
    x, _, dy = point_inputs(n, 7)
    return dict(x=x, dy=dy, n=n)


def silu_reference(d, dev=ident):
    x, dy = f64(d["x"], dev), f64(d["dy"], dev)
    sg, A, C, E_sg, E_C = sig_ref(x)
    y = x * sg
    P = dy * sg
    E_P = dy.abs() * E_sg + e * P.abs()
    bw = P * C
    E_bw = P.abs() * E_C + C.abs() * E_P + e * bw.abs()
    return Ref({"fwd": (cpu(y)[None], cpu(x.abs() * E_sg + e * y.abs())[None]), "bwd": (cpu(bw)[None], cpu(E_bw)[None]),
                "bwd_inplace": (cpu(bw)[None], cpu(E_bw)[None])}, {})


def run_silu(ops, d, dev=ident, sync=lambda: None):
    """forward, backward, backward in place on dy; x must keep its bits"""
    n = d["n"]
    x = vec(d["x"], dev)
    outs = {}
    for name in ("fwd", "bwd", "bwd_inplace"):
        full = dev(nan(n + GUARD))
        if name == "bwd_inplace":
            full[:n] = dev(d["dy"])
        ops.f32_silu(x, full[:n], dy=None if name == "fwd" else (full[:n] if name == "bwd_inplace" else vec(d["dy"], dev)))
        sync()
        full = full.cpu()
        assert untouched(full[n:]), f"silu {name}: elements >= n were written"
        outs[name] = full[:n][None]
    same_bits(x.cpu(), d["x"], "silu: x")
    return outs


RELU_NS = (1, 255, 256, 257, 1000)


def run_relu(ops, n, dev=ident, sync=lambda: None):
    """from the ReLU's input and from its output, out of place and in place on dy: the selection, bit for bit (+0 where y <= 0,
    y = +-0 included)"""
    g = gen(107, n)
    xin, dy = torch.randn(n, generator=g), torch.randn(n, generator=g) * 2.0 ** torch.randint(-10, 11, (n,), generator=g).to(F32)
    xin[::5] = 0.0
    xin[1::10] = -0.0
    for y in (xin, xin.clamp_min(0)):
        want = torch.where(y > 0, dy, torch.zeros(n))
        for inplace in (False, True):
            full = dev(nan(n + GUARD))
            if inplace:
                full[:n] = dev(dy)
            ops.f32_relu_bwd(vec(y, dev), full[:n] if inplace else vec(dy, dev), full[:n])
            sync()
            full = full.cpu()
            assert untouched(full[n:]), "relu_bwd: elements >= n were written"
            assert torch.equal(full[:n], want)
            same_bits(full[:n], want, f"relu_bwd n = {n}, in place = {inplace}")


# ------------------------------------------------------------------------------------------------ lora_dropout
Drop = collections.namedtuple("Drop", "M C ldx ldo p sid step acc")
DROP_SHAPES = ((1, 1, 3, 2), (3, 85, 88, 91), (5, 256, 260, 257), (2, 257, 300, 264))
DROP_CASES = ([Drop(M, C, ldx, ldo, p, 1, 3, acc) for (M, C, ldx, ldo) in DROP_SHAPES for p in (0.0, 0.5, 0.1, 0.25, 0.999999) for acc in (0, 1)]
              + [Drop(3, 85, 88, 91, 0.1, sid, step, 0) for sid in (0, 70000) for step in (1, 12345)])
DROP_SEED = 987654321


def drop_inputs(c):
    g = gen(109, c.M, c.C, c.sid)
    return dict(x=torch.randn(c.M, c.C, generator=g), out0=torch.randn(c.M, c.C, generator=g),
                rng=torch.tensor([DROP_SEED, c.step], dtype=I64), case=c)


def drop_reference(d, dev=ident):
    c = d["case"]
    v = d["x"] * lora_keep_scale((DROP_SEED, c.step), c.sid, (c.M, c.C), c.p)        # one fp32 product: its bits
    if c.p == 0.0:
        assert torch.equal(bits(v), bits(d["x"]))
    if not c.acc:
        return Ref({}, {"out": v})
    ref = d["out0"].to(F64) + v.to(F64)
    return Ref({"out": (ref, e * ref.abs())}, {})


def run_drop(ops, d, dev=ident, sync=lambda: None):
    c = d["case"]
    full, ov = output(c.M, c.C, c.ldo, dev, init=d["out0"] if c.acc else None)
    ops.f32_lora_dropout(operand(d["x"], c.ldx, dev), ov, c.M, c.C, c.p, dev(d["rng"]), c.sid, accumulate=bool(c.acc))
    sync()
    return {"out": owed(full, c.M, c.C, f"lora_dropout {case_id(c)}")}


# ------------------------------------------------------------------------------------------------ colsum, layernorm_bwd_params
Cols = collections.namedtuple("Cols", "R C ld profile")
COLS_CASES = [Cols(R, C, C + ld, p) for R in (1, 2, 1000) for (C, ld) in ((1, 1), (255, 3), (256, 8), (257, 5)) for p in ("exact", "scales", "outlier")]


def cols_inputs(c):
    """exact: integers in [-4, 4]; scales: N(0, 1), rows x 2^10 .. 2^-10 (the LAST row the smallest); outlier: scales with one column
    x 2^10 on top"""
    g = gen(113, c.R, c.C)
    if c.profile == "exact":
        x = torch.randint(-4, 5, (c.R, c.C), generator=g).to(F32)
    else:
        x = torch.randn(c.R, c.C, generator=g) * row_scales(c.R).flip(0)[:, None]
        if c.profile == "outlier":
            x[:, min(1, c.C - 1)] *= 1024.0
    return dict(x=x, case=c)


def cols_reference(d, dev=ident):
    c = d["case"]
    x = f64(d["x"], dev)
    s = cpu(x.sum(0))[None]
    if c.profile == "exact":
        return Ref({}, {"out": s.to(F32)})
    return Ref({"out": (s, cpu((c.R - 1) * e * x.abs().sum(0))[None])}, {})


def run_cols(ops, d, dev=ident, sync=lambda: None):
    c = d["case"]
    full = dev(nan(c.C + GUARD))
    ops.f32_colsum(operand(d["x"], c.ld, dev), full[:c.C], c.R, c.C)
    sync()
    full = full.cpu()
    assert untouched(full[c.C:]), f"colsum {case_id(c)}: elements >= C were written"
    return {"out": full[:c.C][None]}


Lnp = collections.namedtuple("Lnp", "R D lddy ldx profile")
LNP_CASES = [Lnp(R, D, D + a, D + b, p) for R in (1, 50) for (D, a, b) in ((1, 2, 1), (203, 5, 9), (256, 4, 1), (257, 3, 7)) for p in ("scales", "outlier")]


def lnp_inputs(c):
    """mean and rstd are handed in (not taken from a forward); scales: dy rows x 2^-10 .. 2^10; outlier: one column of dy and x x 2^10"""
    g = gen(127, c.R, c.D)
    dy, x = torch.randn(c.R, c.D, generator=g), torch.randn(c.R, c.D, generator=g) * 3
    if c.profile == "scales":
        dy *= row_scales(c.R)[:, None]
    else:
        dy[:, min(1, c.D - 1)] *= 1024.0
        x[:, min(1, c.D - 1)] *= 1024.0
    return dict(dy=dy, x=x, mean=torch.randn(c.R, generator=g) * 0.3, rstd=torch.rand(c.R, generator=g) + 0.25, case=c)


def lnp_reference(d, dev=ident):
    c = d["case"]
    dy, x, mean, rstd = (f64(d[k], dev) for k in ("dy", "x", "mean", "rstd"))
    t = dy * ((x - mean[:, None]) * rstd[:, None])
    return Ref({"dgamma": (cpu(t.sum(0))[None], cpu((c.R + 2) * e * t.abs().sum(0))[None]),
                "dbeta": (cpu(dy.sum(0))[None], cpu((c.R - 1) * e * dy.abs().sum(0))[None])}, {})


def run_lnp(ops, d, dev=ident, sync=lambda: None):
    c = d["case"]
    dg, db = dev(nan(c.D + GUARD)), dev(nan(c.D + GUARD))
    ops.f32_layernorm_bwd_params(operand(d["dy"], c.lddy, dev), operand(d["x"], c.ldx, dev), vec(d["mean"], dev), vec(d["rstd"], dev),
                                 dg[:c.D], db[:c.D], c.R, c.D)
    sync()
    dg, db = dg.cpu(), db.cpu()
    assert untouched(dg[c.D:]) and untouched(db[c.D:]), f"layernorm_bwd_params {case_id(c)}: elements >= D were written"
    return {"dgamma": dg[:c.D][None], "dbeta": db[:c.D][None]}


# ------------------------------------------------------------------------------------------------ transpose, gather_rows
TR_SIZES = (1, 31, 32, 33, 65)


def tr_rpads(R):
    return sorted({R, R + 1, cdiv(R, 32) * 32, R + 40})


def run_transpose(ops, R, C, Rpad, dev=ident, sync=lambda: None):
    """dst[c, r] = src[r, c], +0 for R <= r < Rpad; lds = C + 3, ldd = Rpad + 5: everything else of dst keeps its NaN"""
    src = torch.randn(R, C, generator=gen(131, R, C))
    full, dv = output(C, Rpad, Rpad + 5, dev)
    ops.f32_transpose(operand(src, C + 3, dev), dv, R, C, Rpad)
    sync()
    want = torch.zeros(C, Rpad)
    want[:, :R] = src.t()
    same_bits(owed(full, C, Rpad, f"transpose {R} x {C} -> Rpad {Rpad}"), want, f"transpose {R} x {C} -> Rpad {Rpad}")


GATHER_CASES = ((1, 1, (-1,)), (1, 1, (0,)), (6, 85, (4, -3, 0, 4, 4, -1)), (3, 257, (0, 4, 0)))
GATHER_SRC_ROWS = 5


def run_gather(ops, n, D, rows, dev=ident, sync=lambda: None):
    src = torch.randn(GATHER_SRC_ROWS, D, generator=gen(137, n, D))
    full, ov = output(n, D, None, dev)
    ops.f32_gather_rows(operand(src, None, dev), vec(torch.tensor(rows, dtype=I32), dev), ov, n, D)
    sync()
    want = torch.stack([src[r] if r >= 0 else torch.zeros(D) for r in rows])
    same_bits(owed(full, n, D, f"gather_rows {n} x {D}"), want, f"gather_rows {n} x {D} rows {rows}")


# ------------------------------------------------------------------------------------------------ attention backward
Attb = collections.namedtuple("Attb", "B S H G kstart profile")       # kstart: "0" | "mid" | "last" | "all" per batch row


def _ks(S, name):
    return {"0": 0, "mid": S // 2, "last": S - 1, "all": S}[name]


ATTB_CASES = ([Attb(3, 65, rep, 1, ("0", "mid", "all"), "scales") for rep in range(1, 9)]
              + [Attb(3, 64, H, G, ("mid", "last", "0"), "outlier") for (H, G) in ((12, 2), (28, 4), (16, 2))]
              + [Attb(3, S, 4, 2, ("0", "all", "last"), "scales") for S in (1, 2, 64)]
              + [Attb(3, 257, 6, 2, ("0", "last", "mid"), "outlier"), Attb(3, 257, 1, 1, ("mid", "0", "all"), "scales"),
                 Attb(3, 65, 7, 1, ("0", "mid", "last"), "outlier")])
ATTB_LONG = Attb(1, 2048, 8, 1, ("0",), "scales")


def attb_id(c):
    return f"B{c.B}-S{c.S}-{c.H}x{c.G}-{'.'.join(c.kstart)}-{c.profile}"


def attb_inputs(c):
    """q, k, v N(0, 1); scales: the rows of dout x 2^-10 .. 2^10 over the sequence; outlier: the dout of the FIRST query head of each
    group x 2^10 (its dK contribution sits beside the small heads' in the same sum)"""
    g = gen(139, c.B, c.S, c.H, c.G)
    qkv = torch.randn(c.B * c.S, (c.H + 2 * c.G) * HD, generator=g)
    dout = torch.randn(c.B, c.S, c.H, HD, generator=g)
    if c.profile == "scales":
        dout *= row_scales(c.S)[None, :, None, None]
    else:
        dout[:, :, ::c.H // c.G] *= 1024.0
    return dict(qkv=qkv, dout=dout.view(c.B * c.S, c.H * HD), kstart=torch.tensor([_ks(c.S, n) for n in c.kstart], dtype=I32), case=c)


def attb_group(q, k, v, do, lo, scale):
    """one batch row and KV group in float64: q, do [rep, S, 128], k, v [S, 128], keys [lo, s] for the queries s >= lo.
    Returns the values and bounds of dq [rep, S, 128], dk, dv [S, 128], lse, delta [rep, S]."""
    rep, S, _ = q.shape
    dvc = q.device
    ar = torch.arange(S, device=dvc)
    allow = ((ar[None, :] <= ar[:, None]) & (ar[None, :] >= lo) & (ar[:, None] >= lo))[None]
    z = torch.zeros((), dtype=F64, device=dvc)
    live = allow.any(-1, keepdim=True)
    nk = allow.sum(-1, keepdim=True).to(F64)
    s, A = (q @ k.t()) * scale, (q.abs() @ k.abs().t()) * scale
    m = torch.where(live, s.masked_fill(~allow, -math.inf).amax(-1, keepdim=True), z)
    d = torch.where(allow, s - m, z)
    p = torch.where(allow, torch.exp(d), z)
    l = torch.where(live, p.sum(-1, keepdim=True), z + 1)
    P = p / l
    Es = 21 * e * A
    dlt = torch.where(allow, e * (2 + 2 * d.abs()) + Es, z)
    bar = (P * dlt).sum(-1, keepdim=True)
    depth_l = torch.ceil(nk / 256) + 10
    rho = dlt + bar + e * (depth_l + 2)
    lse = torch.where(live, m + torch.log(l), z)
    E_lse = torch.where(live, e * lse.abs() + 4 * e * torch.log(l).abs() + 2 * e + e * depth_l + bar, z)
    dP, E_dP = do @ v.t(), 21 * e * (do.abs() @ v.abs().t())
    delta = (P * dP).sum(-1, keepdim=True)
    E_delta = ((P * dP).abs() * (rho + e + e * depth_l) + P * E_dP).sum(-1, keepdim=True)
    c = dP - delta
    E_c = E_dP + E_delta + e * c.abs()
    dS = P * c * scale
    E_dS = scale * (P * E_c + (P * c).abs() * (rho + 2 * e))
    dq = dS @ k
    E_dq = (E_dS + e * (torch.ceil(nk / 4) + 4) * dS.abs()) @ k.abs()
    one_key = (nk == 1)                                          # the query at s = kstart: P = 1, delta = dP, dS = 0 exactly
    assert not bool((dq.abs() * one_key).any())
    E_dq = torch.where(one_key, z, E_dq)
    d2 = torch.where(allow, s - lse, z)
    rel2 = torch.where(allow, e * (2 + 2 * d2.abs()) + Es + E_lse, z)
    E_dS2 = scale * (P * E_c + (P * c).abs() * (rel2 + 2 * e))
    depth_kv = (torch.ceil((S - ar).to(F64) / 4) * rep + 4)[None, :]             # per key j: nq = S - j
    dv = torch.einsum("hij,hid->jd", P, do)
    E_dv = torch.einsum("hij,hid->jd", P * (rel2 + e * depth_kv), do.abs())
    dk = torch.einsum("hij,hid->jd", dS, q)
    E_dk = torch.einsum("hij,hid->jd", E_dS2 + e * depth_kv * dS.abs(), q.abs())
    return dq, E_dq, dk, E_dk, dv, E_dv, lse[..., 0], E_lse[..., 0], delta[..., 0], E_delta[..., 0]


def attb_reference(d, dev=ident):
    c = d["case"]
    B, S, H, G, rep = c.B, c.S, c.H, c.G, c.H // c.G
    x, do = f64(d["qkv"], dev).view(B, S, H + 2 * G, HD), f64(d["dout"], dev).view(B, S, H, HD)
    out = {k: torch.zeros(B, S, H + 2 * G, HD, dtype=F64, device=x.device) for k in ("v", "E")}
    st = {k: torch.zeros(B, H, S, dtype=F64, device=x.device) for k in ("lse", "E_lse", "delta", "E_delta")}
    for b in range(B):
        lo = int(d["kstart"][b])
        for g in range(G):
            hs = slice(g * rep, (g + 1) * rep)
            r = attb_group(x[b, :, hs].transpose(0, 1), x[b, :, H + g], x[b, :, H + G + g], do[b, :, hs].transpose(0, 1), lo, HD ** -0.5)
            out["v"][b, :, hs], out["E"][b, :, hs] = r[0].transpose(0, 1), r[1].transpose(0, 1)
            out["v"][b, :, H + g], out["E"][b, :, H + g], out["v"][b, :, H + G + g], out["E"][b, :, H + G + g] = r[2], r[3], r[4], r[5]
            st["lse"][b, hs], st["E_lse"][b, hs], st["delta"][b, hs], st["E_delta"][b, hs] = r[6], r[7], r[8], r[9]
        assert not bool(out["v"][b, :lo].any() | out["E"][b, :lo].any() | st["lse"][b, :, :lo].any() | st["E_delta"][b, :, :lo].any())
    return Ref({"dqkv": (cpu(out["v"]).view(B * S, -1), cpu(out["E"]).view(B * S, -1)),
                "lse": (cpu(st["lse"]).view(B * H, S), cpu(st["E_lse"]).view(B * H, S)),
                "delta": (cpu(st["delta"]).view(B * H, S), cpu(st["E_delta"]).view(B * H, S))}, {})


def run_attb(ops, d, dev=ident, sync=lambda: None, zeros=True):
    """twice (lse / delta are a workspace the second launch reads), equal bits; rows before kstart hold +0 bit for bit and dQ of the
    query at kstart is 0 (zeros = False: left to the caller's check against the reference, for scoring the mutants)"""
    c = d["case"]
    B, S, H, G = c.B, c.S, c.H, c.G
    LD = (H + 2 * G) * HD
    qkv, dout, ks = operand(d["qkv"], None, dev), operand(d["dout"], None, dev), vec(d["kstart"], dev)
    res = []
    for _ in range(2):
        full, dv = output(B * S, LD, None, dev)
        lse, dl = dev(nan(B * H * S + GUARD)), dev(nan(B * H * S + GUARD))
        ops.f32_attn_bwd(qkv, dout, ks, dv, lse, dl, B, S, H, G, HD ** -0.5)
        sync()
        lse, dl = lse.cpu(), dl.cpu()
        assert untouched(lse[B * H * S:]) and untouched(dl[B * H * S:]), f"attn_bwd {attb_id(c)}: lse / delta written past B H S"
        res.append({"dqkv": owed(full, B * S, LD, f"attn_bwd {attb_id(c)}"), "lse": lse[:B * H * S].view(B * H, S), "delta": dl[:B * H * S].view(B * H, S)})
    for k in res[0]:
        same_bits(res[1][k], res[0][k], f"attn_bwd {attb_id(c)} second run, {k}")
    got = res[0]
    for b in range(B if zeros else 0):
        lo = int(d["kstart"][b])
        if lo:
            zq = got["dqkv"].view(B, S, LD)[b, :lo]
            same_bits(zq, torch.zeros_like(zq), f"attn_bwd {attb_id(c)}: dQ / dK / dV rows before kstart of batch row {b}")
            for name in ("lse", "delta"):
                zs = got[name].view(B, H, S)[b, :, :lo].contiguous()
                same_bits(zs, torch.zeros_like(zs), f"attn_bwd {attb_id(c)}: {name} before kstart of batch row {b}")
        if lo < S:
            assert not bool(got["dqkv"].view(B, S, LD)[b, lo, :H * HD].any()), f"attn_bwd {attb_id(c)}: dQ of the query at kstart is not 0"
    return got


# ------------------------------------------------------------------------------------------------ cross-attention
def ca_rows(dh):
    return 64 if dh <= 128 else (32 if dh <= 256 else 16)


def ca_kt(dh):
    return 64 if dh <= 256 else 32


def ca_plan(R, V, D, H):
    """plan_splits of csrc/f32_ca.hip restated: (splits, key tiles per split)"""
    dh = D // H
    rt, n_tiles = cdiv(R, ca_rows(dh)), cdiv(V, ca_kt(dh))
    want = cdiv(512, rt * H)
    s = max(1, min(want, 64, n_tiles // 4))
    per = cdiv(n_tiles, s)
    return cdiv(n_tiles, per), per


def ca_ws_floats(R, V, D, H):
    return ca_plan(R, V, D, H)[0] * R * (D + 2 * H)


Ca = collections.namedtuple("Ca", "dh H R V profile")
CA_DHS = (16, 128, 144, 256, 272, 512)
CA_PROFILES = ("n01", "onehot", "flat")


def ca_cases(dh):
    """R = 1 and the row-tile edge +- 1 (63 | 64 | 65 at dh <= 128 ...), V = 1, KT - 1, KT, KT + 1 and, at dh <= 256, 257 and 513 (nine
    tiles: two splits, the last tile one key), H = 1, 3 and (dh <= 64) 8; the three query profiles in turn, and the flat one at every
    V = KT + 1 (where an unmasked padding key would carry real mass); V = 1 also on the integer profile"""
    rows, kt = ca_rows(dh), ca_kt(dh)
    Rs = (1, rows - 1, rows, rows + 1) if dh <= 128 else (1, rows, rows + 1)
    Vs = (1, kt - 1, kt, kt + 1) + ((257, 513) if dh <= 256 else ())
    out, i = [], 0
    for H in (1, 3) + ((8,) if dh <= 64 else ()):
        for R in Rs:
            for V in Vs:
                out.append(Ca(dh, H, R, V, "flat" if V == kt + 1 else CA_PROFILES[i % 3]))
                i += 1
            out.append(Ca(dh, H, R, 1, "int"))
    return out


CA_MANY = Ca(64, 2, 1, 16385, "n01")                              # 257 tiles: 52 splits of 5, the last tile one key


def ca_inputs(c):
    """table N(0, 1); n01: q N(0, 0.15^2); onehot: n01 with every third row along one key x 40 / sqrt(dh); flat: n01 scaled by a
    power of two until every |score| <= 2^-6; int: q and the table integers in [-4, 4].  dout: N(0, 1), rows x 2^-10 .. 2^10."""
    D, g = c.dh * c.H, gen(149, c.dh, c.H, c.R, c.V)
    if c.profile == "int":
        table, q = (torch.randint(-4, 5, s, generator=g).to(F32) for s in ((c.V, D), (c.R, D)))
    else:
        table, q = torch.randn(c.V, D, generator=g), torch.randn(c.R, D, generator=g) * 0.15
    if c.profile == "onehot":
        for r in range(0, c.R, 3):
            q[r] = table[int(torch.randint(0, c.V, (1,), generator=g))] * (40.0 / c.dh ** 0.5)
    if c.profile == "flat":
        smax = float((q.to(F64).view(c.R, c.H, c.dh).transpose(0, 1) @ table.to(F64).view(c.V, c.H, c.dh).permute(1, 2, 0)).abs().max()) / c.dh ** 0.5
        q *= 2.0 ** math.floor(math.log2(2.0 ** -6 / smax))
    dout = torch.randn(c.R, D, generator=g) * row_scales(c.R)[:, None]
    return dict(q=q, table=table, dout=dout, case=c)


def ca_heads(t, H, dev=ident):
    n, D = t.shape
    return f64(t, dev).view(n, H, D // H).transpose(0, 1)          # [H, n, dh]


def ca_forward64(qh, kh, denom):
    s = (qh @ kh.transpose(1, 2)) / denom
    M = s.amax(-1, keepdim=True)
    p = torch.exp(s - M)
    L = p.sum(-1, keepdim=True)
    return s, M, L, p / L


def ca_forward_bounds(d, dev=ident):
    """the float64 forward in head layout [H, R, .] with its bounds: dict(qh, kh, denom, s, Es, out, E_out, lse, E_lse)"""
    c = d["case"]
    R, V, H, dh = c.R, c.V, c.H, c.dh
    denom = float(torch.tensor(dh ** 0.5, dtype=F32))
    qh, kh = ca_heads(d["q"], H, dev), ca_heads(d["table"], H, dev)
    s, M, L, P = ca_forward64(qh, kh, denom)
    if c.profile == "flat":
        assert float(s.abs().max()) <= 2.0 ** -6
    Z, T = ca_plan(R, V, dh * H, H)
    depth = ca_kt(dh) + 2 * T + 2 * (T + 1) + Z + 1 + 1
    Es = (dh + 1) * e * (qh.abs() @ kh.abs().transpose(1, 2)) / denom
    rel = Es + 2 * e * (s - M).abs() + e * depth
    bar = (P * rel).sum(-1, keepdim=True)
    E_out = (P * (rel + bar)) @ kh.abs() + TINY * (2 * kh.abs().sum(1, keepdim=True) + 2 * V)
    lse = M + torch.log(L)
    E_lse = e * lse.abs() + 4 * e * torch.log(L).abs() + 2 * e + bar
    return dict(qh=qh, kh=kh, denom=denom, s=s, Es=Es, out=P @ kh, E_out=E_out, lse=lse, E_lse=E_lse)


def ca_reference(d, dev=ident):
    """the forward: {"out" [R, D], "lse" [R, H]}; V = 1: out the table row's bits, and on the integer profile lse the quotient's"""
    c = d["case"]
    R, V, H, dh = c.R, c.V, c.H, c.dh
    f = ca_forward_bounds(d, dev)
    flat = lambda t: cpu(t.transpose(0, 1).reshape(R, -1))       # noqa: E731  [H, R, x] -> [R, H x]
    ref = Ref({"out": (flat(f["out"]), flat(f["E_out"])), "lse": (flat(f["lse"]), flat(f["E_lse"]))}, {})
    if V == 1:
        del ref.tol["out"]
        ref.exact["out"] = d["table"][:1].expand(R, -1).contiguous()
        if c.profile == "int":
            del ref.tol["lse"]
            sc = (d["q"].view(R, H, dh) * d["table"].view(1, H, dh)).sum(-1)        # integers below 2^24: exact in any order
            assert float((sc.to(F64) - flat(f["s"] * f["denom"])).abs().max()) < 1e-9
            ref.exact["lse"] = sc / torch.tensor(f["denom"], dtype=F32)
        else:
            ref.tol["lse"] = (flat(f["lse"]), flat(f["Es"]))                     # the score itself: M + logf(1)
    return ref


def ca_handed(d, dev=ident):
    """what the backward is handed: the float64 forward rounded to fp32 (out [R, D], lse [R, H])"""
    c = d["case"]
    qh, kh = ca_heads(d["q"], c.H, dev), ca_heads(d["table"], c.H, dev)
    _, M, L, P = ca_forward64(qh, kh, float(torch.tensor(c.dh ** 0.5, dtype=F32)))
    return cpu((P @ kh).transpose(0, 1).reshape(c.R, -1)).to(F32), cpu((M + torch.log(L)).transpose(0, 1).reshape(c.R, -1)).to(F32)


def ca_bwd64(qh, kh, oh, gh, lse, denom):
    """the backward's definition on its operands [H, n, dh], lse [H, R, 1]: (dq, s, p, dP, delta, c, dS)"""
    s = (qh @ kh.transpose(1, 2)) / denom
    p = torch.exp(s - lse)
    dP = gh @ kh.transpose(1, 2)
    delta = (gh * oh).sum(-1, keepdim=True)
    c = dP - delta
    dS = p * c / denom
    return dS @ kh, s, p, dP, delta, c, dS


def ca_bwd_reference(d, out32=None, lse32=None, dev=ident):
    """out32 / lse32 given: the backward on exactly these operands.  None (the chain): the backward is handed the forward
    kernel's own out and lse, the reference is the float64 gradient of the definition, and the forward's bounds enter where the
    operands are read: E_out in delta (sum |dout| E_out), E_lse in the argument of expf(s - lse)."""
    c = d["case"]
    R, V, H, dh = c.R, c.V, c.H, c.dh
    f = ca_forward_bounds(d, dev)
    qh, kh, denom, gh = f["qh"], f["kh"], f["denom"], ca_heads(d["dout"], H, dev)
    if out32 is None:
        oh, lse, E_oh, E_ls = f["out"], f["lse"], f["E_out"], f["E_lse"]
    else:
        oh, lse, E_oh, E_ls = ca_heads(out32, H, dev), f64(lse32, dev).t()[:, :, None], 0.0, 0.0
    dq, s, p, dP, delta, cc, dS = ca_bwd64(qh, kh, oh, gh, lse, denom)
    tpr = 512 // ca_rows(dh)
    E_dl = (cdiv(dh, tpr) + int(math.log2(tpr)) + 1) * e * (gh * oh).abs().sum(-1, keepdim=True) + (gh.abs() * E_oh).sum(-1, keepdim=True)
    rel_p = 2 * e + 2 * e * (s - lse).abs() + f["Es"] + E_ls
    E_c = dh * e * (gh.abs() @ kh.abs().transpose(1, 2)) + E_dl + e * cc.abs()
    E_dS = (p * E_c + (p * cc).abs() * (rel_p + 2 * e)) / denom
    Z, T = ca_plan(R, V, dh * H, H)
    E_dq = (E_dS + e * (ca_kt(dh) + T + Z) * dS.abs()) @ kh.abs() + TINY * 2 * ((cc.abs() / denom + 1) @ (kh.abs() + 1))
    return Ref({"dq": (cpu(dq.transpose(0, 1).reshape(R, -1)), cpu(E_dq.transpose(0, 1).reshape(R, -1)))}, {})


CA_PAD = dict(ldq=4, ldo=3, lddo=8, lddq=5)                         # floats beyond D (ldq and lddo multiples of 4: the entry point's rule)


def run_ca(ops, d, dev=ident, sync=lambda: None, splits=None):
    """the plain form once, the lse form twice on a NaN workspace of exactly the owed size: {"out", "lse"}; the lse form's out and
    the second run bit-equal.  splits: the split count the library is asked to confirm (the GPU file), else the restated plan."""
    c = d["case"]
    R, V, H, D = c.R, c.V, c.H, c.dh * c.H
    q, table = operand(d["q"], D + CA_PAD["ldq"], dev), operand(d["table"], None, dev)
    n_ws = ca_ws_floats(R, V, D, H)
    res = []
    for form in ("plain", "lse", "lse"):
        ws = dev(nan(n_ws + GUARD))
        full, ov = output(R, D, D + CA_PAD["ldo"], dev)
        if form == "plain":
            ops.f32_ca_attn(q, table, ov, R, H, ws=ws[:n_ws])
            lf = None
        else:
            lf, lv = output(R, H, None, dev)
            ops.f32_ca_attn_lse(q, table, ov, lv, R, H, ws=ws[:n_ws])
        sync()
        assert untouched(ws.cpu()[n_ws:]), f"ca_attn {case_id(c)}: the workspace was written past its size"
        r = {"out": owed(full, R, D, f"ca_attn {case_id(c)} out")}
        if lf is not None:
            r["lse"] = owed(lf, R, H, f"ca_attn {case_id(c)} lse")
        res.append(r)
    same_bits(res[1]["out"], res[0]["out"], f"ca_attn {case_id(c)}: the lse form's out against the plain form's")
    same_bits(res[2]["out"], res[1]["out"], f"ca_attn {case_id(c)}: second run, out")
    same_bits(res[2]["lse"], res[1]["lse"], f"ca_attn {case_id(c)}: second run, lse")
    return res[1]


def run_ca_bwd(ops, d, out32, lse32, dev=ident, sync=lambda: None):
    c = d["case"]
    R, V, H, D = c.R, c.V, c.H, c.dh * c.H
    q, table = operand(d["q"], D + CA_PAD["ldq"], dev), operand(d["table"], None, dev)
    o, g, ls = operand(out32, D + CA_PAD["ldo"], dev), operand(d["dout"], D + CA_PAD["lddo"], dev), operand(lse32, None, dev)
    n_ws = ca_ws_floats(R, V, D, H)
    res = []
    for _ in range(2):
        ws = dev(nan(n_ws + GUARD))
        full, dv = output(R, D, D + CA_PAD["lddq"], dev)
        ops.f32_ca_attn_bwd(q, table, o, g, ls, dv, R, H, ws=ws[:n_ws])
        sync()
        assert untouched(ws.cpu()[n_ws:]), f"ca_attn_bwd {case_id(c)}: the workspace was written past its size"
        res.append({"dq": owed(full, R, D, f"ca_attn_bwd {case_id(c)}")})
    same_bits(res[1]["dq"], res[0]["dq"], f"ca_attn_bwd {case_id(c)}: second run")
    return res[0]


# ------------------------------------------------------------------------------------------------ the older metrics (for the mutant table)
def old_ca_metric(got, ref, H):
    """the per-head max |err| / max |ref| of the older cross-attention tests (bar 2e-5)"""
    R = ref.shape[0]
    g, r = got.to(F64).view(R, H, -1), ref.to(F64).view(R, H, -1)
    return float(((g - r).abs().amax((0, 2)) / r.abs().amax((0, 2)).clamp_min(1e-30)).max())
