"""TEST HELPER (not a test, never shipped): plain float64 restatements of Qwen3's per-head q/k RMSNorm in the fp32 family --
tasu_f32_qk_norm_rope, tasu_f32_qk_norm_bwd (csrc/qk_norm.hip) and tasu_f32_gemm_qkv_norm_rope (csrc/fp32.hip) -- on the exact fp32
input values, each with a first-order bound E for every element it returns.  Nothing is shared with the kernels or with
tests/qwen3_f32_ops.py.  `check`, `worst_of`, `same_bits`, `untouched`, `nan`, e = 2^-24 and LIMIT = 1.0 are those of
tests/row_ref64.py; the guarded buffers, the GEMM inputs and their bound F (`gemm_inputs`, `gemm_sum`), the rotation tables and
`cache_check` those of tests/f32_ref64.py, whose rules hold here: an fp32 +, * : e relative; rsqrtf 4 e; a fixed-order sum of terms
t_i carries depth . e . sum |t_i|.

    forward   per row and q / k head, x = the 128 fp32 values of the projection (each known to within F_x: 0 for the row kernel, the
              GEMM's F behind the fused entry point), w the head's fp32 weight, (c, s) the row's table:
                  r = (mean_128 x^2 + eps)^(-1/2)        y = w (x r)        out = (y1 c - y2 s | y2 c + y1 s),  (y1, y2) = dims (d, d + 64)
              Where the fp32 kernel can differ from float64:
                * r.  ss = sum x^2 is 4 serial FMAs per lane and 5 shuffle levels: 9 roundings, every term >= 0, so 9 e relative on
                  ss; ss / 128 is exact and + eps one rounding: 10 e on the argument (both parts are <= the argument), halved by
                  the inverse square root: 5 e; rsqrtf's own 4 e.  rel_r = R_E e + sum |x| F_x / (ss + 128 eps), R_E = 5 + 4 = 9
                  (the second term: d log r = - sum x dx / (ss + 128 eps)).
                * y = fl(w fl(x r)): two rounded products.  A_y = |w| r F_x + |y| (rel_r + 2 e).
                * the rotation, products and sum rounded separately (tests/f32_ref64.py rope_ref):
                  E_1 = |c| A_y1 + |s| A_y2 + e (|y1 c| + |y2 s| + |out_1|), E_2 likewise.
              An all-zero head: r = eps^(-1/2), out = 0 as a value (E = 0).  v heads: the input's bits (row kernel) / the GEMM's
              sum within F (fused).  rstd: rel_r r.
    backward  g = the fp32 gradient w.r.t. y, rstd an fp32 INPUT (the float64 r rounded once: the same values go to both):
                  wg = w g     xn = x rstd     m = mean_128(wg xn)     dpre = rstd (wg - xn m)
              wg and xn one rounding each; the terms wg xn carry 2 e from their factors and pass 4 serial FMAs + 5 shuffle levels
              (DEPTH = 9), the scaling by 1 / 128 is exact: E_m = (DEPTH + 2) e mean |wg xn|.  wg - xn m: e |wg| + 2 e |xn m|
              (xn's rounding, the product's -- absent where the compiler contracts it into the subtraction) + |xn| E_m + e of the
              difference; the product with rstd e |dpre|:
                  E = rstd (e |wg| + 2 e |xn m| + |xn| E_m) + 2 e |dpre|.          v block: dqkv's bits.
    append    no arithmetic of its own: with a cache, out is what it is without one and cache[m, slot[m]] holds the BITS of out's k
              and v heads of row m; every other cell keeps its bits.
    fused     tasu_f32_gemm_qkv_norm_rope: the float64 product (+ bias) with f32_ref64's bound F = (K + 2) e (sum |a w| + |bias|)
              through the forward above with F_x = F; the v heads within F.

The module also holds the cases, the seeded inputs with their NaN guards, the fp32 torch restatement (F32QkTorch, HipOps' method
names) and the runs that tests/test_qk_norm_f32_ref64_cpu.py (the restatement and its mutants) and tests/test_gpu_qk_norm_f32_f64.py
(HipOps) share."""
import collections

import torch

from f32_ref64 import (CTX_QKV, EPS, F32, F64, GUARD, HD, I32, Gemm, cache_check, case_id, gemm_inputs, gemm_sum, ident, operand,  # noqa: F401
                       output, owed, rope_eager, rope_tables, vec)
from row_ref64 import LIMIT, Ref, check, e, gen, nan, same_bits, untouched, worst_of  # noqa: F401

R_E = 9.0                                                        # rel_r = R_E e without an input error
DEPTH = 9                                                        # 4 serial FMAs + 5 shuffle levels

Case = collections.namedtuple("Case", "M H G profile")
SHAPES = [(M, H, G) for M in (1, 3, 17, 64, 65) for (H, G) in ((2, 1), (3, 3), (12, 2), (16, 8))]
PROFILES = ("n01", "scales", "special")                          # N(0, 1) | heads x 1e4 / x 1e-4 | an all-zero head and a one-hot head
CASES = [Case(M, H, G, p) for (M, H, G) in SHAPES for p in PROFILES]
CTX = 7


def inputs(c):
    """weights 1 + 0.5 N(0, 1) with a negative one forced in each; the gradient 0.25 N(0, 1); slots spread over [0, CTX)"""
    M, H, G, profile = c
    NH = H + 2 * G
    g = gen(23, M, H, G, PROFILES.index(profile))
    pre = torch.randn(M, NH, HD, generator=g)
    if profile == "scales":
        k = (torch.arange(M)[:, None] + torch.arange(NH)[None]) % 3
        pre = pre * torch.where(k == 0, 1e4, torch.where(k == 1, 1e-4, 1.0))[..., None]
    if profile == "special":
        pre[M - 1, 0] = 0.0                                      # r = rsqrt(eps)
        pre[0, H] = 0.0
        pre[0, H, 37] = 1.75                                     # a one-hot k head
    wq, wk = 1.0 + 0.5 * torch.randn(HD, generator=g), 1.0 + 0.5 * torch.randn(HD, generator=g)
    wq[3], wk[70], wq[127] = -0.75, -1.25, -0.5
    cos, sin = rope_tables(M, g)
    dy = torch.randn(M, NH, HD, generator=g) * 0.25
    slot = ((torch.arange(M) * 5 + 3) % CTX).to(I32)
    return dict(pre=pre.view(M, NH * HD), dy=dy.view(M, NH * HD), wq=wq, wk=wk, cos=cos, sin=sin, slot=slot, M=M, H=H, G=G, eps=EPS, case=c)


def _weights(d):
    H, G = d["H"], d["G"]
    return torch.cat([d["wq"].to(F64)[None].expand(H, HD), d["wk"].to(F64)[None].expand(G, HD)])[None]      # [1, H+G, 128]


def norm_rope_ref(x, Fx, d):
    """x, Fx [M, H + 2G, 128] float64 -> (out, E) [M, H + 2G, 128], (r, E_r) [M, H + G]"""
    H, G, eps = d["H"], d["G"], d["eps"]
    xq, F = x[:, :H + G], Fx[:, :H + G]
    w = _weights(d)
    ss = xq.pow(2).sum(-1, keepdim=True)
    r = (ss / HD + eps).rsqrt()
    rel_r = R_E * e + (xq.abs() * F).sum(-1, keepdim=True) / (ss + HD * eps)
    y = w * (xq * r)
    A = w.abs() * r * F + y.abs() * (rel_r + 2 * e)
    c, s = d["cos"].to(F64)[:, None], d["sin"].to(F64)[:, None]
    y1, y2, A1, A2 = y[..., :64], y[..., 64:], A[..., :64], A[..., 64:]
    o1, o2 = y1 * c - y2 * s, y2 * c + y1 * s
    E1 = c.abs() * A1 + s.abs() * A2 + e * ((y1 * c).abs() + (y2 * s).abs() + o1.abs())
    E2 = c.abs() * A2 + s.abs() * A1 + e * ((y2 * c).abs() + (y1 * s).abs() + o2.abs())
    out = torch.cat([torch.cat([o1, o2], -1), x[:, H + G:]], 1)
    E = torch.cat([torch.cat([E1, E2], -1), Fx[:, H + G:]], 1)
    return out, E, r[..., 0], (rel_r * r)[..., 0]


def fwd_reference(d, want_rstd=True):
    M, H, G = d["M"], d["H"], d["G"]
    x = d["pre"].to(F64).view(M, H + 2 * G, HD)
    out, E, r, Er = norm_rope_ref(x, torch.zeros_like(x), d)
    tol = {"qk": (out[:, :H + G].reshape(M, -1), E[:, :H + G].reshape(M, -1))}
    if want_rstd:
        tol["rstd"] = (r, Er)
    return Ref(tol, {"v": d["pre"].view(M, H + 2 * G, HD)[:, H + G:].reshape(M, -1).contiguous()})


def bwd_rstd(d):
    """the backward's rstd input: the float64 statistic rounded once to fp32"""
    M, H, G = d["M"], d["H"], d["G"]
    x = d["pre"].to(F64).view(M, H + 2 * G, HD)[:, :H + G]
    return (x.pow(2).mean(-1) + d["eps"]).rsqrt().to(F32)


def bwd_reference(d):
    M, H, G = d["M"], d["H"], d["G"]
    x = d["pre"].to(F64).view(M, H + 2 * G, HD)[:, :H + G]
    g = d["dy"].to(F64).view(M, H + 2 * G, HD)[:, :H + G]
    r = bwd_rstd(d).to(F64)[..., None]
    wg, xn = _weights(d) * g, x * r
    m = (wg * xn).mean(-1, keepdim=True)
    dx = r * (wg - xn * m)
    E_m = (DEPTH + 2) * e * (wg * xn).abs().mean(-1, keepdim=True)
    E = r * (e * wg.abs() + 2 * e * (xn * m).abs() + xn.abs() * E_m) + 2 * e * dx.abs()
    return Ref({"qk": (dx.reshape(M, -1), E.reshape(M, -1))}, {"v": d["dy"].view(M, H + 2 * G, HD)[:, H + G:].reshape(M, -1).contiguous()})


def split(t, d):
    W = (d["H"] + d["G"]) * HD
    return {"qk": t[:, :W].contiguous(), "v": t[:, W:].contiguous()}


# ------------------------------------------------------------------------------------------------ the fp32 restatement
class F32QkTorch:
    """plain torch fp32 on the CPU under HipOps' names and signatures; outputs are written into the caller's views"""

    def _w(self, wq, wk, H, G):
        return torch.cat([wq[:HD].view(1, HD).expand(H, HD), wk[:HD].view(1, HD).expand(G, HD)])[None]

    def _stat(self, x, eps):
        return torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)

    def _norm(self, x, w, eps):
        r = self._stat(x, eps)
        return w * (x * r), r

    def _head(self, x, w, cos, sin, eps):
        y, r = self._norm(x, w, eps)
        return rope_eager(y, cos, sin), r

    def f32_qk_norm_rope(self, pre, wq, wk, cos, sin, out, rstd, M, H, G, eps, kc=None, vc=None, slot=None, ctx=0):
        x = pre[:M].view(M, H + 2 * G, HD).clone()
        o = out[:M].view(M, H + 2 * G, HD)
        y, r = self._head(x[:, :H + G], self._w(wq, wk, H, G), cos[:M], sin[:M], eps)
        o[:, :H + G] = y
        o[:, H + G:] = x[:, H + G:]
        if rstd is not None:
            rstd[:M].view(M, H + G).copy_(r[..., 0])
        if kc is not None:
            rows, sl = torch.arange(M), slot[:M].long()
            kc.view(-1, ctx, G * HD)[rows, sl] = o[:, H:H + G].reshape(M, -1)
            vc.view(-1, ctx, G * HD)[rows, sl] = o[:, H + G:].reshape(M, -1)

    def _dpre(self, wg, xn, r):
        return r * (wg - xn * (wg * xn).mean(-1, keepdim=True))

    def f32_qk_norm_bwd(self, dqkv, pre, wq, wk, rstd, M, H, G):
        x = pre[:M].view(M, H + 2 * G, HD)[:, :H + G]
        g = dqkv[:M].view(M, H + 2 * G, HD)
        r = rstd[:M].view(M, H + G, 1)
        g[:, :H + G] = self._dpre(self._w(wq, wk, H, G) * g[:, :H + G], x * r, r)

    def f32_gemm(self, a, w, c, M, N, K, bias=None, resid=None, act=0, ws=None):
        v = a[:M, :K] @ w[:N, :K].t()
        c[:M, :N] = v + bias[:N] if bias is not None else v

    def f32_gemm_qkv_norm_rope(self, a, wqkv, bias, qkv, wq, wk, cos, sin, M, H, G, K, eps, ws, kc=None, vc=None, slot=None, ctx=0):
        self.f32_gemm(a, wqkv, qkv, M, (H + 2 * G) * HD, K, bias=bias)
        self.f32_qk_norm_rope(qkv, wq, wk, cos, sin, qkv, None, M, H, G, eps, kc, vc, slot, ctx)


# ------------------------------------------------------------------------------------------------ the runs
def _tables(d, dev):
    return vec(d["wq"], dev), vec(d["wk"], dev), operand(d["cos"], None, dev), operand(d["sin"], None, dev)


def run_fwd(ops, d, dev=ident, sync=lambda: None, alias=False, want_rstd=True, cache=False):
    """out / rstd / the caches start as NaN with guard rows that must keep their bits; ``alias``: out == pre; twice, equal bits"""
    M, H, G = d["M"], d["H"], d["G"]
    N = (H + 2 * G) * HD
    res = []
    for _ in range(2):
        pf, pv = output(M, N, None, dev, init=d["pre"])
        of, ov = (pf, pv) if alias else output(M, N, None, dev)
        rf, rv = output(M, H + G, None, dev) if want_rstd else (None, None)
        kc = dev(nan(M + GUARD, CTX, G * HD)) if cache else None
        vc = dev(nan(M + GUARD, CTX, G * HD)) if cache else None
        ops.f32_qk_norm_rope(pv, *_tables(d, dev), ov, rv, M, H, G, d["eps"], kc=kc, vc=vc, slot=vec(d["slot"], dev) if cache else None,
                             ctx=CTX if cache else 0)
        sync()
        o = owed(of, M, N, "f32_qk_norm_rope out")
        if not alias:
            same_bits(owed(pf, M, N, "f32_qk_norm_rope pre"), d["pre"], "f32_qk_norm_rope: the input was changed")
        got = split(o, d)
        if want_rstd:
            got["rstd"] = owed(rf, M, H + G, "f32_qk_norm_rope rstd")
        if cache:
            cache_check(kc.cpu(), vc.cpu(), o, d["slot"], M, H, G, CTX, f"f32_qk_norm_rope {case_id(d['case'])}")
        res.append(got)
    for k in res[0]:
        same_bits(res[1][k], res[0][k], f"f32_qk_norm_rope {case_id(d['case'])} second run, {k}")
    return res[0]


def run_bwd(ops, d, dev=ident, sync=lambda: None):
    M, H, G = d["M"], d["H"], d["G"]
    N = (H + 2 * G) * HD
    res = []
    for _ in range(2):
        gf, gv = output(M, N, None, dev, init=d["dy"])
        pf, pv = output(M, N, None, dev, init=d["pre"])
        ops.f32_qk_norm_bwd(gv, pv, vec(d["wq"], dev), vec(d["wk"], dev), operand(bwd_rstd(d), None, dev), M, H, G)
        sync()
        same_bits(owed(pf, M, N, "f32_qk_norm_bwd pre"), d["pre"], "f32_qk_norm_bwd: pre was changed")
        res.append(split(owed(gf, M, N, "f32_qk_norm_bwd dqkv"), d))
    for k in res[0]:
        same_bits(res[1][k], res[0][k], f"f32_qk_norm_bwd {case_id(d['case'])} second run, {k}")
    return res[0]


# ---- the fused entry point
Fused = collections.namedtuple("Fused", "M H G K bias ws cache")


def fused_inputs(c, profile="n01"):
    N = (c.H + 2 * c.G) * HD
    d = gemm_inputs(Gemm("tile", c.M, N, c.K, 0, c.bias, False, profile, 0, 0, 0, 16 * 64 * N if c.ws else 0))
    g = gen(29, c.M, c.H, c.G, c.K)
    d["wq"], d["wk"] = 1.0 + 0.5 * torch.randn(HD, generator=g), 1.0 + 0.5 * torch.randn(HD, generator=g)
    d["wq"][3], d["wk"][70] = -0.75, -1.25
    d["cos"], d["sin"] = rope_tables(c.M, g)
    d["slot"] = ((torch.arange(c.M) * 3 + 1) % CTX).to(I32)
    d.update(M=c.M, H=c.H, G=c.G, eps=EPS, fused=c)
    return d


def fused_reference(d):
    c = d["fused"]
    s, F = gemm_sum(d)
    NH = c.H + 2 * c.G
    out, E, _, _ = norm_rope_ref(s.view(c.M, NH, HD), F.view(c.M, NH, HD), d)
    return Ref({"qkv": (out.reshape(c.M, -1), E.reshape(c.M, -1))}, {})


def run_fused(ops, d, dev=ident, sync=lambda: None, unfused=False, w=None):
    """{"qkv", "kc", "vc"} of the fused entry point -- or, ``unfused``, of f32_gemm followed by f32_qk_norm_rope in place; ``w``:
    the weight operand to hand over (a fragment-order copy) instead of the guarded row-major one"""
    c = d["fused"]
    M, H, G, K = c.M, c.H, c.G, c.K
    N = (H + 2 * G) * HD
    a = operand(d["a"], K + 4, dev)
    w = operand(d["w"], K + 8, dev) if w is None else w
    ws = dev(nan(16 * 64 * N)) if c.ws else None
    qf, qv = output(M, N, None, dev)
    kc = dev(nan(M + GUARD, CTX, G * HD)) if c.cache else None
    vc = dev(nan(M + GUARD, CTX, G * HD)) if c.cache else None
    bias = vec(d["bias"], dev) if d["bias"] is not None else None
    kw = dict(kc=kc, vc=vc, slot=vec(d["slot"], dev) if c.cache else None, ctx=CTX if c.cache else 0)
    if unfused:
        ops.f32_gemm(a, w, qv, M, N, K, bias=bias, ws=ws)
        ops.f32_qk_norm_rope(qv, *_tables(d, dev), qv, None, M, H, G, d["eps"], **kw)
    else:
        ops.f32_gemm_qkv_norm_rope(a, w, bias, qv, *_tables(d, dev), M, H, G, K, d["eps"], ws, **kw)
    sync()
    got = {"qkv": owed(qf, M, N, "f32_gemm_qkv_norm_rope qkv")}
    if c.cache:
        got["kc"], got["vc"] = kc.cpu(), vc.cpu()
        cache_check(got["kc"], got["vc"], got["qkv"], d["slot"], M, H, G, CTX, f"f32_gemm_qkv_norm_rope {case_id(c)}")
    return got
