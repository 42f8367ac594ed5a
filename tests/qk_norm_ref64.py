"""TEST HELPER (not a test, never shipped): plain float64 restatements of Qwen3's per-head q/k RMSNorm kernels -- tasu_qk_norm_rope_fwd,
tasu_qk_norm_bwd, tasu_qk_norm_rope_append (csrc/qk_norm.hip) -- on the exact input values, each with a first-order bound E for
every element it returns.  Nothing is shared with the kernels or with tests/qwen3_ops.py.  `check`, `worst_of`, `same_bits`,
`untouched`, `nan`, U = 2^-8 and e = 2^-24 are those of tests/row_ref64.py, `bf16r` that of tests/lora_ref64.py, the fp32 table
(an INPUT: the same values go to the kernel and to the reference) that of tests/point_ref64.py.  LIMIT = 1.0.

    forward   per row and q / k head, x = the 128 bf16 values of the projection, w the head's fp32 weight, (c, s) the row's table:
                  r  = (mean x^2 + eps)^(-1/2)            t = x r            xh = bf16(t)            y = w xh
                  out = bf16(y1 c - y2 s | y2 c + y1 s),   (y1, y2) = dims (d, d + 64)
              Where the fp32 kernel can differ from float64:
                * r.  ss = sum x^2 is 8 serial FMAs per lane and 4 shuffle levels (12 roundings, all terms >= 0: 12 e relative),
                  the scaling by 1 / 128 is exact, + eps one rounding, rsqrtf 2 ulp = 4 e (what the project grants it): on r half
                  of the sum's error and rsqrtf's own, E_r = R_E e r with R_E = 6 + 1 + 4 = 11.
                * xh.  The kernel rounds t' = fl32(x r') with |t' - t| <= T_E e |t|, T_E = R_E + 1.  If no bf16 rounding boundary
                  (a midpoint between neighbours) lies within that distance of t, xh is bf16(t) EXACTLY -- the bound then grants
                  the intermediate rounding nothing and so sees it missing.  If one does (`near_tie`; a few elements in ten
                  thousand), xh may land on either neighbour: one bf16 ulp of t, A_xh = ulp(t), which reaches the output scaled by
                  |w| (|c| + |s|) over the pair.
                * y = w xh one rounded product; the rotation one rounded product and one FMA (rope_pair_f): 2^-22 of the two
                  products' magnitudes, as tests/point_ref64.py grants tasu_rope_fwd, + e of them for y's own rounding.
                * the store: u |out|.
              E = u |out| + (1 + u) [(2^-22 + e) (|y1 c| + |y2 s|) + |c| A1 + |s| A2],  A = |w| A_xh of the element the factor
              multiplies.  An all-zero head: r = eps^(-1/2), out = 0 as a value (E = 0).  v heads: the input's bits.
              rstd: E_r.
    backward  g = the bf16 gradient w.r.t. y, rstd an fp32 INPUT (the float64 r rounded once: the same values go to both):
                  xn = x rstd     dot = mean_128(w g xn)     dpre = bf16(rstd (w g - xn dot))
              (the rounding of xh is the identity here, as the kernel's contract states).  The form of row_ref64's RMSNorm backward
              with depth = 12 (8 serial FMAs + 4 shuffle levels):  E_dot = (depth + 4) e sum |w g xn| / 128,
              A = rstd (3 e |w g| + 4 e |xn dot| + |xn| E_dot) + e |dpre|,  E = u |dpre| + (1 + u) A.  v block: dqkv's bits.
    append    no arithmetic of its own: qkv in place and the cells cache[row, pos[row]] carry the BITS of the forward kernel's
              output on the same rows; every other cell keeps its bits (`run_append`).

The module also holds the cases, the seeded inputs with their NaN guards and the runs that tests/test_qk_norm_ref64_cpu.py (the
torch double) and tests/test_gpu_qk_norm_f64.py (HipOps) share."""
import collections

import torch

from lora_ref64 import bf16r
from point_ref64 import guarded_flat, guarded_rows, normal, table_f32, twice
from row_ref64 import BF, F32, F64, GUARD, I32, LIMIT, NAN, U, Ref, _back, _call, check, e, gen, nan, same_bits, untouched, worst_of  # noqa: F401

HD = 128
EPS = 1e-6
R_E = 11.0                                                       # E_r = R_E e r
T_E = R_E + 1.0                                                  # |fl32(x r') - x r| <= T_E e |x r|
DEPTH = 12

Case = collections.namedtuple("Case", "M H G")
CASES = [Case(5, 2, 1), Case(64, 12, 2), Case(67, 16, 8)]        # an odd row count, one whole 64-row chunk, one row past it; both head ratios
FIXED_POS = [0, 1, 4095]


def case_id(c):
    return "-".join(str(v) for v in c)


def inputs(c):
    """N(0, 1) heads; every third (row + head) scaled by 1e-3, where eps decides the result; head 1 of row 2 all zero; weights
    1 + 0.5 N(0, 1) with a negative one forced in each"""
    M, H, G = c
    NH = H + 2 * G
    g = gen(M, H, G, 17)
    pre = torch.randn(M, NH, HD, generator=g)
    small = ((torch.arange(M)[:, None] + torch.arange(NH)[None]) % 3 == 0)
    pre = torch.where(small[..., None], pre * 1e-3, pre)
    pre[min(2, M - 1), 1] = 0.0
    pre = pre.to(BF)
    wq, wk = (1.0 + 0.5 * torch.randn(HD, generator=g)).to(F32), (1.0 + 0.5 * torch.randn(HD, generator=g)).to(F32)
    wq[3], wk[70], wq[127] = -0.75, -1.25, -0.5
    pos = torch.tensor((FIXED_POS + torch.randint(0, 4096, (M,), generator=g).tolist())[:M], dtype=I32)
    cs, sn = table_f32(pos)
    dy = (torch.randn(M, NH, HD, generator=g) * 0.25).to(BF)
    return dict(pre=pre.view(M, NH * HD), dy=dy.view(M, NH * HD), wq=wq, wk=wk, pos=pos, cos=cs, sin=sn, M=M, H=H, G=G, eps=EPS)


def _weights(d):
    H, G = d["H"], d["G"]
    return torch.cat([d["wq"].to(F64)[None].expand(H, HD), d["wk"].to(F64)[None].expand(G, HD)])[None]      # [1, H+G, 128]


def _ulp_bf16(t):
    """the spacing of bf16 at |t| (float64; t != 0)"""
    return torch.exp2(torch.floor(torch.log2(t.abs())) - 7)


def near_tie(t, rel):
    """a bf16 rounding boundary lies within rel |t| of t"""
    a = torch.where(t == 0, torch.ones_like(t), t.abs())
    lo = bf16r(a)                                                # the nearest bf16; the boundaries around it: half a spacing away,
    ulp = _ulp_bf16(lo)                                          # below a power of two half of the FINER spacing
    below = torch.where(lo == torch.exp2(torch.floor(torch.log2(lo))), ulp / 4, ulp / 2)
    dist = torch.minimum((a - (lo - below)).abs(), (a - (lo + ulp / 2)).abs())
    return (t != 0) & (dist <= rel * a)


def fwd_reference(d):
    M, H, G = d["M"], d["H"], d["G"]
    x = d["pre"].to(F64).view(M, H + 2 * G, HD)[:, :H + G]
    w = _weights(d)
    r = (x.pow(2).mean(-1) + d["eps"]).rsqrt()
    t = x * r[..., None]
    safe = torch.where(t == 0, torch.ones_like(t), t)
    xh = torch.where(t == 0, t, bf16r(safe))
    A = torch.where(near_tie(t, T_E * e), _ulp_bf16(safe), torch.zeros_like(t)) * w.abs()
    y = w * xh
    c, s = d["cos"].to(F64)[:, None], d["sin"].to(F64)[:, None]
    y1, y2, A1, A2 = y[..., :64], y[..., 64:], A[..., :64], A[..., 64:]
    out = torch.cat([y1 * c - y2 * s, y2 * c + y1 * s], -1)
    slop = torch.cat([(y1 * c).abs() + (y2 * s).abs(), (y2 * c).abs() + (y1 * s).abs()], -1)
    tie = torch.cat([c.abs() * A1 + s.abs() * A2, c.abs() * A2 + s.abs() * A1], -1)
    E = U * out.abs() + (1 + U) * ((2.0 ** -22 + e) * slop + tie)
    normal(out, "qk_norm_rope_fwd")
    v = d["pre"].view(M, H + 2 * G, HD)[:, H + G:].reshape(M, -1).contiguous()
    return Ref({"qk": (out.reshape(M, -1), E.reshape(M, -1)), "rstd": (r, R_E * e * r)}, {"v": v})


def bwd_reference(d):
    M, H, G = d["M"], d["H"], d["G"]
    x = d["pre"].to(F64).view(M, H + 2 * G, HD)[:, :H + G]
    g = d["dy"].to(F64).view(M, H + 2 * G, HD)[:, :H + G]
    r = bwd_rstd(d).to(F64)[..., None]
    wg, xn = _weights(d) * g, x * r
    dot = (wg * xn).mean(-1, keepdim=True)
    dx = r * (wg - xn * dot)
    E_dot = (DEPTH + 4) * e * (wg * xn).abs().mean(-1, keepdim=True)
    A = r * (3 * e * wg.abs() + 4 * e * (xn * dot).abs() + xn.abs() * E_dot) + e * dx.abs()
    E = U * dx.abs() + (1 + U) * A
    normal(dx, "qk_norm_bwd")
    v = d["dy"].view(M, H + 2 * G, HD)[:, H + G:].reshape(M, -1).contiguous()
    return Ref({"qk": (dx.reshape(M, -1), E.reshape(M, -1))}, {"v": v})


def bwd_rstd(d):
    """the backward's rstd input: the float64 statistic rounded once to fp32"""
    M, H, G = d["M"], d["H"], d["G"]
    x = d["pre"].to(F64).view(M, H + 2 * G, HD)[:, :H + G]
    return (x.pow(2).mean(-1) + d["eps"]).rsqrt().to(F32)


def split(t, d):
    W = (d["H"] + d["G"]) * HD
    return {"qk": t[:, :W].contiguous(), "v": t[:, W:].contiguous()}


def weights(d, to):
    """the two [128] weights with NaN behind them"""
    return to(guarded_flat(d["wq"]))[:HD], to(guarded_flat(d["wk"]))[:HD]


def run_fwd(ops, d, to=None, alias=False, want_rstd=True, again=True):
    """out / rstd start as NaN with guard rows that must keep their bits; ``alias``: out == pre"""
    ops, to = _call(ops, to)
    M, H, G = d["M"], d["H"], d["G"]

    def once():
        pre = to(guarded_rows(d["pre"]))
        out = pre if alias else to(nan(M + GUARD, (H + 2 * G) * HD, dtype=BF))
        rstd = to(nan(M + GUARD, H + G)) if want_rstd else None
        ops.qk_norm_rope_fwd(pre[:M], *weights(d, to), to(guarded_rows(d["cos"]))[:M], to(guarded_rows(d["sin"]))[:M], out[:M],
                             None if rstd is None else rstd[:M], M, H, G, d["eps"])
        pre_b, out_b, rstd_b = _back(pre, out, rstd)
        assert untouched(out_b[M:]), "qk_norm_rope_fwd: rows past M of out were written"
        if not alias:
            same_bits(pre_b[:M], d["pre"], "qk_norm_rope_fwd: the input was changed")
        res = split(out_b[:M], d)
        if rstd_b is not None:
            assert untouched(rstd_b[M:]), "qk_norm_rope_fwd: rows past M of rstd were written"
            res["rstd"] = rstd_b[:M]
        return res

    return twice(once, "qk_norm_rope_fwd", again)


def run_bwd(ops, d, to=None, again=True):
    ops, to = _call(ops, to)
    M, H, G = d["M"], d["H"], d["G"]

    def once():
        dqkv, pre = to(guarded_rows(d["dy"])), to(guarded_rows(d["pre"]))
        ops.qk_norm_bwd(dqkv[:M], pre[:M], *weights(d, to), to(guarded_rows(bwd_rstd(d)))[:M], M, H, G)
        dq, pr = _back(dqkv, pre)
        assert untouched(dq[M:]), "qk_norm_bwd: rows past M of dqkv were written"
        same_bits(pr[:M], d["pre"], "qk_norm_bwd: pre was changed")
        return split(dq[:M], d)

    return twice(once, "qk_norm_bwd", again)


def append_positions(M, ctx, kind):
    return {"first": torch.zeros(M, dtype=I32), "last": torch.full((M,), ctx - 1, dtype=I32),
            "mixed": ((torch.arange(M) * 5 + 3) % ctx).to(I32)}[kind]


def run_append(ops, d, fwd_out, ctx, kind, to=None):
    """qkv in place and cache[row, pos[row]] against ``fwd_out`` (the forward kernel's qk | v on the same rows): the same bits;
    every other cell of the patterned caches, the guard rows of qkv and a guard cache row keep theirs"""
    ops, to = _call(ops, to)
    M, H, G = d["M"], d["H"], d["G"]
    W = G * HD
    slot = append_positions(M, ctx, kind)
    qkv = to(guarded_rows(d["pre"]))
    kc, vc = to(nan(M + 1, ctx, W, dtype=BF)), to(nan(M + 1, ctx, W, dtype=BF))
    ops.qk_norm_rope_append(qkv[:M], *weights(d, to), to(guarded_rows(d["cos"]))[:M], to(guarded_rows(d["sin"]))[:M], kc[:M], vc[:M],
                            to(slot), M, H, G, ctx, d["eps"])
    qkv, kc, vc = _back(qkv, kc, vc)
    assert untouched(qkv[M:]), "qk_norm_rope_append: rows past M of qkv were written"
    want = torch.cat([fwd_out["qk"], fwd_out["v"]], 1)
    same_bits(qkv[:M], want, "qk_norm_rope_append: qkv in place against the forward kernel")
    rows = torch.arange(M)
    same_bits(kc[rows, slot.long()], want[:, H * HD:H * HD + W].contiguous(), "qk_norm_rope_append: the appended key against the forward kernel")
    same_bits(vc[rows, slot.long()], want[:, H * HD + W:].contiguous(), "qk_norm_rope_append: the appended value against the projection")
    hit = torch.zeros(M + 1, ctx, dtype=torch.bool)
    hit[rows, slot.long()] = True
    assert untouched(kc[~hit]) and untouched(vc[~hit]), "qk_norm_rope_append: a cache cell other than [row, pos[row]] was written"
