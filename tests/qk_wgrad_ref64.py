"""TEST HELPER (not a test, never shipped): plain float64 restatement of the q_norm / k_norm weight-gradient kernels --
tasu_qk_norm_wgrad and tasu_f32_qk_norm_wgrad (csrc/qk_norm.hip) -- on the exact input values, with a bound E for every element.
Nothing is shared with the kernels or with tests/qwen3_full_ft_ops.py.  `nan`, `untouched`, `same_bits`, `gen` and e = 2^-24 are
those of tests/row_ref64.py, `twice` that of tests/point_ref64.py.

    dwq[d] = (prev[d] +) sum over rows m and q heads h of g[m, h, d] xn[m, h, d];   dwk: the same over the k heads
    g = dqkv (the gradient of w * xn), rstd an fp32 INPUT (the same values go to the kernel and to the reference).

    bf16 family   xn = bf16(fl32(pre r)).  pre is bf16 and r fp32, so pre r is exact in float64 and its rounding to fp32 and then
                  to bf16 IS the kernel's operand; g xn is a product of two bf16 values, exact in fp32.  All the kernel can add
                  is the rounding of its N - 1 fp32 additions (N = rows x heads summed into the element), each at most e times a
                  partial sum, every partial sum at most sum |g xn| to first order, in ANY order:
                      E = (N - 1) e sum |g xn|.
    fp32 family   xn = pre r and g xn: two rounded products per term, e each, relative to the term:
                      E = (N + 2 - 1) e sum |g xn|.
    accumulate    the previous value is one more term of the sum: N + 1 terms, |prev| joins the sum of magnitudes.
    A term count of 1 in the bf16 family gives E = 0: the single exact product must arrive as it is.

    exact profile   integer pre and g in [-4, 4] and r in {1/4, 1/2, 1, 2}: xn and every product are multiples of 1/4 below 2^5,
                    every partial sum of at most 700 x 16 of them stays below 2^24 quarters -- fp32 adds them without rounding in
                    any order, so the result must EQUAL the float64 sum (compared as values: a sum of zeros may carry either sign).
    general profile N(0, 1) pre, 0.25 N(0, 1) g, r = the float64 statistic of pre rounded once to fp32.

The v block of dqkv and pre is NaN in every run: it must never be read.  dwq, dwk and ws sit between NaN guards; without
accumulate they start as NaN themselves (the kernel must overwrite, not add).  The module holds the cases, the inputs and the run
that tests/test_qk_wgrad_ref64_cpu.py (the torch double) and tests/test_gpu_qk_wgrad_f64.py (HipOps) share."""
import collections

import torch

from point_ref64 import twice
from row_ref64 import NAN, e, gen, nan, same_bits, untouched  # noqa: F401

HD = 128
EPS = 1e-6
SPLIT = 512                                                      # TASU_QK_WGRAD_SPLIT
WS_FLOATS = SPLIT * 2 * HD
GUARD = 8                                                        # floats in front of and behind dwq / dwk / ws (32 bytes: alignment kept)
F32, F64, BF = torch.float32, torch.float64, torch.bfloat16

Case = collections.namedtuple("Case", "M H G")
# the smallest that can go wrong: one row, an odd count, one past a 64-row chunk, and 300 rows -- with (16, 8) 7200 units, a ragged
# share per workgroup; (700, 16, 8): 16800 units, so that every 16-lane group of the bf16 kernel (512 x 16 per sweep) and every
# 32-lane group of the fp32 kernel (512 x 8) walks more than one unit and the last sweep is ragged
CASES = [Case(M, H, G) for M in (1, 5, 67, 300) for H, G in ((2, 1), (4, 4), (16, 8))] + [Case(700, 16, 8)]
FAMILIES = ("bf16", "f32")


def case_id(c):
    return "-".join(str(v) for v in c)


def inputs(c, family, profile):
    """dqkv / pre [M, (H+2G)*128] in the family's dtype with a NaN v block, rstd [M, H+G] fp32, prev [2, 128] fp32"""
    M, H, G = c
    NH, NQK = H + 2 * G, H + G
    g = gen(M, H, G, 23, family == "f32", profile == "exact")
    dt = BF if family == "bf16" else F32
    if profile == "exact":
        pre = torch.randint(-4, 5, (M, NH, HD), generator=g).to(F32)
        dy = torch.randint(-4, 5, (M, NH, HD), generator=g).to(F32)
        rstd = torch.exp2(torch.randint(-2, 2, (M, NQK), generator=g).to(F32))
        prev = torch.randint(-64, 65, (2, HD), generator=g).to(F32) * 0.25
    else:
        pre = torch.randn(M, NH, HD, generator=g).to(dt).to(F32)
        dy = (0.25 * torch.randn(M, NH, HD, generator=g)).to(dt).to(F32)
        rstd = (pre[:, :NQK].to(F64).pow(2).mean(-1) + EPS).rsqrt().to(F32)
        prev = torch.randn(2, HD, generator=g)
    pre[:, NQK:] = NAN
    dy[:, NQK:] = NAN
    return dict(pre=pre.to(dt).view(M, NH * HD), dy=dy.to(dt).view(M, NH * HD), rstd=rstd, prev=prev, M=M, H=H, G=G, family=family,
                profile=profile)


def reference(d, accumulate):
    """(dw [2, 128] float64, E [2, 128]): row 0 = dwq, row 1 = dwk"""
    M, H, G = d["M"], d["H"], d["G"]
    NQK = H + G
    x = d["pre"].view(M, H + 2 * G, HD)[:, :NQK].to(F64)
    g = d["dy"].view(M, H + 2 * G, HD)[:, :NQK].to(F64)
    t = x * d["rstd"].to(F64)[..., None]
    xn = t.to(F32).to(BF).to(F64) if d["family"] == "bf16" else t
    p = g * xn
    assert bool(torch.isfinite(p).all())
    dw = torch.stack([p[:, :H].sum((0, 1)), p[:, H:].sum((0, 1))])
    mag = torch.stack([p[:, :H].abs().sum((0, 1)), p[:, H:].abs().sum((0, 1))])
    n = torch.tensor([M * H, M * G], dtype=F64)[:, None]
    if accumulate:
        dw, mag, n = dw + d["prev"].to(F64), mag + d["prev"].to(F64).abs(), n + 1
    extra = 2 if d["family"] == "f32" else 0
    return dw, (n + extra - 1) * e * mag


def guarded(t, fill_nan=False):
    """a flat fp32 buffer [GUARD | t | GUARD] with NaN guards (fill_nan: NaN in place of t's values too)"""
    side = torch.full((GUARD,), NAN)
    return torch.cat([side, torch.full((t.numel(),), NAN) if fill_nan else t.reshape(-1).to(F32), side])


def run(ops, d, accumulate, to=None, again=True):
    """one call through ``ops`` (HipOps or the torch double; ``to`` moves a tensor to where it computes): dw [2, 128] fp32"""
    to = to or (lambda t: t)
    M, H, G = d["M"], d["H"], d["G"]
    op = ops.qk_norm_wgrad if d["family"] == "bf16" else ops.f32_qk_norm_wgrad
    rows = lambda t: torch.cat([t, torch.full((3, t.shape[1]), NAN, dtype=t.dtype)])      # noqa: E731  (NaN rows behind every operand)

    def once():
        dq, pr, rs = to(rows(d["dy"])), to(rows(d["pre"])), to(rows(d["rstd"]))
        bq, bk = to(guarded(d["prev"][0], not accumulate)), to(guarded(d["prev"][1], not accumulate))
        ws = to(guarded(torch.zeros(WS_FLOATS), True))
        op(dq[:M], pr[:M], rs[:M], bq[GUARD:GUARD + HD], bk[GUARD:GUARD + HD], ws[GUARD:GUARD + WS_FLOATS], M, H, G, accumulate=accumulate)
        if dq.is_cuda:
            torch.cuda.synchronize()
        dq, pr, bq, bk, ws = (t.cpu() for t in (dq, pr, bq, bk, ws))
        same_bits(dq[:M], d["dy"], "qk_norm_wgrad: dqkv was changed")
        same_bits(pr[:M], d["pre"], "qk_norm_wgrad: pre was changed")
        for name, b, n in (("dwq", bq, HD), ("dwk", bk, HD), ("ws", ws, WS_FLOATS)):
            assert untouched(b[:GUARD]) and untouched(b[GUARD + n:]), f"qk_norm_wgrad: the guards around {name} were written"
        return {"dw": torch.stack([bq[GUARD:GUARD + HD], bk[GUARD:GUARD + HD]])}

    return twice(once, "qk_norm_wgrad", again)["dw"]


def ratio(got, ref):
    """the largest |got - ref| / E over the elements (E = 0: 0 where equal, inf where not; NaN: inf)"""
    want, E = ref
    err = (got.to(F64) - want).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / E)
    return float(torch.nan_to_num(r, nan=float("inf")).max())


def exact(got, ref):
    """the float64 sum's value in fp32, element for element"""
    return torch.equal(got, ref[0].to(F32)) and bool((ref[0].to(F32).to(F64) == ref[0]).all())
