"""TEST HELPER (not a test, never shipped): plain float64 restatements of what the LoRA recipe adds to the bf16 step -- the rank-sized
GEMMs (csrc/gemm_rank.hip), the fused low-rank accumulate, the dropout / scale / refresh kernels (csrc/lora.hip), the padded
transpose that feeds them (csrc/elementwise.hip) -- and of the fused AdamW update (adamw_kernel, csrc/misc.hip), on the exact
input values, each with the bound or the interval its result must lie in.  Nothing is shared with the kernels or with
tests/fake_ops.py (the dropout mask is oracle/lora_oracle.py's numpy restatement).  The checker, U = 2^-8 and RMS_RATIO = 1.5 are
those of tests/row_ref64.py; e = 2^-24 is the unit roundoff of fp32.  LIMIT = 1.0: every allowance is inside E.

ROUNDINGS.  fl32(x): one round-to-nearest-even from float64 (torch's double -> float conversion).  bf16r(x): one round-to-nearest-
even from float64 to bf16 by integer arithmetic on the double's bits (`double -> float -> bf16` would round twice).  A product of
an fp32 and a bf16 / fp32 value is exact in float64 (at most 48 bits), so fl32 of it IS the kernel's fp32 product; a sum of two
such values is exact in float64 while their exponents lie within 29 of each other (`exact_sum` asserts it).

RANK GEMMs  C = A B^T, N <= 64, K % 64 == 0: eight waves take the 64-wide chunks of K round-robin, each chunk is two MFMA steps
of 32 products, the eight partial tiles meet in LDS and are summed in wave order.
    exact profile   A integers in [-4, 4], B integers in [-4, 4] x 2^-3, 16 K < 2^24 (asserted): every partial sum is an integer
                    multiple of 2^-3 below 2^24 units, exact in fp32 in any order.  fp32 out: float64's bits; bf16 out: bf16r of it.
    N(0, 1) x 0.5   a term passes at most K additions (the MFMA's internal order is not specified; K covers any) and the sum of
                    eight partials: F = (K + 2) e sum |a b|.  fp32 out: |err| <= F;  bf16 out: |err| <= u |c| + F.  Second check:
                    rms(err / (u |c|)) over |c| >= 2^-6, where at least 4096 elements qualify, at most 1.5 x the double's.

LORA APPLY  v = bf16(sum_r u w), d = bf16(fl32(v s)), masked d = bf16(fl32(d keep)), y = bf16(fl32(y + d)), x_out = fl32(x_in + y):
one fp32 operation and one rounding per step, nothing for -ffp-contract to fuse.  `chain` restates everything after v bit for bit.
    exact profile   u integers in [-2, 2], W integers in [-1, 1] x 2^-2, R <= 128: |sum| <= 256 in units of 2^-2, v is exact.
                    y and x_out must have the reference's bits.
    N(0, 1)         F = (R + 2) e sum |u w|, v_lo = bf16r(sum - F), v_hi = bf16r(sum + F); s > 0 and keep >= 0, so every later
                    step is monotone non-decreasing in v: y in [chain(v_lo), chain(v_hi)], for a group with every member at its
                    v_lo / at its v_hi, in member order; where the ends agree, exactly that value.  x_out = fl32(x_in + y_got).
                    CAPS (on the reference alone): the share of elements whose ends differ is at most 5 % (R = 64, y = 0), 10 %
                    (R = 128, y = 0), 2 % (y ~ N(0, 1)), for a group launch as for one member.  A share is a statistic:
                    asserted where the case has at least 4096 elements, and on the pooled count of every class.  Operands 0.3 N(0, 1) at R = 64, 0.15 N(0, 1) at R = 128
                    (at 0.3 the share at R = 128, y ~ N(0, 1), s = 2 is 3.0 %: above its cap).
    mask            y = 0, u[:, 0] = W[:, 0] = 1, zeros elsewhere: v = 1, the result is bf16(bf16(s) keep): the bits of
                    tasu_lora_dropout on a bf16(s)-filled [M, N] matrix with the same (rng, sid) and of lora_keep_scale.

ELEMENTWISE  scale: bf16(fl32(x s)); dropout: bf16(fl32(x keep)); dropout_norm: bf16(fl32(fl32(g fl32(x rstd)) keep)): bits.
REFRESH  bf16(fl32(src scale)), plain or transposed: bits.   TRANSPOSE  the transpose's bits, zeros in the padding.

ADAMW  on the fp32 inputs with the constants the kernel is handed: beta, eps, wd, lr, grad_scale as fp32 values, c = 1 - beta from
the fp32 beta (exact: Sterbenz), isb1 = fl32(1 / bc1) and isb2 = fl32(1 / sqrt(bc2)) from the host's double (bc = 1 - beta^step
with the fp32 beta), k_lr = fl32(lr isb1), k_wd = fl32(1 - fl32(lr wd)) (the fused form fl32(1 - lr wd) is computed too: the cases
assert that the two agree, the decay-only profile accepts either).  g' = g grad_scale, m' = b1 m + c1 g', v' = b2 v + c2 g'^2,
den = sqrt(v') isb2 + eps, q = m' / den, p' = p k_wd - k_lr q.  Each bound holds with and without FMA contraction (a fused
operation drops one rounding of a term that is counted):
    E_m   = e (|b1 m| + 2 |c1 g'| + |m'|)                  the two products (g' carries its own rounding), the sum
    E_v   = e (|b2 v| + 4 |c2 g'^2| + |v'|)                g' twice, two products, the sum
    E_den = sqrt(v') isb2 (E_v / 2v' + 4 e) + e den        half the relative error of v', sqrtf and the product; 0 where v' = 0
    E_q   = E_m / den + |q| E_den / den + 3 e |q|          the division
    E_p   = e (|p k_wd| + 3 |k_lr q| + |p'|) + k_lr E_q
pb must have the bits of bf16(p_got).

The module also holds the case lists, the seeded inputs and the runs (NaN-filled outputs inside NaN-filled buffers, NaN in the
gaps of every operand's leading dimension) that tests/test_lora_ref64_cpu.py (through the torch double) and
tests/test_gpu_lora_f64.py (through HipOps) share."""
import collections
import math
import struct

import numpy as np
import torch

from oracle.lora_oracle import lora_keep_scale
from row_ref64 import BF, F32, F64, I32, LIMIT, NAN, RMS_RATIO, U, Ref, bits, cdiv, check, e, gen, nan, same_bits, untouched, worst_of  # noqa: F401

I64 = torch.int64


def case_id(c):
    return "-".join(str(v) for v in c)


# ================================================================================================ roundings
def fl32(x):
    """float64 -> the nearest fp32 value (ties to even), returned as float64"""
    return x.to(F32).to(F64)


def bf16r(x):
    """float64 -> the nearest bf16 value (ties to even) in ONE rounding, by integer arithmetic on the double's bits (the top 19
    bits -- sign, 11 exponent bits, 7 fraction bits -- are kept); returned as float64.  Zero or normal in bf16's range only."""
    x = x.contiguous()
    a = x.abs()
    assert bool(((a == 0) | ((a >= 2.0 ** -120) & (a < 2.0 ** 120))).all()), "bf16r: a value outside the normal range it handles"
    b = x.view(I64)
    b = (b + ((1 << 44) - 1) + ((b >> 45) & 1)) & ~((1 << 45) - 1)
    return b.view(F64)


def to_bf(x):
    """a float64 tensor of bf16 values as torch.bfloat16 (exact)"""
    return x.to(F32).to(BF)


def exact_sum(a, b):
    """a + b in float64, asserted exact (TwoSum's error term is zero everywhere)"""
    s = a + b
    bb = s - a
    assert bool((((a - (s - bb)) + (b - bb)) == 0).all()), "a float64 sum of the reference is not exact"
    return s


def f32c(x):
    """a Python float as the fp32 value a C `float` argument receives, in float64"""
    return float(np.float32(x))


# ================================================================================================ layouts
class Slab:
    """a [rows, cols] matrix inside a NaN-filled flat buffer: `lead` elements in front, leading dimension ld, first column col
    (col + cols may pass ld: the transposed store's ldc = M + 3); every cell outside the matrix holds NaN"""

    def __init__(self, x, ld, col=0, lead=0):
        self.rows, self.cols = x.shape
        self.ld, self.col, self.lead = ld, col, lead
        self.buf = nan(lead + col + self.rows * max(ld, self.cols) + 16, dtype=x.dtype)
        self.view(self.buf).copy_(x)

    def view(self, buf):
        return buf.as_strided((self.rows, self.cols), (self.ld, 1), self.lead + self.col)

    def outside_untouched(self, buf):
        b = buf.clone()
        self.view(b).fill_(NAN)
        return untouched(b)


def out_slab(rows, cols, ld, col=8, lead=0, dtype=F32):
    return Slab(nan(rows, cols, dtype=dtype), ld, col, lead)


def _call(ops, to):
    return ops, (to or (lambda t: t))


def _sync(*ts):
    if any(t is not None and t.is_cuda for t in ts):
        torch.cuda.synchronize()
    return [None if t is None else t.cpu() for t in ts]


# ================================================================================================ rank GEMMs
NtCase = collections.namedtuple("NtCase", "M N K profile lead")        # lead: elements in front of C's buffer (1: C off 16-byte alignment)
TnCase = collections.namedtuple("TnCase", "M N K profile")
GroupCase = collections.namedtuple("GroupCase", "M N members profile")
GROUP_K = (256, 64, 576, 128)
EXACT_SHIFT = 3


def _nt_cases():
    shapes = [(1, 8, 64), (15, 16, 448), (16, 24, 512), (17, 40, 576), (141, 48, 1536), (333, 64, 8960),     # the lists, paired
              (333, 8, 576), (17, 64, 64), (141, 64, 448), (16, 64, 512), (15, 64, 576), (1, 64, 8960), (333, 40, 1536), (141, 16, 8960)]
    out = [NtCase(M, N, K, p, 0) for M, N, K in shapes for p in ("exact", "n01")]
    out += [NtCase(17, 40, 576, p, 1) for p in ("exact", "n01")]
    return out


NT_CASES = _nt_cases()
TN_CASES = [TnCase(M, N, K, p) for M, N, K in [(64, 8, 64), (64, 16, 448), (192, 40, 512), (192, 64, 576), (1536, 64, 4096), (64, 64, 4096),
                                                (1536, 8, 576), (192, 16, 64), (64, 24, 448)] for p in ("exact", "n01")]   # (N = 24: ntn = 2)
GROUP_CASES = [GroupCase(M, N, n, p) for M, N in ((100, 40), (333, 64)) for n in (1, 2, 3, 4) for p in ("exact", "n01")]


def nt_chunks_per_wave(K):
    """how many 64-wide chunks waves 0..7 of rank_gemm_body take: c = wave, wave + 8, ... < K / 64"""
    return [len(range(w, K // 64, 8)) for w in range(8)]


def _operand(rows, K, profile, g, weight):
    if profile == "exact":
        x = torch.randint(-4, 5, (rows, K), generator=g).to(F32)
        return (x * 2.0 ** -EXACT_SHIFT if weight else x).to(BF)
    return (torch.randn(rows, K, generator=g) * 0.5).to(BF)


def nt_inputs(c):
    """A: a column slice at offset 64 of a [M, K + 72] matrix; B: [N, K] in rows of K + 8; NaN in every other cell"""
    M, N, K = c.M, c.N, c.K
    assert 16 * K < 2 ** 24
    g = gen(M, N, K, 101)
    a, b = _operand(M, K, c.profile, g, False), _operand(N, K, c.profile, g, True)
    return dict(M=M, N=N, K=K, profile=c.profile, a=a, b=b, A=Slab(a, K + 72, 64), B=Slab(b, K + 8), lead=getattr(c, "lead", 0))


def tn_inputs(c):
    """At: [K, M] K-major, a column slice at offset 64 of a [K, M + 128] matrix"""
    M, N, K = c.M, c.N, c.K
    assert 16 * K < 2 ** 24
    g = gen(M, N, K, 102)
    a, b = _operand(M, K, c.profile, g, False), _operand(N, K, c.profile, g, True)
    return dict(M=M, N=N, K=K, profile=c.profile, a=a, b=b, At=Slab(a.t().contiguous(), M + 128, 64), B=Slab(b, K + 8), lead=0)


def gemm_reference(d):
    """Ref of the fp32 output (`c`) and the bf16 output (`cb`) of one rank GEMM"""
    a, b = d["a"].to(F64), d["b"].to(F64)
    c = a @ b.t()
    if d["profile"] == "exact":
        return Ref({}, {"c": c.to(F32), "cb": to_bf(bf16r(c))})
    F = (d["K"] + 2) * e * (a.abs() @ b.abs().t())
    return Ref({"c": (c, F), "cb": (c, U * c.abs() + F)}, {})


def rms_u(got, want):
    """rms(err / (u |c|)) over |c| >= 2^-6; (rms, count)"""
    keep = want.abs() >= 2.0 ** -6
    n = int(keep.sum())
    if n == 0:
        return 0.0, 0
    return float((((got.to(F64) - want).abs() / (U * want.abs()))[keep]).pow(2).mean().sqrt()), n


def _c_slab(M, N, f32, transposed, lead):
    dt = F32 if f32 else BF
    return out_slab(N, M, M + 3, 8, lead, dt) if transposed else out_slab(M, N, N + 24, 8, lead, dt)


def _twice(run):
    first = run()
    second = run()
    for k in first:
        same_bits(second[k], first[k], f"second run, {k}")
    return first


def run_nt(ops, d, to=None):
    """{(f32, transposed): C [M, N]} of the four stores of tasu_gemm_nt_rank, each run twice (equal bits), sentinels checked"""
    ops, to = _call(ops, to)
    M, N, K = d["M"], d["N"], d["K"]
    a, b = d["A"].view(to(d["A"].buf)), d["B"].view(to(d["B"].buf))

    def once():
        out = {}
        for f32 in (True, False):
            for tr in (False, True):
                s = _c_slab(M, N, f32, tr, d["lead"])
                buf = to(s.buf)
                ops.gemm_rank(a, b, s.view(buf), M, N, K, f32=f32, transposed=tr)
                (buf,) = _sync(buf)
                assert s.outside_untouched(buf), f"gemm_rank f32={f32} transposed={tr}: a cell outside C was written"
                got = s.view(buf)
                out[("c" if f32 else "cb") + ("_t" if tr else "")] = (got.t() if tr else got).contiguous()
        return out
    return _twice(once)


def run_tn(ops, d, to=None):
    ops, to = _call(ops, to)
    M, N, K = d["M"], d["N"], d["K"]
    at, b = d["At"].view(to(d["At"].buf)), d["B"].view(to(d["B"].buf))

    def once():
        out = {}
        for tr in (False, True):
            s = _c_slab(M, N, True, tr, 0)
            buf = to(s.buf)
            ops.gemm_rank_tn(at, b, s.view(buf), M, N, K, transposed=tr)
            (buf,) = _sync(buf)
            assert s.outside_untouched(buf), f"gemm_rank_tn transposed={tr}: a cell outside C was written"
            got = s.view(buf)
            out["c_t" if tr else "c"] = (got.t() if tr else got).contiguous()
        return out
    return _twice(once)


def gemm_rank_group(ops, As, Bs, Cs, M, N, Ks):
    """the group launch; an operator set without it (the torch double) runs the members"""
    if hasattr(ops, "gemm_rank_group"):
        return ops.gemm_rank_group(As, Bs, Cs, M, N, Ks)
    for a, b, c, K in zip(As, Bs, Cs, Ks):
        ops.gemm_rank(a, b, c, M, N, K)


def group_inputs(c):
    members = []
    for t in range(c.members):
        g, K = gen(c.M, c.N, t, 103), GROUP_K[t]                   # every member its own operands, K and lda
        a, b = _operand(c.M, K, c.profile, g, False), _operand(c.N, K, c.profile, g, True)
        members.append(dict(M=c.M, N=c.N, K=K, profile=c.profile, a=a, b=b, A=Slab(a, K + 72, 64), B=Slab(b, K + 8)))
    return dict(M=c.M, N=c.N, members=members)


def run_group(ops, d, to=None):
    """[C_t [M, N] bf16] of tasu_gemm_nt_rank_group: the members' outputs are column blocks of one NaN-filled [M, ldc] buffer"""
    ops, to = _call(ops, to)
    M, N, ms = d["M"], d["N"], d["members"]
    n = len(ms)
    ldc = n * (N + 8) + 16

    def once():
        buf = to(nan(M * ldc + 16, dtype=BF))
        Cs = [buf.as_strided((M, N), (ldc, 1), 8 + t * (N + 8)) for t in range(n)]
        gemm_rank_group(ops, [m["A"].view(to(m["A"].buf)) for m in ms], [m["B"].view(to(m["B"].buf)) for m in ms], Cs, M, N, [m["K"] for m in ms])
        (buf,) = _sync(buf)
        out = {}
        chk = buf.clone()
        for t in range(n):
            v = buf.as_strided((M, N), (ldc, 1), 8 + t * (N + 8))
            out[f"cb{t}"] = v.contiguous()
            chk.as_strided((M, N), (ldc, 1), 8 + t * (N + 8)).fill_(NAN)
        assert untouched(chk), "gemm_rank_group: a cell outside the members' blocks was written"
        return out
    return _twice(once)


# ================================================================================================ lora_apply
ApplyCase = collections.namedtuple("ApplyCase", "M N R members")       # members 0: tasu_lora_apply; 1..4: tasu_lora_apply_group
APPLY_CASES = [ApplyCase(M, N, R, 0) for M, N, R in [(1, 8, 64), (63, 248, 64), (64, 256, 128), (65, 264, 64), (141, 520, 64), (333, 1536, 64),
                                                      (333, 8, 128), (1, 1536, 64), (64, 128, 128), (70, 264, 64), (141, 256, 64), (333, 512, 64)]]
APPLY_CASES += [ApplyCase(M, N, 64, n) for M, N, n in [(65, 264, 1), (141, 520, 2), (333, 248, 3), (64, 1536, 4), (1, 8, 3), (333, 512, 2)]]
SCALES, DROPS = (1.0, 0.25, 2.0, 0.3), (0.0, 0.05, 0.25)
EXACT_SETTINGS = [(s, p, r) for s in SCALES for p in DROPS for r in (False, True)]
N01_SETTINGS = [(1.0, 0.0, False), (0.25, 0.05, True), (0.3, 0.25, False), (2.0, 0.05, True)]
RNG = (987654321, 3)
CAP_MIN = 4096


def sids_of(c):
    return [5 + 8 * t for t in range(max(c.members, 1))]


def share_cap(R, y_zero):
    return 0.02 if not y_zero else (0.05 if R == 64 else 0.10)


def apply_inputs(c, profile, y_zero=False):
    """u_t: column slices at offset 64 of [M, R + 72]; W_t: [N, R] in rows of R + 8; y: columns 8.. of [M, N + 16]; x_in / x_out:
    columns 4.. of [M, N + 8] (fp32); NaN in every gap"""
    M, N, R = c.M, c.N, c.R
    us, ws = [], []
    for t in range(max(c.members, 1)):
        g = gen(M, N, R, t, 111)
        if profile == "exact":
            u = torch.randint(-2, 3, (M, R), generator=g).to(BF)
            w = (torch.randint(-1, 2, (N, R), generator=g).to(F32) * 0.25).to(BF)
        elif profile == "mask":
            u, w = torch.zeros(M, R, dtype=BF), torch.zeros(N, R, dtype=BF)
            u[:, 0] = 1
            w[:, 0] = 1
        else:                                                      # 0.3 N(0, 1) at R = 64, 0.15 at R = 128: the scales at which the caps hold
            sc = 0.3 if R == 64 else 0.15
            u, w = (torch.randn(M, R, generator=g) * sc).to(BF), (torch.randn(N, R, generator=g) * sc).to(BF)
        us.append(u)
        ws.append(w)
    g = gen(M, N, R, 112)
    y = torch.zeros(M, N, dtype=BF) if (y_zero or profile == "mask") else torch.randn(M, N, generator=g).to(BF)
    x_in = torch.randn(M, N, generator=g)
    return dict(M=M, N=N, R=R, members=c.members, sids=sids_of(c), us=us, ws=ws, y=y, x_in=x_in, rng=torch.tensor(RNG, dtype=I64),
                U=[Slab(u, R + 72, 64) for u in us], W=[Slab(w, R + 8) for w in ws], Y=Slab(y, N + 16, 8), X=Slab(x_in, N + 8, 4))


def keep_of(d, t, p):
    return None if p == 0.0 else lora_keep_scale(RNG, d["sids"][t], (d["M"], d["N"]), p).to(F64)


def chain(v, y, s, keep):
    """one member's accumulate after v, in float64 with every rounding explicit: y' = bf16(fl32(y + [bf16(fl32(. keep))] bf16(fl32(v s))))"""
    dlt = bf16r(fl32(v * f32c(s)))
    if keep is not None:
        dlt = bf16r(fl32(dlt * keep))
    return bf16r(fl32(exact_sum(y, dlt)))


def apply_reference(d, s, p, exact):
    """exact profile: (y, y) with y the one result; else (y_lo, y_hi), every member at v_lo / at v_hi in member order"""
    assert s > 0
    lo = hi = d["y"].to(F64)
    for t, (u, w) in enumerate(zip(d["us"], d["ws"])):
        u, w = u.to(F64), w.to(F64)
        acc = u @ w.t()
        keep = keep_of(d, t, p)
        if exact:
            assert float(acc.abs().max()) <= 256
            lo = hi = chain(bf16r(acc), lo, s, keep)
        else:
            F = (d["R"] + 2) * e * (u.abs() @ w.abs().t())
            lo, hi = chain(bf16r(acc - F), lo, s, keep), chain(bf16r(acc + F), hi, s, keep)
    assert bool((lo <= hi).all())
    return lo, hi


def lora_apply_group(ops, y, us, ws, M, N, R, sids, s, p, rng):
    if hasattr(ops, "lora_apply_group"):
        return ops.lora_apply_group(y, us, ws, M, N, R, sids, s=s, p=p, rng=rng)
    for u, w, sid in zip(us, ws, sids):
        ops.lora_apply(y, u, w, M, N, R, s=s, p=p, rng=rng, sid=sid)


def run_apply(ops, d, s, p, resid, to=None):
    """(y [M, N] bf16, x_out [M, N] fp32 or None) of one tasu_lora_apply / _group; the columns around y and x_out keep their NaN"""
    ops, to = _call(ops, to)
    M, N, R = d["M"], d["N"], d["R"]
    ybuf = to(d["Y"].buf.clone())
    us, ws = [S.view(to(S.buf)) for S in d["U"]], [S.view(to(S.buf)) for S in d["W"]]
    rng = to(d["rng"]) if p > 0 else None
    xo, xbuf, xobuf = None, None, None
    if d["members"]:
        assert not resid
        lora_apply_group(ops, d["Y"].view(ybuf), us, ws, M, N, R, d["sids"], s, p, rng)
    else:
        if resid:
            xo = out_slab(M, N, N + 8, 4)
            xbuf, xobuf = to(d["X"].buf), to(xo.buf)
        ops.lora_apply(d["Y"].view(ybuf), us[0], ws[0], M, N, R, s=s, p=p, rng=rng, sid=d["sids"][0],
                       x_in=d["X"].view(xbuf) if resid else None, x_out=xo.view(xobuf) if resid else None)
    ybuf, xobuf = _sync(ybuf, xobuf)
    assert d["Y"].outside_untouched(ybuf), "lora_apply: a cell outside y[M, N] was written"
    if resid:
        assert xo.outside_untouched(xobuf), "lora_apply: a cell outside x_out[M, N] was written"
    return d["Y"].view(ybuf).contiguous(), xo.view(xobuf).contiguous() if resid else None


def check_apply(got_y, got_x, d, ref, resid, what):
    """y inside [lo, hi] (equal ends: that value), x_out = fl32(x_in + y_got) exactly; raises, naming the first element outside"""
    lo, hi = ref
    g = got_y.to(F64)
    bad = ~((g >= lo) & (g <= hi))
    if bool(bad.any()):
        i = tuple(torch.nonzero(bad)[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {g.numel()} elements of y outside [chain(v_lo), chain(v_hi)], first at {i}: got "
                             f"{float(g[i])!r}, interval [{float(lo[i])!r}, {float(hi[i])!r}]")
    if resid:
        same_bits(got_x, exact_sum(d["x_in"].to(F64), g).to(F32), f"{what} x_out against fl32(x_in + y_got)")


# ================================================================================================ elementwise, refresh, transpose
ElemCase = collections.namedtuple("ElemCase", "M D")
ELEM_CASES = [ElemCase(M, D) for D in (4, 256, 1536) for M in (1, 37)] + [ElemCase(1100, 4096)]
ELEM_BIG8 = ElemCase(2100, 4096)          # more than 4096 x 256 vectors of EIGHT: the grid-stride loop of the bf16x8 kernels


def elem_inputs(c):
    g = gen(c.M, c.D, 121)
    x = torch.randn(c.M, c.D, generator=g)
    return dict(M=c.M, D=c.D, x=x, xb=x.to(BF), w=1 + 0.1 * torch.randn(c.D, generator=g),
                rstd=torch.rsqrt(x.to(F64).pow(2).mean(-1) + 1e-6).to(F32), rng=torch.tensor(RNG, dtype=I64))


def scale_reference(d, s):
    return to_bf(bf16r(fl32(d["xb"].to(F64) * f32c(s))))


def dropout_reference(d, p, sid):
    return to_bf(bf16r(fl32(d["xb"].to(F64) * lora_keep_scale(RNG, sid, (d["M"], d["D"]), p).to(F64))))


def dropout_norm_reference(d, p, sid):
    t = fl32(d["w"].to(F64) * fl32(d["x"].to(F64) * d["rstd"].to(F64)[:, None]))
    return to_bf(bf16r(fl32(t * lora_keep_scale(RNG, sid, (d["M"], d["D"]), p).to(F64))))


def _guarded(n, dtype, to):
    return to(nan(n + 16, dtype=dtype))


def run_scale(ops, d, s, to=None):
    ops, to = _call(ops, to)
    n = d["M"] * d["D"]
    dst = _guarded(n, BF, to)
    ops.scale_bf16(to(d["xb"].reshape(-1)), dst[:n], s)
    (dst,) = _sync(dst)
    assert untouched(dst[n:]), "scale_bf16: wrote past n"
    return dst[:n].view(d["M"], d["D"])


def run_dropout(ops, d, p, sid, to=None):
    """source: a column slice of a wider NaN-padded matrix; destination rows of D + 8"""
    ops, to = _call(ops, to)
    M, D = d["M"], d["D"]
    src, dst = Slab(d["xb"], D + 16, 8), out_slab(M, D, D + 8, 0, 0, BF)
    buf = to(dst.buf)
    ops.lora_dropout(src.view(to(src.buf)), dst.view(buf), p, to(d["rng"]), sid)
    (buf,) = _sync(buf)
    assert dst.outside_untouched(buf), "lora_dropout: a cell outside dst[M, C] was written"
    return dst.view(buf).contiguous()


def lora_dropout_norm_group(ops, x, w, rstd, dsts, M, D, p, rng, sids):
    if hasattr(ops, "lora_dropout_norm_group"):
        return ops.lora_dropout_norm_group(x, w, rstd, dsts, M, D, p, rng, sids)
    for dst, sid in zip(dsts, sids):
        ops.lora_dropout_norm(x, w, rstd, dst, M, D, p, rng, sid)


def run_dropout_norm(ops, d, p, sids, group, to=None):
    ops, to = _call(ops, to)
    M, D = d["M"], d["D"]
    n = M * D
    dsts = [_guarded(n, BF, to) for _ in sids]
    args = [to(d["x"]), to(d["w"]), to(d["rstd"])]
    if group:
        lora_dropout_norm_group(ops, *args, [t[:n].view(M, D) for t in dsts], M, D, p, to(d["rng"]), sids)
    else:
        ops.lora_dropout_norm(*args, dsts[0][:n].view(M, D), M, D, p, to(d["rng"]), sids[0])
    dsts = _sync(*dsts)
    assert all(untouched(t[n:]) for t in dsts), "lora_dropout_norm: wrote past M x D"
    return [t[:n].view(M, D) for t in dsts]


REFRESH_ENTRIES = [(16, 264, 0, 0.25), (16, 264, 1, 0.3), (64, 1536, 0, 0.3), (64, 1536, 1, 0.25)]      # rows, cols, transpose, scale


def refresh_inputs():
    g = gen(131)
    srcs = [torch.randn(r, c, generator=g).to(BF) for r, c, _, _ in REFRESH_ENTRIES]
    offs, pb = [], [nan(8, dtype=BF)]
    for sr in srcs:                                                # the entries' sources lie in one image, NaN between them
        offs.append(sum(t.numel() for t in pb))
        pb += [sr.reshape(-1), nan(8, dtype=BF)]
    return dict(srcs=srcs, offs=offs, pb=torch.cat(pb))


def refresh_reference(d):
    out = []
    for sr, (r, c, tr, sc) in zip(d["srcs"], REFRESH_ENTRIES):
        v = to_bf(bf16r(fl32(sr.to(F64) * f32c(sc))))
        out.append(v.t().contiguous() if tr else v)
    return out


def run_refresh(ops, d, to=None):
    """every destination inside its own NaN-filled buffer (rows of its width + 24, first column 8); an operator set without the
    one-launch kernel builds the copies with scale_bf16 and transpose, as LoraParams.refresh_working_copies does"""
    ops, to = _call(ops, to)
    pb = to(d["pb"])
    slabs = [out_slab(c if tr else r, r if tr else c, (r if tr else c) + 24, 8, 0, BF) for r, c, tr, _ in REFRESH_ENTRIES]
    bufs = [to(s.buf) for s in slabs]
    if hasattr(ops, "lora_refresh"):
        rows, tiles = [], 0
        for s, buf, off, (r, c, tr, sc) in zip(slabs, bufs, d["offs"], REFRESH_ENTRIES):
            rows.append([off, s.view(buf).data_ptr(), r, c, s.ld, tr, struct.unpack("<i", struct.pack("<f", sc))[0], tiles])
            tiles += cdiv(r, 64) * cdiv(c, 64)
        ops.lora_refresh(pb, to(torch.tensor(rows, dtype=I64)), len(rows), tiles)
    else:
        for s, buf, off, (r, c, tr, sc) in zip(slabs, bufs, d["offs"], REFRESH_ENTRIES):
            src = pb[off:off + r * c].view(r, c)
            tmp = torch.empty_like(src)
            ops.scale_bf16(src, tmp, sc)
            if tr:
                ops.transpose(tmp, s.view(buf), r, c, r, c)
            else:
                s.view(buf).copy_(tmp)
    bufs = _sync(*bufs)
    assert all(s.outside_untouched(b) for s, b in zip(slabs, bufs)), "lora_refresh: a cell outside a destination was written"
    return [s.view(b).contiguous() for s, b in zip(slabs, bufs)]


TrCase = collections.namedtuple("TrCase", "R C Rpad Cpad ld_in ld_out")
TR_CASES = [TrCase(16, 264, 64, 264, 264, 72), TrCase(141, 192, 192, 192, 200, 200), TrCase(128, 128, 128, 128, 128, 128),
            TrCase(128, 128, 128, 128, 131, 131)]                  # the last two: the 16-byte vector path / odd rows: the scalar path


def run_transpose(ops, c, to=None):
    """(got [Cpad, Rpad], src [R, C]): the destination inside a NaN-filled buffer (rows of ld_out, 16 elements behind the last)"""
    ops, to = _call(ops, to)
    src = torch.randn(c.R, c.C, generator=gen(c.R, c.C, c.ld_in, 141)).to(BF)
    S = Slab(src, c.ld_in)
    dst = Slab(nan(c.Cpad, c.Rpad, dtype=BF), c.ld_out)
    buf = to(dst.buf)
    ops.transpose(S.view(to(S.buf)), dst.view(buf), c.R, c.C, c.Rpad, c.Cpad)
    (buf,) = _sync(buf)
    assert dst.outside_untouched(buf), "transpose: a cell outside [Cpad, Rpad] was written"
    return dst.view(buf).contiguous(), src


# ================================================================================================ AdamW
AdamCase = collections.namedtuple("AdamCase", "profile n step wd gscale pb")
LR, BETA1, BETA2, EPS = 5e-5, 0.9, 0.999, 1e-6
ADAM_BIG = 4096 * 1024 + 4
ADAM_PROFILES = ("n01", "p0", "first", "decay", "v0")


def _adam_cases():
    out, k = [], 0
    for profile in ADAM_PROFILES:
        for step in (1, 3, 100000):
            for wd in (0.0, 0.01, 0.1):
                for gs in (1.0, 0.125):
                    out.append(AdamCase(profile, 4160, step, wd, gs, k % 2))
                    k += 1
    out += [AdamCase(p, 4, 3, 0.01, 0.125, 1) for p in ADAM_PROFILES]
    out += [AdamCase("n01", ADAM_BIG, 3, 0.01, 0.125, 1)]
    return out


ADAM_CASES = _adam_cases()


def adam_inputs(c):
    n = c.n
    g = gen(n, 151)
    p, gr = torch.randn(n, generator=g), torch.randn(n, generator=g)
    m, v = torch.randn(n, generator=g).abs() * 0.1, torch.randn(n, generator=g).abs() * 0.01      # the state of test_posterior_merge_adamw
    if c.profile == "p0":
        p = torch.zeros(n)
    elif c.profile == "first":
        m, v, gr = torch.zeros(n), torch.zeros(n), gr * 1e-3
    elif c.profile == "decay":
        gr, m, v = torch.zeros(n), torch.zeros(n), torch.zeros(n)
    elif c.profile == "v0":
        gr, v, m = torch.zeros(n), torch.zeros(n), torch.randn(n, generator=g) * 0.1
    return dict(n=n, p=p, g=gr, m=m, v=v, step=c.step, wd=c.wd, gscale=c.gscale, pb=c.pb, profile=c.profile)


def adam_constants(step, wd, kernel=True):
    """the constants of one update: as the kernel is handed / forms them (fp32), or (kernel=False) the same expressions in float64"""
    b1, b2, eps, lr, wd = f32c(BETA1), f32c(BETA2), f32c(EPS), f32c(LR), f32c(wd)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    r = (lambda x: float(np.float32(x))) if kernel else (lambda x: x)
    isb1, isb2 = r(1.0 / bc1), r(1.0 / math.sqrt(bc2))
    return dict(b1=b1, b2=b2, c1=1.0 - b1, c2=1.0 - b2, eps=eps, isb2=isb2, k_lr=r(lr * isb1), k_wd=r(1.0 - r(lr * wd)), k_wd_fused=r(1.0 - lr * wd))


def adam_reference(d, kernel=True):
    k = adam_constants(d["step"], d["wd"], kernel)
    p, g, m, v = (d[n].to(F64) for n in "pgmv")
    g1 = g * f32c(d["gscale"])
    m1 = k["b1"] * m + k["c1"] * g1
    v1 = k["b2"] * v + k["c2"] * g1 * g1
    den = v1.sqrt() * k["isb2"] + k["eps"]
    q = m1 / den
    p1 = p * k["k_wd"] - k["k_lr"] * q
    E_m = e * ((k["b1"] * m).abs() + 2 * (k["c1"] * g1).abs() + m1.abs())
    E_v = e * ((k["b2"] * v).abs() + 4 * (k["c2"] * g1 * g1).abs() + v1.abs())
    pos = v1 > 0
    E_den = torch.where(pos, v1.sqrt() * k["isb2"] * (E_v / (2 * torch.where(pos, v1, torch.ones_like(v1))) + 4 * e) + e * den, torch.zeros_like(v1))
    E_q = E_m / den + q.abs() * E_den / den + 3 * e * q.abs()
    E_p = e * ((p * k["k_wd"]).abs() + 3 * (k["k_lr"] * q).abs() + p1.abs()) + k["k_lr"] * E_q
    row = lambda t: t[None]
    tol = {"m": (row(m1), row(E_m)), "v": (row(v1), row(E_v)), "p": (row(p1), row(E_p))}
    if d["profile"] == "decay":                                   # p' = fl32(p k_wd), nothing else: the bits, for one of the two k_wd
        tol.pop("p")
    return Ref(tol, {}), k


def check_decay(got_p, d, k, what):
    p = d["p"].to(F64)
    a, b = (p * k["k_wd"]).to(F32), (p * k["k_wd_fused"]).to(F32)
    assert torch.equal(bits(got_p), bits(a)) or torch.equal(bits(got_p), bits(b)), f"{what}: p' is not fl32(p k_wd) for either form of k_wd"


ADAM_GUARD = 8


def run_adam(ops, d, to=None):
    ops, to = _call(ops, to)
    n = d["n"]
    bufs = {}
    for name in "pgmv":
        t = nan(n + ADAM_GUARD)
        t[:n] = d[name]
        bufs[name] = to(t)
    pb = to(nan(n + ADAM_GUARD, dtype=BF)) if d["pb"] else None
    ops.adamw(bufs["p"][:n], bufs["g"][:n], bufs["m"][:n], bufs["v"][:n], None if pb is None else pb[:n], LR, BETA1, BETA2, EPS, d["wd"],
              d["step"], d["gscale"])
    p, g, m, v, pb = _sync(bufs["p"], bufs["g"], bufs["m"], bufs["v"], pb)
    assert all(untouched(t[n:]) for t in (p, m, v)) and (pb is None or untouched(pb[n:])), "adamw: wrote past n"
    same_bits(g[:n], d["g"], "adamw: the gradient")
    out = {"p": p[None, :n], "m": m[None, :n], "v": v[None, :n]}
    if pb is not None:
        same_bits(pb[:n], p[:n].to(BF), "adamw: pb against bf16(p_got)")
    return out
