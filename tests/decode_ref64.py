"""TEST HELPER (not a test, never shipped): plain float64 restatements of the bf16 decode-step operators -- the cache attention
(csrc/attn_decode_body.h) and the M <= 64 weight-streaming GEMMs with their epilogues (csrc/gemm_skinny.hip, csrc/gemm_stream.hip /
stream_body.h) -- on the exact bf16 input values, each with a bound E for every element it returns.  Nothing is shared with the
kernels or with tests/fake_ops.py.  u = 2^-8 is the unit roundoff of bf16 under round-to-nearest-even; `check_within` /
`assert_within` are those of tests/attn_ref64.py.

(a) CACHE ATTENTION.  Row r sees the keys at positions [kstart[r], lens[r]) of physical cache row index[r, pos] (its own row when
index is None).  With s_j = scale q.k_j, p_j = exp(s_j - max s), l = sum p_j, P = p / l, the kernel's rounding points are: scores
and exp in fp32; the UNNORMALISED p_j rounded to bf16 before P.V; l summed from the unrounded p; one bf16 rounding of the output:

    o = P v              E = u (P|v| + |o|)  +  sum_j P_j e_j |v_j|  +  |o| sum_j P_j e_j
    e_j = 2^-24 ((128 + 3) A_j + 4 (max s - s_j) + 4),   A_j = scale sum_d |q_d k_jd|

e_j bounds the absolute error of s_j - max s (a 128-term fp32 dot product, the scale, the subtraction) and the relative error of
__expf on it (its argument error grows with |s_j - max s|); dP_j = P_j (ds_j - sum_i P_i ds_i) gives the two score terms.  They are
some 1e-6 on N(0, 1) inputs and up to a tenth of u on the peaked profile (q and k x 3: A_j ~ 65).
ATTN_LIMIT = 1.1 is derived, not measured: the bound is rigorous to first order; the fp32 accumulation of P.V over the longest
context the kernel serves costs at most 2048 . 2^-24 / 2^-8 = 3 % of u P|v|, the fp32 sum l as much of u |o|, the second-order
terms u^2 and the two fp32 operations of the normalisation under 1 %: 7 %, held at 10 %.

(b) DECODE GEMMS  C[M, N] = A[M, K] W[N, K]^T, M <= 64.

EXACT PROFILE: A = integers in [-4, 4], W = integers in [-4, 4] x 2^-s, bias = integers in [-8, 8] x 2^-s, the fp32 residual =
integers in [-64, 64] x 2^-s.  `exact_inputs` asserts max|a| . max|w_int| . K < 2^24: every partial sum is then an integer below
2^24 (times 2^-s), exact in fp32 in ANY order -- across waves, K splits and slabs -- so the accumulation has one right answer and
the linear epilogues one right bit pattern, which float64 gives:  bf16(sum + bias);  fp32 sum + bias;  R + bf16(sum).  The check
is torch.equal.  s = ceil(log2(6.67 sqrt(K))) puts the outputs at O(1) (a power of two changes no bit of the mantissas); an
output needs a bf16 rounding when its integer sum reaches 2^8: about 1 % of them at K = 256 (half of those exact ties), a quarter
at K = 1024, over half from K = 8960.  The non-linear epilogues get exact accumulations as input, and their E bounds their own
rounding points only (gemm_skinny.hip / stream_body.h / rope.hip / norm.hip):

    SwiGLU       g = bf16(sum_g), t = bf16(sum_u) exact;  act = bf16(bf16(silu(g)) t)        E = (2u + u^2 + 2^-20) |silu(g) t|
                 (2^-20: silu_f = g / (1 + __expf(-g)) in fp32 and the fp32 product)
    bias + RoPE  x = bf16(sum + bias) exact;  y = bf16(x1 c - x2 s | x2 c + x1 s), c / s the fp32 table
                                                                                              E = u |y| + 2^-22 (|x1 c| + |x2 s|)
                 the v block and the appended cache slot: exact bits
    RMSNorm      C = R + bf16(sum) exact;  y = bf16(w (C rstd)),  rstd = rsqrtf(sum C^2 / N + eps)
                                                                                              E = (u + (N + 8) 2^-24) |y|
                 (the fp32 sum of N squares in any order: N 2^-24 relative, 5 % of u at N = 3584; 8: rsqrtf, the division,
                 the two products)
GEMM_LIMIT = 1.0: every fp32 allowance is inside E, nothing is left to a factor.

N(0, 1) PROFILE: A ~ N(0, 1), W ~ N(0, 1 / K), the inputs of tests/test_gpu_ops.py.  Second check, as for attention:
rms(err / (u |c|)) over the elements with |c| >= 2^-6 (below that the fp32 accumulation noise, ~sqrt(K) 2^-24, is no longer small
against u |c|) at most RMS_RATIO = 1.5 x the torch double's on the same inputs: round-to-nearest has rms 0.29 ulp, truncation
0.58 = 2 x, and 1.5 separates them.

The module also holds the case lists the CPU and the GPU file share, the seeded inputs of a case and the runs of the torch double
(tests/fake_ops.py) on them."""
import collections
import math

import numpy as np
import torch

from attn_ref64 import Check, assert_within, check_within  # noqa: F401  (re-exported: one checker for both reference modules)

HD = 128
U = 2.0 ** -8
ATTN_LIMIT = 1.1
GEMM_LIMIT = 1.0
RMS_RATIO = 1.5
F64, F32, BF, I32 = torch.float64, torch.float32, torch.bfloat16, torch.int32
MAX_CTX = 2048
LDS_BYTES = 160 * 1024


# ================================================================================================ cache attention
def attn_lds_floats(rep, ctx):
    """attn_decode_lds_floats of csrc/attn_decode_body.h, as written there"""
    rup4 = lambda x: (x + 3) & ~3
    return rup4(rep * ctx) + rup4(rep + 1) + rup4(ctx) + rup4(rep * ((ctx + 31) & ~31) // 2) + 8 * 2048


def attn_first_refused_ctx(rep):
    """the first context whose LDS need exceeds 160 KB (may lie beyond MAX_CTX, where the kernel refuses anyway)"""
    ctx = 1
    while attn_lds_floats(rep, ctx) * 4 <= LDS_BYTES:
        ctx += 1
    return ctx


def attn_reference(qkv, kc, vc, index, kstart, lens, M, H, G, ctx, scale):
    """qkv [M, (H+2G)*128] bf16, kc / vc [rows, ctx, G*128] bf16 (cells no visible key refers to may hold anything), index
    [M, ctx] int32 or None, kstart / lens [M].  Returns (out, E), float64 [1, M, H, 128] (the layout of check_within: s = row)."""
    rep = H // G
    q = qkv[:M, :H * HD].to(F64).view(M, G, rep, HD)
    k3, v3 = kc.view(-1, ctx, G, HD), vc.view(-1, ctx, G, HD)
    out, E = torch.zeros(1, M, H, HD, dtype=F64), torch.zeros(1, M, H, HD, dtype=F64)
    for r in range(M):
        a, b = int(kstart[r]), int(lens[r])
        pos = torch.arange(a, b)
        rows = torch.full((b - a,), r, dtype=torch.long) if index is None else index.view(M, ctx)[r, a:b].long()
        kr, vr = k3[rows, pos].to(F64), v3[rows, pos].to(F64)                      # [n, G, 128]
        s = torch.einsum("grd,ngd->grn", q[r], kr) * scale
        A = torch.einsum("grd,ngd->grn", q[r].abs(), kr.abs()) * scale
        m = s.amax(-1, keepdim=True)
        p = torch.exp(s - m)
        P = p / p.sum(-1, keepdim=True)
        o = torch.einsum("grn,ngd->grd", P, vr)
        Pe = P * (2.0 ** -24 * ((HD + 3) * A + 4 * (m - s) + 4))
        Er = U * (torch.einsum("grn,ngd->grd", P, vr.abs()) + o.abs()) + torch.einsum("grn,ngd->grd", Pe, vr.abs()) \
            + o.abs() * Pe.sum(-1, keepdim=True)
        out[0, r], E[0, r] = o.reshape(H, HD), Er.reshape(H, HD)
    return out, E


AttnCase = collections.namedtuple("AttnCase", "M H G ctx indexed profile")

# visible lengths on every switch of the kernel: one key; the 16-key score chunk; the 32-key V block; the softmax's register-held
# keys; the first K chunk past the prefetch (3 chunks x 8 waves x 16); the first V block past it (2 x 8 x 32); the whole row
SWITCH_LENGTHS = [1, 15, 16, 17, 31, 32, 33, 256, 257, 384, 385, 512, 513]
ATTN_CASES = [AttnCase(64, 12, 2, 640, True, "n01"),      # REP 6, every switch length in one launch
              AttnCase(64, 4, 2, 520, False, "peaked"),   # REP 2, the rows' own cache rows
              AttnCase(9, 2, 2, 530, True, "n01"),        # REP 1
              AttnCase(9, 4, 1, 300, False, "n01"),       # REP 4
              AttnCase(9, 7, 1, 530, True, "peaked"),     # REP 7
              AttnCase(9, 8, 1, 400, True, "n01"),        # REP 8
              AttnCase(9, 28, 4, 530, True, "n01"),       # REP 7, four groups
              AttnCase(1, 12, 2, 2048, True, "n01"),      # the longest context
              AttnCase(1, 2, 2, 2048, False, "peaked"),
              AttnCase(1, 8, 1, attn_first_refused_ctx(8) - 1, True, "n01"),      # REP 8 cannot take 2048: the largest it takes
              AttnCase(1, 6, 1, 40, False, "n01")]


def attn_case_id(c):
    return f"M{c.M}-H{c.H}-G{c.G}-ctx{c.ctx}-{'index' if c.indexed else 'own'}-{c.profile}"


def attn_inputs(c):
    """Seeded inputs of a case.  Row r sees n_r keys, n_r walking through SWITCH_LENGTHS (clipped to the context) with the whole
    context on rows 0 mod 14 ... (M = 1: the whole context); kstart ragged where the row has room.  The caches have one extra
    physical row M; it, every cell no (row, visible position) refers to, are NaN, and every index entry outside the row's visible
    range points at row M -- inside the allocation, poisoned.  dict(qkv, kc, vc, index, kstart, lens) + scalars."""
    M, H, G, ctx = c.M, c.H, c.G, c.ctx
    W, LD = G * HD, (H + 2 * G) * HD
    gen = torch.Generator().manual_seed(100000 * M + 10 * ctx + H + G)
    rs = np.random.RandomState(ctx + M)
    qkv = torch.randn(M, LD, generator=gen)
    k, v = torch.randn(M + 1, ctx, W, generator=gen), torch.randn(M + 1, ctx, W, generator=gen)
    if c.profile == "peaked":
        qkv[:, :H * HD] *= 3.0
        k *= 3.0
    want = ([ctx] + SWITCH_LENGTHS) if M > 1 else [ctx]
    nvis = np.array([min(want[(r + M + H) % len(want)], ctx) for r in range(M)], dtype=np.int64)
    kstart = np.minimum((np.arange(M) * 5) % 9, ctx - nvis).astype(np.int32)
    lens = (kstart + nvis).astype(np.int32)
    seen = torch.zeros(M + 1, ctx, dtype=torch.bool)
    index = torch.full((M, ctx), M, dtype=I32) if c.indexed else None
    for r in range(M):
        a, b = int(kstart[r]), int(lens[r])
        if c.indexed:
            index[r, a:b] = torch.from_numpy(rs.randint(0, M, size=b - a).astype(np.int32))
            seen[index[r, a:b].long(), torch.arange(a, b)] = True
        else:
            seen[r, a:b] = True
    kc, vc = k.to(BF), v.to(BF)
    kc[~seen], vc[~seen] = float("nan"), float("nan")
    return dict(qkv=qkv.to(BF), kc=kc, vc=vc, index=index, kstart=torch.from_numpy(kstart), lens=torch.from_numpy(lens),
                M=M, H=H, G=G, ctx=ctx, scale=HD ** -0.5)


def attn_reference_of(inp):
    return attn_reference(inp["qkv"], inp["kc"], inp["vc"], inp["index"], inp["kstart"], inp["lens"], inp["M"], inp["H"], inp["G"],
                          inp["ctx"], inp["scale"])


def attn_double(fake, inp, **change):
    """fake.attn_decode on the inputs: out [1, M, H, 128] bf16.  `change`: replaced inputs (the mutants).  The double views the
    caches as [M, ctx, ...], so a cache with a poisoned extra row M is run as M + 1 query rows (the last one a dummy that sees
    one key) and the dummy's output row is dropped."""
    i = dict(inp, **change)
    M, H, G, ctx = i["M"], i["H"], i["G"], i["ctx"]
    R = i["kc"].numel() // (ctx * G * HD)
    index = i["index"] if i["index"] is not None else torch.arange(M, dtype=I32)[:, None].expand(M, ctx).contiguous()
    pad = lambda t, fill: torch.cat([t, torch.full((R - M,) + tuple(t.shape[1:]), fill, dtype=t.dtype)])
    out = torch.zeros(R, H * HD, dtype=BF)
    fake.attn_decode(pad(i["qkv"], 0), i["kc"].reshape(-1), i["vc"].reshape(-1), pad(index, 0), pad(i["kstart"], 0), pad(i["lens"], 1),
                     out, R, H, G, ctx, i["scale"])
    return out[:M].view(1, M, H, HD)


def attn_legacy_inputs(H, G, ctx):
    """the inputs of tests/test_gpu_ops.py::test_attn_decode_long_ragged_contexts (no poison, M = 9): the mutants' old scores are
    measured where that test measures"""
    M, W, LD = 9, G * HD, (H + 2 * G) * HD
    rn = lambda n, seed, scale=1.0: (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale).to(BF)
    rs = np.random.RandomState(ctx)
    qkv = rn(M * LD, 11).view(M, LD)
    kc, vc = rn(M * ctx * W, 12, 0.7), rn(M * ctx * W, 13, 0.7)
    lens = np.array([1, 2, 17, ctx, ctx - 1, ctx // 2, 385, min(513, ctx), 33][:M], dtype=np.int32).clip(1, ctx)
    kstart = np.minimum(rs.randint(0, 9, size=M), lens - 1).astype(np.int32)
    index = torch.from_numpy(rs.randint(0, M, size=(M, ctx)).astype(np.int32))
    return dict(qkv=qkv, kc=kc, vc=vc, index=index, kstart=torch.from_numpy(kstart), lens=torch.from_numpy(lens), M=M, H=H, G=G,
                ctx=ctx, scale=HD ** -0.5)


# ================================================================================================ decode GEMMs
GemmCase = collections.namedtuple("GemmCase", "op M N K mode bias H G ctx")


def _g(op, M, N, K, mode=0, bias=False, H=0, G=0, ctx=0):
    return GemmCase(op, M, N, K, mode, bias, H, G, ctx)


# The smallest shapes that reach each mechanism (256 CUs).  gemm_skinny.hip's plan: BN = 96 needs ceil(N / 96) >= 0.6 x CUs AND
# more than one round of 64-wide tiles, N in (16384, 24576] (SwiGLU: I in (8192, 12288]); fewer tiles are split over K, at most
# 4 ways for K <= 2048, 32 ways beyond, never below 4 K-steps per split.  gemm_stream.hip: one K range of 256 / 512 / 1280 / 1536 /
# 1792 / 3584, or slabs of those.
PLAIN_CASES = [_g("plain", 1, 64, 256),                          # BN = 64, unsplit
               _g("plain", 17, 64, 1024, bias=True),             # split 4 ways (K <= 2048)
               _g("plain", 64, 64, 8960, mode=2),                # split 32 ways
               _g("plain", 64, 1536, 8960, mode=1),              # 24 tiles x 10 splits
               _g("plain", 64, 1000, 256, mode=1, bias=True),    # N no multiple of 16, ldc > N
               _g("plain", 17, 40, 512, bias=True),              # N < a tile
               _g("plain", 17, 40, 512, mode=2, bias=True),
               _g("plain", 64, 16500, 256, bias=True),           # BN = 96
               _g("plain", 17, 16500, 256, mode=2),
               _g("plain", 64, 208, 1280),                       # the streaming kernels' K ranges
               _g("plain", 33, 1000, 1536, bias=True),
               _g("plain", 64, 208, 1792, bias=True),
               _g("plain", 1, 1000, 3584),
               _g("plain", 64, 72, 3584, bias=True),
               _g("plain", 64, 256, 18944, mode=2)]              # the one model-sized K
SWIGLU_CASES = [_g("swiglu", 64, 8200, 256),                     # BN = 96
                _g("swiglu", 17, 200, 512),
                _g("swiglu", 1, 96, 1792),
                _g("swiglu", 64, 256, 3584),
                _g("swiglu", 40, 40, 1280),
                _g("swiglu", 33, 64, 1024)]                      # split K on gemm_skinny.hip only
NORM_CASES = [_g("norm", 64, 256, 256),                          # unsplit + tasu_rmsnorm_fwd / one range
              _g("norm", 17, 1536, 1024),                        # 2 equal ranges
              _g("norm", 64, 1536, 8960),                        # 7 x 1280 and 5 x 1792; row-in-registers finish
              _g("norm", 1, 256, 18944),                         # ragged: 12 x 1536 + 512
              _g("norm", 33, 4352, 1024),                        # N > 4096: the looped finish
              _g("norm", 64, 512, 1536)]
QKV_CASES = [_g("qkv", 64, 512, 256, bias=True, H=2, G=1, ctx=16),
             _g("qkv", 17, 2048, 1536, bias=True, H=12, G=2, ctx=24),
             _g("qkv", 1, 512, 1024, bias=True, H=2, G=1, ctx=8),            # split K finish (skinny_reduce_rope)
             _g("qkv", 33, 512, 3584, bias=False, H=2, G=1, ctx=40)]
GEMM_CASES = PLAIN_CASES + SWIGLU_CASES + NORM_CASES + QKV_CASES
EPS = 1e-6


def gemm_case_id(c):
    return f"{c.op}-{c.M}x{c.N}x{c.K}-mode{c.mode}{'-bias' if c.bias else ''}"


def exact_shift(K):
    return int(math.ceil(math.log2(6.67 * math.sqrt(K))))


def gemm_inputs(c, profile):
    """Seeded inputs of a case, profile "exact" or "n01": dict(a [M, K] bf16, w [rows, K] bf16 (rows = N, SwiGLU: 2 N gate | up),
    bias [N] bf16 / None, resid [M, ldc] fp32 / None, norm_w [N] fp32, cos / sin [M, 64] fp32, pos [M] int32, ldc)."""
    M, N, K = c.M, c.N, c.K
    rows = 2 * N if c.op == "swiglu" else N
    ldc = N if c.op in ("norm", "qkv", "swiglu") else (N + 63) // 64 * 64 + 64
    gen = torch.Generator().manual_seed(7 * N + K + M)
    ri = lambda lo, hi, *sh: torch.randint(lo, hi + 1, sh, generator=gen).to(F32)
    d = dict(ldc=ldc, profile=profile, bias=None, resid=None)
    if profile == "exact":
        s = 2.0 ** -exact_shift(K)
        a, w = ri(-4, 4, M, K), ri(-4, 4, rows, K)
        assert float(a.abs().max()) * float(w.abs().max()) * K < 2 ** 24
        d["a"], d["w"] = a.to(BF), (w * s).to(BF)
        if c.bias:
            d["bias"] = (ri(-8, 8, N) * s).to(BF)
        if c.mode == 2 or c.op == "norm":
            d["resid"] = ri(-64, 64, M, ldc) * s
    else:
        d["a"] = torch.randn(M, K, generator=gen).to(BF)
        d["w"] = (torch.randn(rows, K, generator=gen) / math.sqrt(K)).to(BF)
        if c.bias:
            d["bias"] = torch.randn(N, generator=gen).to(BF)
        if c.mode == 2 or c.op == "norm":
            d["resid"] = torch.randn(M, ldc, generator=gen)
    d["norm_w"] = torch.randn(N, generator=gen).abs() + 0.5
    ang = torch.randn(M, 64, generator=gen)
    d["cos"], d["sin"] = torch.cos(ang), torch.sin(ang)
    if c.op == "qkv":
        pos = torch.randint(0, c.ctx, (M,), generator=gen).to(I32)
        pos[0] = c.ctx - 1                                      # the last slot; the first one where there is a second row
        if M > 1:
            pos[M - 1] = 0
        d["pos"] = pos
    return d


def cache_pattern(M, ctx, W, salt):
    """a recognisable non-zero cache image (every cell != 0, neighbours differ): an append to the wrong slot shows"""
    i = torch.arange(M * ctx * W, dtype=torch.int64)
    return (((i * 37 + salt) % 251).to(F32) + 1.0).to(BF)


def _bf64(x):
    """float64 -> the nearest bf16 (ties to even), as float64.  Through fp32 first: callers pass values exact in fp32 (the
    exact profile) or accept the double rounding's 2^-24 (the N(0, 1) profile's yardstick is statistical)."""
    return x.to(F32).to(BF).to(F64)


GemmRef = collections.namedtuple("GemmRef", "exact tol frac_rounded scale")


def gemm_reference(c, d):
    """The float64 results of a case.  exact: name -> tensor whose BITS are the right answer; tol: name -> (ref, E) float64, held
    within GEMM_LIMIT x E; frac_rounded: the share of accumulations a bf16 rounding changes; scale: name -> the magnitude the
    N(0, 1) statistic divides by where it is not |ref| (the rotation: |x1 c| + |x2 s|, which |y| falls far below where it cancels).  On the N(0, 1) profile the
    accumulation is not exact: `exact` is empty, ref is the operator on the unrounded float64 sums and E is None -- ref serves
    the rms statistic (rms_ulp) alone."""
    M, N = c.M, c.N
    acc = d["a"].to(F64) @ d["w"].to(F64).t()
    ex = d["profile"] == "exact"
    if ex:
        assert torch.equal(acc, acc.to(F32).to(F64)), "the exact profile's sums are not exact in fp32"
    rnd = _bf64 if ex else (lambda t: t)                         # the exact profile's roundings of exact sums are exact bits
    frac = float((_bf64(acc) != acc).double().mean())
    bias = 0.0 if d["bias"] is None else d["bias"].to(F64)
    exact, tol, scale = {}, {}, {}
    if c.op == "plain":
        z = acc + bias
        if c.mode == 2:
            z = d["resid"][:, :N].to(F64) + rnd(z)
        if ex:
            exact["c"] = z.to(F32).to(BF) if c.mode == 0 else z.to(F32)
        else:
            tol["c"] = (z, None)
    elif c.op == "swiglu":
        g, t = rnd(acc[:, :N]), rnd(acc[:, N:])
        act = g / (1.0 + torch.exp(-g)) * t
        tol["act"] = (act, (2 * U + U * U + 2.0 ** -20) * act.abs() if ex else None)
    elif c.op == "norm":
        C = d["resid"].to(F64) + rnd(acc)
        y = d["norm_w"].to(F64) * C * (C.pow(2).mean(-1, keepdim=True) + EPS).rsqrt()
        if ex:
            exact["c"] = C.to(F32)
        else:
            tol["c"] = (C, None)
        tol["y"] = (y, (U + (N + 8) * 2.0 ** -24) * y.abs() if ex else None)
    else:
        H, G = c.H, c.G
        x = rnd(acc + bias).view(M, H + 2 * G, HD)
        cs, sn = d["cos"].to(F64)[:, None, :], d["sin"].to(F64)[:, None, :]
        x1, x2 = x[:, :H + G, :64], x[:, :H + G, 64:]
        rot = torch.cat([x1 * cs - x2 * sn, x2 * cs + x1 * sn], -1)
        slop = torch.cat([(x1 * cs).abs() + (x2 * sn).abs(), (x2 * cs).abs() + (x1 * sn).abs()], -1)
        tol["qk"] = (rot.reshape(M, -1), (U * rot.abs() + 2.0 ** -22 * slop).reshape(M, -1) if ex else None)
        scale["qk"] = slop.reshape(M, -1)
        v = x[:, H + G:].reshape(M, -1)
        if ex:
            exact["v"] = v.to(F32).to(BF)
        else:
            tol["v"] = (v, None)
    return GemmRef(exact, tol, frac, scale)


def gemm_double(fake, c, d, **change):
    """The torch double on a case: name -> result tensor (same names as gemm_reference; qkv: + kc, vc, kc0, vc0 -- the caches after
    and before the append).  `change`: replaced inputs."""
    d = dict(d, **change)
    M, N, K, ldc = c.M, c.N, c.K, d["ldc"]
    if c.op == "plain":
        out = torch.full((M, ldc), float("nan"), dtype=BF if c.mode == 0 else F32)
        fake.gemm_skinny(d["a"], d["w"], out, M, N, K, None, bias=d["bias"], resid=d["resid"], mode=c.mode)
        return {"c": out[:, :N]}
    if c.op == "swiglu":
        act = torch.zeros(M, N, dtype=BF)
        fake.gemm_skinny_swiglu(d["a"], d["w"], act, M, N, K, None)
        return {"act": act}
    if c.op == "norm":
        cc, y = torch.zeros(M, N), torch.zeros(M, N, dtype=BF)
        fake.gemm_skinny_norm(d["a"], d["w"], cc, d["resid"], M, N, K, d["norm_w"], y, EPS, None)
        return {"c": cc, "y": y}
    H, G, W = c.H, c.G, c.G * HD
    kc0, vc0 = cache_pattern(M, c.ctx, W, 1), cache_pattern(M, c.ctx, W, 2)
    kc, vc, qkv = kc0.clone(), vc0.clone(), torch.zeros(M, N, dtype=BF)
    fake.gemm_skinny_qkv_rope(d["a"], d["w"], d["bias"], qkv, M, H, G, K, d["cos"], d["sin"], kc, vc, d["pos"], c.ctx, None)
    return {"qk": qkv[:, :(H + G) * HD], "v": qkv[:, (H + G) * HD:], "kc": kc, "vc": vc, "kc0": kc0, "vc0": vc0}


def _locate(score):
    i = int(score.argmax())
    return i // score.shape[1], i % score.shape[1]


def gemm_message(what, m, n, got, want, K, ranges, extra=""):
    t = n // 16
    return (f"{what}: worst at (row {m}, column {n}) in 16-column tile {t} (columns {16 * t}-{16 * t + 15}), K range [0, {K}) "
            f"{ranges}: got {float(got)!r}, reference {float(want)!r}{extra}")


def assert_bits(got, want, what, K, ranges=""):
    """got == want bit for bit ([M, N], same dtype); names the element furthest off, its 16-column tile and the K range"""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if torch.equal(got, want):
        return
    err = (got.to(F64) - want.to(F64)).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, math.inf))
    bad = int((err > 0).sum())
    m, n = _locate(err)
    raise AssertionError(gemm_message(f"{what}: {bad} of {got.numel()} elements differ from the exact result", m, n, got[m, n], want[m, n],
                                      K, ranges))


def check_gemm(got, ref, E, limit, what, K, ranges=""):
    """check_within on [M, N] tensors with the GEMM's failure message"""
    M, N = ref.shape
    c = check_within(got.reshape(1, M, 1, N), ref.reshape(1, M, 1, N), E.reshape(1, M, 1, N), limit, what)
    if c.ok:
        return c
    g = got.to(F64)
    score = torch.where(torch.isfinite(g), (g - ref).abs() / E.clamp_min(1e-300), torch.full_like(ref, math.inf))
    m, n = _locate(score)
    msg = gemm_message(c.message.split(";")[0], m, n, got[m, n], ref[m, n], K, ranges,
                       f", bound E {float(E[m, n]):.3e}, |err| / E = {c.worst:.3f}")
    return Check(False, c.rms, c.worst, msg)


def assert_gemm_within(got, ref, E, limit, what, K, ranges=""):
    c = check_gemm(got, ref, E, limit, what, K, ranges)
    assert c.ok, c.message
    return c


def rms_ulp(got, ref, scale=None):
    """rms(err / (u |c|)) over the elements with |c| >= 2^-6: the N(0, 1) profile's statistic (scale: in place of |c|)"""
    mag = ref.abs() if scale is None else scale
    g, keep = got.to(F64), mag >= 2.0 ** -6
    return float((((g - ref).abs() / (U * mag.clamp_min(1e-300)))[keep]).pow(2).mean().sqrt())


def check_gemm_case(case, d, ref, out, limit, what, ranges=""):
    """one run's results of a case against the reference: the bits where float64 names them, limit x E elsewhere, the appended
    cache slots; returns the largest |err| / E"""
    worst = 0.0
    for name, want in ref.exact.items():
        assert_bits(out[name], want, f"{what} {name}", case.K, ranges)
    for name, (want, E) in ref.tol.items():
        if E is not None:
            worst = max(worst, assert_gemm_within(out[name], want, E, limit, f"{what} {name}", case.K, ranges).worst)
    if case.op == "qkv":
        check_appended(out, case, d, what)
    return worst


def rms_pairs(c, d, ref, out):
    """(name, got, want, scale) float64 of the results the N(0, 1) statistic is taken on: the bf16-rounded ones -- an fp32
    `R + bf16(sum)` less its R, the fp32-output mode not at all"""
    for name, (want, _) in ref.tol.items():
        if c.op == "plain" and c.mode == 1:
            continue
        got = out[name].to(F64)
        if name == "c" and d["resid"] is not None:
            r = d["resid"][:, :c.N].to(F64)
            got, want = got - r, want - r
        yield name, got, want, ref.scale.get(name)


def check_appended(out, c, d, what):
    """the caches after a q|k|v call: exactly the cells [m, pos[m]] changed, and they hold the bits of the k and v blocks of qkv[m]"""
    M, H, G, W = c.M, c.H, c.G, c.G * HD
    qk, v = out["qk"], out["v"]
    rows = torch.arange(M)
    for name, after, before, block in (("k", out["kc"], out["kc0"], qk[:, H * HD:]), ("v", out["vc"], out["vc0"], v)):
        a3, want = after.view(M, c.ctx, W).view(torch.int16), before.view(M, c.ctx, W).clone()
        want[rows, d["pos"].long()] = block
        wrong = (a3 != want.view(torch.int16)).any(-1)
        assert not bool(wrong.any()), (f"{what}: {name} cache differs from 'old image + the row's block at pos[m]' at (row, slot) "
                                       f"{[tuple(x) for x in torch.nonzero(wrong)[:4].tolist()]}, pos = {d['pos'].tolist()}")


# ================================================================================================ the norm inside its neighbours
def prenorm_weight(N, seed):
    """a norm weight of powers of two: bf16(norm_w . C) of an exact C is then exact, and an integer on the grid again"""
    return 2.0 ** torch.randint(-1, 2, (N,), generator=torch.Generator().manual_seed(seed)).to(F32)


def rstd_consumer_reference(kind, yw, w, ssq, M, K, eps, unit, bias=None, cos=None, sin=None, H=0, G=0):
    """tasu_gemm_stream_swiglu_rstd / _qkv_rope_rstd by their definition (gemm_stream.hip): the accumulators of yw W^T scaled by
    rstd[m] = rsqrt(sum_t ssq[t, m] / K + eps) before the epilogue.  yw [M, K] bf16 and ssq [K / 16, 64] fp32 are INPUTS (what the
    producer left); every product yw w is a multiple of `unit` and sum |yw w| < 2^24 unit, so yw W^T is exact in fp32 in any order
    (asserted).  Returns name -> (ref, E); E mirrors rstd applied to the
    accumulators: the fp32 s = acc . rstd carries e_r = (K / 16 + 10) 2^-24 (the K / 16 partials summed in any order, rsqrtf, the
    division, the product) and one bf16 rounding, which the epilogue propagates to first order -- SwiGLU through silu'(g) t and
    silu(g), the rotation through |c| and |s| -- next to its own roundings (module docstring); (1 + 4u) covers the second order."""
    acc = yw[:M].to(F64) @ w.to(F64).t()
    assert torch.equal(acc / unit, (acc / unit).round()) and float((yw[:M].to(F64).abs() @ w.to(F64).abs().t()).max()) / unit < 2 ** 24, \
        "yw W^T is not exact in fp32"
    rstd = (ssq[:K // 16, :M].to(F64).sum(0) / K + eps).rsqrt()[:, None]
    e_r = (K // 16 + 10) * 2.0 ** -24
    s = acc * rstd
    if kind == "swiglu":
        I = w.shape[0] // 2
        g, t = s[:, :I], s[:, I:]
        sg = 1.0 / (1.0 + torch.exp(-g))
        act = g * sg * t
        dsilu = (sg * (1.0 + g * (1.0 - sg))).abs()
        E = dsilu * (U + e_r) * g.abs() * t.abs() + (g * sg).abs() * (U + e_r) * t.abs() + (2 * U + U * U + 2.0 ** -20) * act.abs()
        return {"act": (act, (1 + 4 * U) * E)}
    b = 0.0 if bias is None else bias.to(F64)
    x = (s + b).view(M, H + 2 * G, HD)
    Ex = (U * (s + b).abs() + e_r * s.abs() + 2.0 ** -24 * (s + b).abs()).view(M, H + 2 * G, HD)
    cs, sn = cos.to(F64)[:, None, :], sin.to(F64)[:, None, :]
    x1, x2, E1, E2 = x[:, :H + G, :64], x[:, :H + G, 64:], Ex[:, :H + G, :64], Ex[:, :H + G, 64:]
    rot = torch.cat([x1 * cs - x2 * sn, x2 * cs + x1 * sn], -1)
    Erot = torch.cat([E1 * cs.abs() + E2 * sn.abs() + 2.0 ** -22 * ((x1 * cs).abs() + (x2 * sn).abs()),
                      E2 * cs.abs() + E1 * sn.abs() + 2.0 ** -22 * ((x2 * cs).abs() + (x1 * sn).abs())], -1) + U * rot.abs()
    return {"qk": (rot.reshape(M, -1), (1 + 4 * U) * Erot.reshape(M, -1)),
            "v": (x[:, H + G:].reshape(M, -1), (1 + 4 * U) * Ex[:, H + G:].reshape(M, -1))}


def check_sumsq(ssq, C, M, N, what):
    """the per-(16-column tile, row) sums of squares ssq [N / 16, 64] of C [M, N]: each within 20 . 2^-24 of its 16 squares' sum
    (16 fp32 products and 15 additions in any order)"""
    want = C[:M].to(F64).pow(2).view(M, N // 16, 16).sum(-1).t()                 # [N / 16, M]
    got = ssq[:N // 16, :M].to(F64)
    bad = (got - want).abs() > 20 * 2.0 ** -24 * want
    assert not bool(bad.any()), f"{what}: sums of squares off at (tile, row) {[tuple(x) for x in torch.nonzero(bad)[:4].tolist()]}"
