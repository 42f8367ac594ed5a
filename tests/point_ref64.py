"""TEST HELPER (not a test, never shipped): plain float64 restatements of the rotary, pointwise and encoder-memory kernels --
tasu_rope_table / tasu_rope_fwd / tasu_rope_bwd (csrc/rope.hip), tasu_silu_fwd/bwd, tasu_relu_fwd/bwd, tasu_swiglu_fwd/bwd,
tasu_cast_f32_bf16 (csrc/elementwise.hip), tasu_sinusoid_pe, tasu_fsmn_fwd, tasu_fsmn_ln_fwd (csrc/encoder_aux.hip) -- on the exact
input values, each with a first-order bound E for every element it returns.  Nothing is shared with the kernels or with
tests/fake_ops.py.  `check` / `check_within`, `same_bits`, `untouched`, `nan`, U = 2^-8, RMS_RATIO = 1.5 and e = 2^-24 are those of
tests/row_ref64.py, `fl32` / `bf16r` those of tests/lora_ref64.py.  LIMIT = 1.0: every fp32 allowance is inside E.  E = 0 means the
reference's VALUE exactly (zeros compare as values); Ref.exact means its bits.

    rope_table     ang = pos theta^(-i / 64).  The kernel: inv = 1 / powf(theta, i / 64), ang = fl32(pos inv), sincosf(ang).
                   E = e (|ang| (P + 2) + Q): P, Q the allowances of powf and sincosf in units of e (POW_E, SINCOS_E below), 2 the
                   correctly rounded division and product.  pos = 0: cos = 1, sin = +0 bit for bit.  i = 0: inv is exactly 1, the
                   angle is the integer pos: E = e Q alone (the argument reduction of sincosf up to 32767).  Q = 4 (2 ulp, what
                   the project grants rsqrtf) holds: sincosf was measured at 0.82 e on those columns.  P = 4 does NOT hold on a
                   correct kernel: at |ang| >= 64 the chain was measured at 8.65 e |ang| (theta 1e6; 7.08 at 1e4), i.e. powf up to
                   3.3 ulp, 1.71 x the E of P = 4.  P is therefore the figure the device library is specified to, OpenCL full
                   profile's 16 ulp for pow = 32 e -- for this function only, and not fitted to the kernel's output.
    rope_fwd       y = bf16(x1 c - x2 s | x2 c + x1 s) on the q and k heads, (x1, x2) = dims (d, d + 64), c / s the fp32 table (an
                   INPUT: the same fp32 values go to the kernel and to the reference).  E = u |y| + 2^-22 (|x1 c| + |x2 s|) (the
                   bound of gemm_ref64 / decode_ref64 for rope_pair_f: one rounded product, one FMA).  pos = 0: the input's bits.
                   v heads: the input's bits.  Transposed copies [B, heads, 128, Spad]: the transpose's bits of the in-place
                   result, +0 in columns S .. Spad - 1, NaN (untouched) behind the last head.
    rope_bwd       q heads: dx = bf16(dy1 c + dy2 s | dy2 c - dy1 s) from the bf16 dQ in place, the bound above.  k heads: the
                   np_g fp32 partials of the group summed in order (np_g - 1 rounded additions), un-rotated, rounded:
                   E = u |dx| + |c| S1 + |s| S2 + 2^-22 (|y1 c| + |y2 s|), S = (np_g - 1) e sum_r |part_r| of the half the factor
                   multiplies.  v heads: bf16(sum), E = u |sum| + S.  np_g = (H / G) / hpb, hpb = 3 | 2 | 1 (the first that divides
                   H / G); partial r of group g of token m sits at m (H / hpb) 128 + (g np_g + r) 128.  Exact profile (partials and
                   dQ integers in [-8, 8] x 2^-3): the v heads, and every head at pos = 0, have float64's value (E = 0).
    silu_fwd       y = g / (1 + exp(-g)); the kernels use __expf: a1 = (2 |g| + 6) e is the relative error of sg and of silu
                   (gemm_ref64's header).  E = (u + a1) (1 + u) |y|.
    swiglu_fwd     bf16(bf16(silu g) t):  E = (2u + u^2 + a1 + 2e) (1 + u) |silu(g) t|.  That bound grants the intermediate rounding
                   and so cannot see it missing; where every value within 4 a1 of silu(g) rounds to one bf16 value sb (all but a few
                   elements in a thousand), sb t is exact in fp32 and the output has ONE right value, bf16(sb t): E = 0 there.
    swiglu_bwd     dg = d t sg f, du = d g sg, f = 1 + g (1 - sg);  E_f = |g| (sg a1 + e) + 2e (1 + |g| (1 - sg)),
                   E_dg = u |dg| + |d t| sg (a1 |f| + E_f) + 4e |dg|,  E_du = (u + a1 + 4e) |du|   (gemm_ref64's dswiglu bounds)
    silu_bwd       E_dg with t = 1
    relu_fwd       max(x, 0) as a value (fmaxf(-0, 0) has no defined sign);  relu_bwd: dy's bits where x > 0, else +0
    cast           the nearest bf16, ties to even, ONE rounding: the reference rounds the fp32 BITS by integer arithmetic
                   (`cast_bits`; equal to bf16r wherever bf16r is defined, which tests/test_point_ref64_cpu.py asserts)
    sinusoid_pe    y = x scale + PE, PE(t, d) = sin | cos((t + 1) exp(-k inc)), inc = ln(1e4) / (D / 2 - 1), k = d mod D / 2.  With
                   arg = k inc and ang the float64 angle:  E = e (|ang| (2 arg + X + 4) + Q) + 2e (|x scale| + |y|): logf, the
                   division, k inc and the product by t + 1 one e each, the argument's error enters expf as 2e arg relative, X =
                   EXP_E = 2 the library expf (1 ulp, as row_ref64 grants it), Q as for the table; the last term holds for a fused
                   and for an unfused x scale + PE.  k = 0: the angle is the integer t + 1 exactly, E = e Q + 2e (...).
    fsmn_fwd       out (+)= [t < len] (sum_j w[d][j] v[t + j - left] [0 <= t + j - left < len] + v[t]), left = (ks - 1) / 2.
                   Any order: E = (ks + 1) e (sum_j |w v| + |v_t|), + e (|out0| + |result|) when accumulating.  Frames t >= len:
                   +0 / out0 exactly.  Exact profile (v integers in [-4, 4], w integers x 2^-3, out0 integers x 2^-3): float64's bits.
    fsmn_ln_fwd    x: the bits of fsmn_fwd(accumulate) through the same ops; xn: row_ref64's LayerNorm reference of THAT x, its E

SUBNORMALS.  The kernels flush and u |ref| means nothing for a bf16 subnormal: every reference asserts that each exact result is
zero or at least 2^-100 in magnitude (`normal`).  One family cannot keep that floor and the edge row it is given: silu(-80) is
1.4e-33 = 2^-109.  The activation references therefore assert 2^-120 (ACT_FLOOR: still 64 binades above bf16's smallest normal
number and the smallest magnitude bf16r handles), and the edge row leaves out (g = -80, |t| = |d| = 2^-6) in SwiGLU backward, whose
fp32 product d t sg would itself be subnormal.  |g| <= 80 is asserted (below about -88.7 __expf overflows: not reached).

The module also holds the case lists, the seeded inputs with their NaN guards (every operand has NaN outside what the kernel is
owed, every output starts as NaN with guard rows / elements that must keep their bits) and the runs (`run_*`: each runs TWICE and
requires equal bits) that tests/test_point_ref64_cpu.py (through the torch double) and tests/test_gpu_point_f64.py (through HipOps)
share."""
import collections
import math

import torch

from lora_ref64 import bf16r, fl32  # noqa: F401
from row_ref64 import (BF, F32, F64, GUARD, I32, LIMIT, NAN, RMS_RATIO, U, Ref, _back, _call, assert_within, bits,  # noqa: F401
                       cdiv, check, check_within, e, gen, ln_reference, nan, rms_stat, same_bits, untouched, worst_of)

HD = 128
POW_E, SINCOS_E, EXP_E = 32.0, 4.0, 2.0                          # allowances of powf, sincosf / sinf / cosf, expf in units of e
TINY, ACT_FLOOR = 2.0 ** -100, 2.0 ** -120
G_MAX = 80.0
GE = 11                                                          # guard elements behind a flat output


def case_id(c):
    return "-".join(str(v) for v in c)


def normal(x, what, floor=TINY):
    """every exact result is zero or at least `floor` in magnitude"""
    a = x.abs()
    assert bool(((a == 0) | (a >= floor)).all()), f"{what}: an exact result below {floor:g} in magnitude (a subnormal in waiting)"
    return x


def guarded_rows(t, rows=GUARD):
    """operand [R, C] -> [R + rows, C] with NaN guard rows (int32: -7)"""
    fill = torch.full((rows,) + tuple(t.shape[1:]), -7 if t.dtype == I32 else NAN, dtype=t.dtype)
    return torch.cat([t, fill])


def guarded_flat(t, n=GE):
    return torch.cat([t.reshape(-1), torch.full((n,), NAN, dtype=t.dtype)])


def twice(run, what, again=True):
    """two runs from fresh buffers: equal bits; the first run's outputs (again = False: one run -- the GPU file's double)"""
    a = run()
    if not again:
        return a
    b = run()
    for name in a:
        if a[name] is not None:
            same_bits(b[name], a[name], f"{what}: second run, {name}")
    return a


# ================================================================================================ rope_table
TableCase = collections.namedtuple("TableCase", "theta")
TABLE_CASES = [TableCase(1e6), TableCase(1e4)]
TABLE_FIXED = [0, 1, 2, 63, 64, 511, 4095, 32767]


def table_inputs(c):
    pos = torch.tensor(TABLE_FIXED + torch.randint(0, 32768, (40,), generator=gen(int(c.theta), 1)).tolist() + [4095], dtype=I32)
    assert pos.numel() == 49 and pos.numel() % 4 and int(pos.max()) <= 32767
    return dict(pos=pos, M=pos.numel(), theta=c.theta)


def table_angles(pos, theta):
    i = torch.arange(HD // 2, dtype=F64)
    return pos.to(F64)[:, None] * torch.tensor(theta, dtype=F64).pow(-i / (HD // 2))[None]


def table_reference(d, P=None, Q=None):
    P, Q = POW_E if P is None else P, SINCOS_E if Q is None else Q
    ang = table_angles(d["pos"], d["theta"])
    E = e * (ang.abs() * (P + 2) + Q)
    E[:, 0] = e * Q                                              # inv = 1 exactly: the integer angle
    E[d["pos"] == 0] = 0.0
    return Ref({"cos": (normal(ang.cos(), "rope_table cos"), E), "sin": (normal(ang.sin(), "rope_table sin"), E.clone())}, {})


def run_table(ops, d, to=None):
    ops, to = _call(ops, to)
    M = d["M"]

    def once():
        cs, sn = to(nan(M + GUARD, HD // 2)), to(nan(M + GUARD, HD // 2))
        ops.rope_table(to(d["pos"]), cs[:M], sn[:M], HD, d["theta"])
        cs, sn = _back(cs, sn)
        assert untouched(cs[M:]) and untouched(sn[M:]), "rope_table: rows past M were written"
        return {"cos": cs[:M], "sin": sn[:M]}

    out = twice(once, "rope_table")
    pos = d["pos"]
    z = pos == 0
    same_bits(out["cos"][z], torch.ones(int(z.sum()), HD // 2), "rope_table cos at pos = 0")
    same_bits(out["sin"][z], torch.zeros(int(z.sum()), HD // 2), "rope_table sin at pos = 0")
    for a in range(M):                                           # equal positions: equal rows
        for b in range(a + 1, M):
            if int(pos[a]) == int(pos[b]):
                same_bits(out["cos"][b], out["cos"][a], f"rope_table cos rows {a} and {b} (one position)")
                same_bits(out["sin"][b], out["sin"][a], f"rope_table sin rows {a} and {b} (one position)")
    return out


def table_f32(pos, theta=1e6):
    """the fp32 table the rotation tests pass to the kernel AND to the reference: the float64 table rounded once"""
    ang = table_angles(pos, theta)
    return ang.cos().to(F32), ang.sin().to(F32)


# ================================================================================================ rope_fwd
RopeCase = collections.namedtuple("RopeCase", "B S H G copies")   # copies: "all" (qt | kt | vt), "none", "kt"
ROPE_FWD_CASES = [RopeCase(1, 1, 2, 1, "all"), RopeCase(2, 63, 4, 2, "none"), RopeCase(2, 64, 12, 2, "kt"), RopeCase(1, 65, 28, 4, "all"),
                  RopeCase(2, 100, 4, 2, "all"), RopeCase(1, 65, 2, 1, "none")]


def rope_fwd_inputs(c):
    M, LD = c.B * c.S, (c.H + 2 * c.G) * HD
    g = gen(c.B, c.S, c.H, c.G, 3)
    qkv = torch.randn(M, LD, generator=g).to(BF)
    assert bool((qkv != 0).all())
    pos = (torch.arange(c.S)[None] + torch.tensor([0, 977])[:c.B, None]).reshape(-1).to(I32)     # batch 0 starts at position 0
    cs, sn = table_f32(pos)
    return dict(qkv=qkv, pos=pos, cos=guarded_rows(cs), sin=guarded_rows(sn), M=M, LD=LD, B=c.B, S=c.S, H=c.H, G=c.G, copies=c.copies,
                Spad=(c.S + 63) // 64 * 64)


def _rot64(x1, x2, cs, sn, inverse=False):
    """(y, slop) of the rotation of the pair halves x1, x2 [..., 64] in float64; slop = |product| + |product| per element"""
    if inverse:
        return (torch.cat([x1 * cs + x2 * sn, x2 * cs - x1 * sn], -1),
                torch.cat([(x1 * cs).abs() + (x2 * sn).abs(), (x2 * cs).abs() + (x1 * sn).abs()], -1))
    return (torch.cat([x1 * cs - x2 * sn, x2 * cs + x1 * sn], -1),
            torch.cat([(x1 * cs).abs() + (x2 * sn).abs(), (x2 * cs).abs() + (x1 * sn).abs()], -1))


def rope_fwd_reference(d):
    M, H, G = d["M"], d["H"], d["G"]
    x = d["qkv"].to(F64).view(M, H + 2 * G, HD)
    cs, sn = d["cos"][:M].to(F64)[:, None], d["sin"][:M].to(F64)[:, None]
    y, slop = _rot64(x[:, :H + G, :64], x[:, :H + G, 64:], cs, sn)
    E = U * y.abs() + 2.0 ** -22 * slop
    E[d["pos"] == 0] = 0.0                                        # the identity
    normal(y, "rope_fwd")
    return Ref({"qk": (y.reshape(M, -1), E.reshape(M, -1))}, {"v": d["qkv"][:, (H + G) * HD:].contiguous()})


def run_rope_fwd(ops, d, to=None):
    ops, to = _call(ops, to)
    M, LD, B, S, H, G, Spad = (d[k] for k in ("M", "LD", "B", "S", "H", "G", "Spad"))
    want = {"all": (1, 1, 1), "none": (0, 0, 0), "kt": (0, 1, 0)}[d["copies"]]

    def once():
        qkv = to(guarded_rows(d["qkv"]))
        cps = [to(nan(B * n * HD * Spad + GE, dtype=BF)) if w else None for n, w in zip((H, G, G), want)]
        ops.rope_fwd(qkv[:M], to(d["cos"])[:M], to(d["sin"])[:M], *[None if t is None else t[:t.numel() - GE] for t in cps], B, S, H, G)
        qkv, qt, kt, vt = _back(qkv, *cps)
        assert untouched(qkv[M:]), "rope_fwd: rows past M of qkv were written"
        out = {"qkv": qkv[:M].contiguous()}
        for name, t, n in (("qt", qt, H), ("kt", kt, G), ("vt", vt, G)):
            if t is not None:
                assert untouched(t[-GE:]), f"rope_fwd: {name} was written behind its last head"
                out[name] = t[:-GE].view(B, n, HD, Spad)
        return out

    out = twice(once, "rope_fwd")
    q4 = out["qkv"].view(B, S, H + 2 * G, HD)
    same_bits(out["qkv"][d["pos"] == 0][:, :(H + G) * HD], d["qkv"][d["pos"] == 0][:, :(H + G) * HD].contiguous(), "rope_fwd at pos = 0 (the identity)")
    for name, lo, n in (("qt", 0, H), ("kt", H, G), ("vt", H + G, G)):
        if name in out:
            exp = torch.zeros(B, n, HD, Spad, dtype=BF)
            exp[..., :S] = q4[:, :, lo:lo + n].permute(0, 2, 3, 1)
            same_bits(out[name], exp, f"rope_fwd {name} against the transpose of the in-place result (+0 in the pad columns)")
    return {"qk": out["qkv"][:, :(H + G) * HD].contiguous(), "v": out["qkv"][:, (H + G) * HD:].contiguous()}


# ================================================================================================ rope_bwd
RopeBwdCase = collections.namedtuple("RopeBwdCase", "H G M profile")
ROPE_BWD_GEOMETRIES = [(2, 1), (4, 1), (10, 2), (16, 2), (28, 4), (4, 4), (12, 2)]
ROPE_BWD_CASES = [RopeBwdCase(H, G, M, p) for H, G in ROPE_BWD_GEOMETRIES for M in (1, 7, 23) for p in ("n01", "exact")]


def dkv_hpb(rep):
    """TASU_ATTN_DKV_HPB: query heads summed per partial by the dK / dV kernel"""
    return 3 if rep % 3 == 0 else (2 if rep % 2 == 0 else 1)


def thread_map(H, G):
    """(units per token, tokens per block, threads per token, passes of the unit loop) of rope_bwd_kernel"""
    upt = (H + 2 * G) * 8
    tpb = 256 // upt if upt <= 128 else 1
    tpt = 256 // tpb
    return upt, tpb, tpt, cdiv(upt, tpt)


def rope_bwd_inputs(c):
    H, G, M = c.H, c.G, c.M
    LD = (H + 2 * G) * HD
    npg = (H // G) // dkv_hpb(H // G)
    np_ = H // dkv_hpb(H // G)
    g = gen(H, G, M, 5)
    if c.profile == "exact":
        draw = lambda *sh: torch.randint(-8, 9, sh, generator=g).to(F32) / 8
    else:
        draw = lambda *sh: torch.randn(*sh, generator=g)
    dqkv = nan(M, LD, dtype=BF)
    dqkv[:, :H * HD] = draw(M, H * HD).to(BF)                     # dQ; the k and v blocks are outputs
    dk, dv = draw(M, np_ * HD), draw(M, np_ * HD)
    pos = torch.arange(M, dtype=I32)                             # row 0: position 0
    cs, sn = table_f32(pos)
    return dict(dqkv=dqkv, dk=guarded_rows(dk), dv=guarded_rows(dv), cos=guarded_rows(cs), sin=guarded_rows(sn), pos=pos, H=H, G=G, M=M, LD=LD,
                npg=npg, np=np_, profile=c.profile)


def rope_bwd_reference(d):
    H, G, M, npg, np_ = d["H"], d["G"], d["M"], d["npg"], d["np"]
    cs, sn = d["cos"][:M].to(F64)[:, None], d["sin"][:M].to(F64)[:, None]
    dq = d["dqkv"][:, :H * HD].to(F64).view(M, H, HD)
    xq, slop = _rot64(dq[..., :64], dq[..., 64:], cs, sn, inverse=True)
    Eq = U * xq.abs() + 2.0 ** -22 * slop
    pk = d["dk"][:M].to(F64).view(M, G, npg, HD)                 # partial r of group g: (g npg + r) 128 into the token's row
    pv = d["dv"][:M].to(F64).view(M, G, npg, HD)
    assert G * npg == np_
    yk, Sk = pk.sum(2), (npg - 1) * e * pk.abs().sum(2)
    xk, slopk = _rot64(yk[..., :64], yk[..., 64:], cs, sn, inverse=True)
    S1, S2 = Sk[..., :64], Sk[..., 64:]
    Ek = U * xk.abs() + torch.cat([cs.abs() * S1 + sn.abs() * S2, cs.abs() * S2 + sn.abs() * S1], -1) + 2.0 ** -22 * slopk
    yv = pv.sum(2)
    Ev = U * yv.abs() + (npg - 1) * e * pv.abs().sum(2)
    if d["profile"] == "exact":                                  # every sum exact in fp32, every result at pos = 0 and every v a bf16 value
        Ev = torch.zeros_like(Ev)
        assert torch.equal(bf16r(yv), yv)
        z = d["pos"] == 0
        Eq[z], Ek[z] = 0.0, 0.0
    ref = torch.cat([xq, xk, yv], 1).reshape(M, -1)
    return Ref({"dqkv": (normal(ref, "rope_bwd"), torch.cat([Eq, Ek, Ev], 1).reshape(M, -1))}, {})


def run_rope_bwd(ops, d, to=None):
    ops, to = _call(ops, to)
    M, H, G = d["M"], d["H"], d["G"]

    def once():
        dqkv = to(guarded_rows(d["dqkv"]))
        dk, dv = to(d["dk"]), to(d["dv"])
        ops.rope_bwd(dqkv[:M], dk, dv, to(d["cos"])[:M], to(d["sin"])[:M], 1, M, H, G)
        dqkv, dk, dv = _back(dqkv, dk, dv)
        assert untouched(dqkv[M:]), "rope_bwd: rows past M of dqkv were written"
        same_bits(dk, d["dk"], "rope_bwd: the dK partials (an input)")
        same_bits(dv, d["dv"], "rope_bwd: the dV partials (an input)")
        return {"dqkv": dqkv[:M].contiguous()}

    return twice(once, "rope_bwd")


# ================================================================================================ SiLU, ReLU, SwiGLU
BIG_UNARY = 2048 * 256 * 8 + 8 + 3                                # the grid-stride loop's second pass is its last vector, + the n & 7 tail
BIG_SWIGLU_I = 8 * (2048 * 256 + 1)
BIG_CAST = 2048 * 256 * 4 + 4 + 3
UnaryCase = collections.namedtuple("UnaryCase", "op n")
UNARY_N = (1, 7, 8, 9, 1003, BIG_UNARY)
UNARY_CASES = [UnaryCase(op, n) for op in ("silu_fwd", "silu_bwd", "relu_fwd", "relu_bwd") for n in UNARY_N]
SwigluCase = collections.namedtuple("SwigluCase", "op M I")
SWIGLU_SHAPES = ((1, 8), (3, 24), (77, 512), (1, BIG_SWIGLU_I))
SWIGLU_CASES = [SwigluCase(op, M, I) for op in ("swiglu_fwd", "swiglu_bwd") for M, I in SWIGLU_SHAPES]

EDGE_G = [0.0, -0.0, 2.0 ** -20, -2.0 ** -20, 1.0, -1.0, -1.28125, 5.0, -5.0, 20.0, -20.0, 80.0, -80.0]
EDGE_TD = [1.0, -1.0, 0.75, -0.75, 2.0 ** -6, -2.0 ** -6]
EDGE_RELU = [0.0, -0.0, 2.0 ** -126, -2.0 ** -126, 1.0, -1.0]


def edge_tuples(with_t, with_d):
    """the edge row: (g, t, d) over the edge sets of the module's header (t / d = 1 where the operation has none), then d = 0 for every g"""
    out = []
    for g in EDGE_G:
        for t in (EDGE_TD if with_t else [1.0]):
            for dd in (EDGE_TD if with_d else [1.0]):
                if with_t and with_d and g == -G_MAX and abs(t) == 2.0 ** -6 and abs(dd) == 2.0 ** -6:
                    continue                                     # d t sg is an fp32 subnormal
                out.append((g, t, dd))
    if with_d:
        out += [(g, 0.75, 0.0) for g in EDGE_G]
    return out


def _put_edge(flat_g, flat_t, flat_d, with_t, with_d):
    """overwrite the tail of the flat element order with the edge tuples: all of them where they fit into half the elements,
    else an even stride through the list over at most half the elements (the rest keeps its N(0, 1) values)"""
    ed = edge_tuples(with_t, with_d)
    k = min(len(ed), flat_g.numel() // 2)
    ed = ed if k == len(ed) else [ed[i * len(ed) // k] for i in range(k)]
    if k == 0:
        return
    flat_g[-k:] = torch.tensor([v[0] for v in ed]).to(BF)
    if flat_t is not None:
        flat_t[-k:] = torch.tensor([v[1] for v in ed]).to(BF)
    if flat_d is not None:
        flat_d[-k:] = torch.tensor([v[2] for v in ed]).to(BF)


def unary_inputs(c):
    n = c.n
    g = gen(n, len(c.op), 7)
    x = (torch.randn(n, generator=g) * 2).to(BF)
    dy = torch.randn(n, generator=g).to(BF) if c.op.endswith("bwd") else None
    if c.op.startswith("relu"):
        k = min(n, len(EDGE_RELU))
        x[n - k:] = torch.tensor(EDGE_RELU[:k]).to(BF)
    else:
        _put_edge(x, None, dy, False, dy is not None)
    assert float(x.float().abs().max()) <= G_MAX
    return dict(op=c.op, n=n, x=guarded_flat(x), dy=None if dy is None else guarded_flat(dy))


def _sig(g):
    sg = 1.0 / (1.0 + torch.exp(-g))
    return sg, 1.0 + g * (1.0 - sg), (2 * g.abs() + 6) * e


def _dgate(dd, t, g):
    """(dg, E_dg) of dg = d t sg f (gemm_ref64's dswiglu bound)"""
    sg, f, a1 = _sig(g)
    dg = dd * t * sg * f
    Ef = g.abs() * (sg * a1 + e) + 2 * e * (1.0 + g.abs() * (1.0 - sg))
    return dg, U * dg.abs() + (dd * t).abs() * sg * (a1 * f.abs() + Ef) + 4 * e * dg.abs()


def unary_reference(d):
    n, op = d["n"], d["op"]
    x = d["x"][:n].to(F64)[None]
    if op == "silu_fwd":
        sg, _, a1 = _sig(x)
        y = x * sg
        return Ref({"y": (normal(y, op, ACT_FLOOR), (U + a1) * (1 + U) * y.abs())}, {})
    if op == "silu_bwd":
        dx, E = _dgate(d["dy"][:n].to(F64)[None], torch.ones_like(x), x)
        return Ref({"y": (normal(dx, op, ACT_FLOOR), E)}, {})
    if op == "relu_fwd":
        return Ref({"y": (x.clamp_min(0.0), torch.zeros_like(x))}, {})
    dy = d["dy"][:n]
    return Ref({}, {"y": torch.where(d["x"][:n].to(F64) > 0, dy, torch.zeros_like(dy))[None]})


def run_unary(ops, d, to=None, again=True):
    ops, to = _call(ops, to)
    n, op = d["n"], d["op"]

    def once():
        y = to(nan(n + GE, dtype=BF))
        x = to(d["x"])
        if op.endswith("bwd"):
            getattr(ops, op)(to(d["dy"])[:n], x[:n], y[:n])
        else:
            getattr(ops, op)(x[:n], y[:n])
        (y,) = _back(y)
        assert untouched(y[n:]), f"{op}: elements past n were written"
        return {"y": y[None, :n]}

    return twice(once, op, again)


def swiglu_inputs(c):
    M, I = c.M, c.I
    g = gen(M, I % 100003, len(c.op), 9)
    gate, up = (torch.randn(M, I, generator=g) * 2).to(BF), (torch.randn(M, I, generator=g) * 2).to(BF)
    dact = torch.randn(M, I, generator=g).to(BF) if c.op == "swiglu_bwd" else None
    _put_edge(gate.view(-1), up.view(-1), None if dact is None else dact.view(-1), True, dact is not None)
    assert float(gate.float().abs().max()) <= G_MAX
    return dict(op=c.op, M=M, I=I, gu=guarded_rows(torch.cat([gate, up], 1), 1), dact=None if dact is None else guarded_rows(dact, 1))


def swiglu_reference(d, plain=False):
    """plain: silu(g) t alone, without the one-right-answer elements (what an autograd formulation gives)"""
    M, I = d["M"], d["I"]
    g, t = d["gu"][:M, :I].to(F64), d["gu"][:M, I:].to(F64)
    sg, _, a1 = _sig(g)
    if d["op"] == "swiglu_fwd":
        s = g * sg
        y = s * t
        if plain:
            return y
        E = (2 * U + U * U + a1 + 2 * e) * (1 + U) * y.abs()
        # where every value within 4 a1 of silu(g) rounds to ONE bf16 value sb, the kernel's intermediate is sb, its fp32 product
        # sb t (16 significant bits) is exact and the result has one right answer: bf16(sb t)
        sb = bf16r(normal(s, "silu", ACT_FLOOR))
        decided = (bf16r(s * (1 + 4 * a1)) == sb) & (bf16r(s * (1 - 4 * a1)) == sb)
        y, E = torch.where(decided, bf16r(sb * t), y), torch.where(decided, torch.zeros_like(E), E)
        return Ref({"act": (normal(y, "swiglu_fwd", ACT_FLOOR), E)}, {})
    dd = d["dact"][:M].to(F64)
    dg, Edg = _dgate(dd, t, g)
    du = dd * g * sg
    return Ref({"dgu": (normal(torch.cat([dg, du], 1), "swiglu_bwd", ACT_FLOOR), torch.cat([Edg, (U + a1 + 4 * e) * du.abs()], 1))}, {})


def run_swiglu(ops, d, to=None, again=True):
    ops, to = _call(ops, to)
    M, I = d["M"], d["I"]

    def once():
        gu = to(d["gu"])
        if d["op"] == "swiglu_fwd":
            act = to(nan(M + 1, I, dtype=BF))
            ops.swiglu_fwd(gu[:M], act[:M], M, I)
            (act,) = _back(act)
            assert untouched(act[M:]), "swiglu_fwd: rows past M were written"
            return {"act": act[:M]}
        dgu = to(nan(M + 1, 2 * I, dtype=BF))
        ops.swiglu_bwd(to(d["dact"])[:M], gu[:M], dgu[:M], M, I)
        (dgu,) = _back(dgu)
        assert untouched(dgu[M:]), "swiglu_bwd: rows past M were written"
        return {"dgu": dgu[:M]}

    return twice(once, d["op"], again)


# ================================================================================================ cast
CastCase = collections.namedtuple("CastCase", "n")
CAST_CASES = [CastCase(n) for n in (1, 3, 4, 5, 1003, BIG_CAST)]


def cast_bits(x):
    """fp32 -> the nearest bf16, ties to even, by integer arithmetic on the fp32 bits (finite inputs)"""
    b = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = (b + 0x7FFF + ((b >> 16) & 1)) >> 16
    return (r - ((r >> 15) << 16)).to(torch.int16).view(BF)      # the 16 bits as a signed integer


def cast_edges():
    """fp32 bit patterns: exact ties with an even and an odd kept bit, one fp32 ulp either side, both signs; the largest finite
    bf16 (0x7F7F) and what still rounds to it (nothing below the last tie 0x7F7F8000 may become inf); +-0"""
    out = []
    for hi in (0x3F80, 0x3F81, 0x4049, 0x40FE, 0x0080, 0x7F00):   # even, odd, odd, even kept bits; the smallest normal; a large binade
        for lo in (0x8000, 0x7FFF, 0x8001, 0x0001, 0xFFFF):
            for sign in (0, 0x8000):
                out.append(((hi | sign) << 16) | lo)
    for lo in (0x0000, 0x0001, 0x7FFF):
        out += [(0x7F7F << 16) | lo, (0xFF7F << 16) | lo]
    out += [0x00000000, 0x80000000, (0x7F7E << 16) | 0x8000, (0x7F7E << 16) | 0x8001]
    t = torch.tensor(out, dtype=torch.int64)
    return (t - ((t >> 31) << 32)).to(torch.int32).view(F32)


def cast_inputs(c):
    n = c.n
    x = torch.randn(n, generator=gen(n, 13))
    ed = cast_edges()[:n]
    x[n - ed.numel():] = ed
    assert bool(torch.isfinite(x).all())
    return dict(n=n, x=guarded_flat(x))


def cast_reference(d):
    return Ref({}, {"y": cast_bits(d["x"][:d["n"]])})


def run_cast(ops, d, to=None, again=True):
    ops, to = _call(ops, to)
    n = d["n"]

    def once():
        y = to(nan(n + GE, dtype=BF))
        ops.cast_bf16(to(d["x"])[:n], y[:n])
        (y,) = _back(y)
        assert untouched(y[n:]), "cast_f32_bf16: elements past n were written"
        return {"y": y[:n]}

    return twice(once, "cast_f32_bf16", again)


# ================================================================================================ sinusoid_pe
PeCase = collections.namedtuple("PeCase", "B T D profile")        # profile: n01 | zero (x = 0) | same (every batch holds batch 0's x)
PE_CASES = [PeCase(B, T, D, p) for B, T, D in ((1, 1, 4), (2, 37, 80), (2, 5, 560)) for p in ("n01", "zero", "same") if p != "same" or B > 1] + \
           [PeCase(1, 504, 560, "enc"), PeCase(1, 504, 560, "zero")]   # the encoder's rows, scale = sqrt(512): with x, and the PE alone


def pe_inputs(c):
    B, T, D = c.B, c.T, c.D
    x = torch.randn(B, T, D, generator=gen(B, T, D, 17))
    if c.profile == "zero":
        x.zero_()
    if c.profile == "same":
        x[1:] = x[0]
    scale = math.sqrt(512.0) if T == 504 else math.sqrt(float(D))
    return dict(B=B, T=T, D=D, x=guarded_flat(x), scale=scale, profile=c.profile)


def pe_angles(T, D):
    half = D // 2
    arg = torch.arange(half, dtype=F64) * (math.log(10000.0) / (half - 1))
    return torch.arange(1, T + 1, dtype=F64)[:, None] * torch.exp(-arg)[None], arg


def pe_reference(d, Q=None, X=None):
    Q, X = SINCOS_E if Q is None else Q, EXP_E if X is None else X
    B, T, D = d["B"], d["T"], d["D"]
    ang, arg = pe_angles(T, D)
    pe = torch.cat([ang.sin(), ang.cos()], 1)
    Ea = e * (ang.abs() * (2 * arg[None] + X + 4) + Q)
    Ea[:, 0] = e * Q                                             # k = 0: the integer t + 1
    xs = d["x"][:B * T * D].to(F64).view(B, T, D) * float(torch.tensor(d["scale"], dtype=F32))    # the fp32 value the kernel is passed
    y = xs + pe[None]
    E = torch.cat([Ea, Ea], 1)[None] + 2 * e * (xs.abs() + y.abs())
    return Ref({"y": (normal(y, "sinusoid_pe").reshape(B * T, D), E.reshape(B * T, D))}, {})


def run_pe(ops, d, to=None):
    ops, to = _call(ops, to)
    B, T, D = d["B"], d["T"], d["D"]
    n = B * T * D

    def once():
        y = to(nan(n + GE))
        ops.sinusoid_pe(to(d["x"])[:n].view(B * T, D), y[:n].view(B * T, D), B, T, D, d["scale"])
        (y,) = _back(y)
        assert untouched(y[n:]), "sinusoid_pe: elements past B T D were written"
        return {"y": y[:n].view(B * T, D)}

    out = twice(once, "sinusoid_pe")
    if d["profile"] == "same":                                   # the PE depends on t only
        y3 = out["y"].view(B, T, D)
        for b in range(1, B):
            same_bits(y3[b].contiguous(), y3[0].contiguous(), f"sinusoid_pe batch {b} against batch 0 (equal x)")
    return out


# ================================================================================================ FSMN
FsmnCase = collections.namedtuple("FsmnCase", "D ks T acc profile")
FSMN_ROUTES = [(8, 11), (512, 11), (520, 11), (84, 11), (16, 4), (16, 1)]     # vector kernel: D % 8 == 0 and ks = 11 (520: a second c += 512 trip)
FSMN_T = (1, 16, 19, 37)
FSMN_CASES = [FsmnCase(D, ks, T, acc, p) for D, ks in FSMN_ROUTES for T in FSMN_T for acc in (0, 1) for p in ("exact", "n01")]


def fsmn_lens(T):
    """one batch: len = T, 0, 1, 5 (shorter than left = 5 + the frame itself), 16, 17, T - 1 -- those that fit under T"""
    return [min(max(v, 0), T) for v in (T, 0, 1, 5, 16, 17, T - 1)]


def fsmn_route(D, ks, ldv):
    return "vector" if D % 8 == 0 and ldv % 8 == 0 and ks == 11 else "scalar"


def fsmn_inputs(c):
    D, ks, T = c.D, c.ks, c.T
    lens = torch.tensor(fsmn_lens(T), dtype=I32)
    B, ldv = lens.numel(), 3 * D
    g = gen(D, ks, T, c.acc, 19)
    if c.profile == "exact":
        v = torch.randint(-4, 5, (B, T, D), generator=g).to(F32)
        w = torch.randint(-4, 5, (D, ks), generator=g).to(F32) / 8
        out0 = torch.randint(-64, 65, (B * T, D), generator=g).to(F32) / 8
    else:
        v, w, out0 = torch.randn(B, T, D, generator=g), torch.randn(D, ks, generator=g) * 0.2, torch.randn(B * T, D, generator=g)
    buf = nan(B, T, ldv, dtype=BF)                               # v: the last third of every row; NaN in the other columns and in frames t >= len
    live = torch.arange(T)[None] < lens[:, None]
    buf[..., 2 * D:] = torch.where(live[..., None], v.to(BF), torch.full((), NAN, dtype=BF))
    return dict(D=D, ks=ks, T=T, B=B, ldv=ldv, lens=lens, vbuf=buf.view(B * T, ldv), w=guarded_flat(w), out0=out0, acc=c.acc, profile=c.profile,
                live=live)


def fsmn_sums(d):
    """(result without out0, sum of |terms|) float64 [B, T, D]: shifted copies of the masked v, one per tap"""
    D, ks, T, B = d["D"], d["ks"], d["T"], d["B"]
    left = (ks - 1) // 2
    live = d["live"]
    v = d["vbuf"].view(B, T, -1)[..., 2 * D:].to(F64)
    vm = torch.where(live[..., None], v, torch.zeros_like(v))
    w = d["w"][:D * ks].to(F64).view(D, ks)
    pad = torch.zeros(B, T + 2 * ks, D, dtype=F64)
    pad[:, ks:ks + T] = vm
    r, a = torch.zeros(B, T, D, dtype=F64), torch.zeros(B, T, D, dtype=F64)
    for j in range(ks):
        term = w[:, j][None, None] * pad[:, ks + j - left:ks + j - left + T]
        r, a = r + term, a + term.abs()
    r, a = r + vm, a + vm.abs()
    z = torch.zeros_like(r)
    return torch.where(live[..., None], r, z), torch.where(live[..., None], a, z)     # frames behind len: +0


def fsmn_reference(d):
    B, T, D, ks = d["B"], d["T"], d["D"], d["ks"]
    r, a = fsmn_sums(d)
    r, a = r.reshape(B * T, D), a.reshape(B * T, D)
    lv = d["live"].reshape(B * T, 1).to(F64)
    out0 = d["out0"].to(F64)
    res = out0 + r if d["acc"] else r
    if d["profile"] == "exact":
        assert torch.equal(fl32(res), res)
        return Ref({}, {"out": res.to(F32)})
    E = (ks + 1) * e * a + (e * (out0.abs() + res.abs()) * lv if d["acc"] else 0.0)
    return Ref({"out": (normal(res, "fsmn_fwd"), E)}, {})


def run_fsmn(ops, d, to=None):
    ops, to = _call(ops, to)
    B, T, D, ks = d["B"], d["T"], d["D"], d["ks"]
    R = B * T

    def once():
        out = nan(R + GUARD, D)
        if d["acc"]:
            out[:R] = d["out0"]
        out = to(out)
        ops.fsmn_fwd(to(d["vbuf"])[:, 2 * D:], d["ldv"], to(d["w"])[:D * ks].view(D, ks), to(d["lens"]), out[:R], B, T, D, ks, bool(d["acc"]))
        (out,) = _back(out)
        assert untouched(out[R:]), "fsmn_fwd: rows past B T were written"
        return {"out": out[:R]}

    return twice(once, "fsmn_fwd")


FsmnLnCase = collections.namedtuple("FsmnLnCase", "T ldy profile")
FSMN_LN_CASES = [FsmnLnCase(19, 520, "n01"), FsmnLnCase(19, 512, "exact")]
EPS_LN = 1e-5


def fsmn_ln_inputs(c):
    d = fsmn_inputs(FsmnCase(512, 11, c.T, 1, c.profile))
    g = gen(c.T, c.ldy, 23)
    d.update(ldy=c.ldy, gamma=guarded_flat(1 + 0.1 * torch.randn(512, generator=g)), beta=guarded_flat(0.1 * torch.randn(512, generator=g)))
    return d


def run_fsmn_ln(ops, d, to=None):
    """x and xn of fsmn_ln_fwd, and x of fsmn_fwd(accumulate) through the same ops"""
    ops, to = _call(ops, to)
    B, T, D, ks, ldy = d["B"], d["T"], d["D"], d["ks"], d["ldy"]
    R = B * T

    def once():
        x = nan(R + GUARD, D)
        x[:R] = d["out0"]
        x, xn = to(x), to(nan(R + GUARD, ldy, dtype=BF))
        ops.fsmn_ln_fwd(to(d["vbuf"])[:, 2 * D:], d["ldv"], to(d["w"])[:D * ks].view(D, ks), to(d["lens"]), x[:R], to(d["gamma"])[:D], to(d["beta"])[:D],
                        xn[:R], B, T, D, ks, EPS_LN)
        x, xn = _back(x, xn)
        assert untouched(x[R:]) and untouched(xn[R:]), "fsmn_ln_fwd: rows past B T were written"
        return {"x": x[:R], "xn": xn[:R]}

    out = twice(once, "fsmn_ln_fwd")
    same_bits(out["x"], run_fsmn(ops, d, to)["out"], "fsmn_ln_fwd x against fsmn_fwd(accumulate)")
    return out


def fsmn_ln_reference(d, x_got):
    """row_ref64's LayerNorm reference of the x the call left behind (pad columns D .. ldy - 1: exactly 0)"""
    R, D = d["B"] * d["T"], d["D"]
    assert not bool(torch.isnan(x_got).any()), "fsmn_ln_fwd: NaN in x"
    ref = ln_reference(dict(x=x_got, gamma=d["gamma"][:D], beta=d["beta"][:D], R=R, D=D, ldy=d["ldy"], f32=0, stats=0))
    return Ref({"xn": ref.tol["y"]}, {})
