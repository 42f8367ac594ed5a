"""The rotary, pointwise and encoder-memory kernels against float64 references, element by element (tests/point_ref64.py; its own
checks: tests/test_point_ref64_cpu.py), through HipOps like tests/test_gpu_ops.py:

  csrc/rope.hip         tasu_rope_table (theta 1e6 and 1e4; positions 0 .. 32767, a repeated position, M no multiple of 4),
                        tasu_rope_fwd (S = 1, 63, 64, 65, 100; H / G = 2/1, 4/2, 12/2, 28/4; all three transposed copies, none, kt
                        alone), tasu_rope_bwd (the thread maps of H / G = 2/1, 4/1, 10/2, 16/2, 28/4, 4/4, 12/2 at M = 1, 7, 23)
  csrc/elementwise.hip  tasu_silu_fwd/bwd, tasu_relu_fwd/bwd (n = 1, 7, 8, 9, 1003 and the grid-stride loop's second pass),
                        tasu_swiglu_fwd/bwd ((1, 8), (3, 24), (77, 512), one row of 2048 x 256 + 1 vectors), tasu_cast_f32_bf16
  csrc/encoder_aux.hip  tasu_sinusoid_pe, tasu_fsmn_fwd (vector kernel at D = 8, 512, 520; scalar kernel at D = 84, at ks = 4 and
                        ks = 1; seven lengths per batch, T = 1, 16, 19, 37; accumulate on and off), tasu_fsmn_ln_fwd

Every output starts as NaN with guard rows / elements that must keep their bits; every operand has NaN outside what the kernel is
owed (for the FSMN: every frame behind `lens` and every column beside v).  Every case runs twice and must give equal bits.  Every
output within 1.0 x E of the float64 value on every element, the reference's value where E = 0, its bits on the exact profiles.
Second check, bf16 outputs: rms(err / (u |ref|)) over the elements whose fp32 allowance is at most a tenth of u |ref| (cases with
at least 4096 of them) at most 1.5 x the torch double's on the same inputs (F64RATIO lines).  Bit identities: tasu_gemm_qkv_rope =
tasu_gemm_nt_bf16 (bias) + tasu_rope_fwd, tasu_gemm_dswiglu's dgu = tasu_swiglu_bwd of its dact.  Refusals leave the outputs
untouched, among them the pointer alignments the 16-byte (cast output: 8-byte) vector accesses need.

Measured on MI355X (205 tests, 4.8 s for the file; the slowest test, swiglu_bwd on 4194312 elements, 1.3 s): every check passes.
Largest |err| / E per operation (the F64WORST lines):
    rope_table 0.336   rope_fwd 0.996   rope_bwd 0.996   silu_fwd 0.992   silu_bwd 0.996   swiglu_fwd 0.910   swiglu_bwd 0.996
    sinusoid_pe 0.503   fsmn_fwd vector 0.413  scalar 0.584   fsmn_ln_fwd 0.995   relu_fwd, relu_bwd, cast_f32_bf16: exact
Largest rms ratio, kernel / double: 1.000 for rope_fwd qk, rope_bwd dqkv, silu_fwd, silu_bwd, swiglu_bwd dgu, fsmn_ln_fwd xn
(swiglu_fwd's eligible elements are the ones with one right answer: exact on both sides, no ratio).
Library functions (the F64LIB lines): sincosf on the integer angles 0 .. 32767: 0.82 e = 0.41 ulp against the 4 e = 2 ulp allowed;
sinf / cosf on the integers 1 .. 504: 0.89 e = 0.44 ulp against 4 e; the PE's chain (logf, the division, two products, expf) at
|ang| >= 64: 3.38 e |ang| against 2 arg + 6.  powf: the table's chain at |ang| >= 64 measured 8.65 e |ang| (theta 1e6; 7.08 at
1e4), the division and the product being 2 of it: powf is up to 3.3 ulp off, and the 2 ulp (P = 4) the project grants rsqrtf gave
1.71 x E on this correct kernel.  P is therefore 32 e = 16 ulp, what the device library's pow is specified to (OpenCL full
profile), for powf only; the worst |err| / E is then 0.336.  Scratch mutants of three kernels fail this file
where they should.  No kernel needed a fix; the entry points of elementwise.hip and rope.hip gained the alignment checks tested
at the end of this file, and no caller in the project trips them."""
import math

import pytest
import torch

import gemm_ref64 as G
import point_ref64 as P
from fake_ops import FakeOps

pytestmark = pytest.mark.gpu
F64, F32, BF, I32 = torch.float64, torch.float32, torch.bfloat16, torch.int32


@pytest.fixture(scope="module")
def hip():
    from ps_slm_amd.ops import HipOps
    return HipOps()


@pytest.fixture(scope="module")
def fake():
    return FakeOps()


def cuda(t):
    return t.cuda()


def nan(*shape, dtype=F32):
    return P.nan(*shape, dtype=dtype).cuda()


_worst, _ratios = {}, {}


def hold(op, case, got, ref, double=None):
    """one run against its Ref: the element-wise check, then the rms ratio of every bf16 output against the double's"""
    what = f"{op} {P.case_id(case)}"
    w = P.check(got, ref, what)
    _worst[op] = max(_worst.get(op, 0.0), w)
    print(f"F64WORST {what} |err| / E {w:.3f} (largest so far for {op}: {_worst[op]:.3f})")
    for name, (want, E) in ref.tol.items():
        if double is None or got[name].dtype != BF:
            continue
        k, n = P.rms_stat(got[name], want, E)
        dbl, _ = P.rms_stat(double[name], want, E)
        if n < 4096 or (k == 0.0 and dbl == 0.0):                 # (both exact on every eligible element: nothing to compare)
            continue
        ratio = k / dbl if dbl > 0 else 0.0
        _ratios[(op, name)] = max(_ratios.get((op, name), 0.0), ratio)
        print(f"F64RATIO {op} {name} {ratio:.3f} kernel {k:.5f} double {dbl:.5f} over {n} elements {P.case_id(case)} "
              f"(largest so far {_ratios[(op, name)]:.3f})")
        assert k <= P.RMS_RATIO * dbl, (f"{what} {name}: rms {k:.5f} is {ratio:.2f} x the double's {dbl:.5f} (at most {P.RMS_RATIO} x: "
                                        f"a systematic error, not rounding)")


# ------------------------------------------------------------------------------------------------ csrc/rope.hip
@pytest.mark.parametrize("case", P.TABLE_CASES, ids=P.case_id)
def test_rope_table(hip, case):
    d = P.table_inputs(case)
    got = P.run_table(hip, d, cuda)
    ref = P.table_reference(d)
    ang = P.table_angles(d["pos"], d["theta"])
    err = torch.maximum((got["cos"].double() - ref.tol["cos"][0]).abs(), (got["sin"].double() - ref.tol["sin"][0]).abs()) / P.e
    far = ang.abs() >= 64
    far[:, 0] = False
    print(f"F64LIB rope_table theta {case.theta:g}: sincosf on the integer angles of column 0: {float(err[:, 0].max()):.2f} e = "
          f"{float(err[:, 0].max()) / 2:.2f} ulp of 1 (allowed {P.SINCOS_E:g} e); the chain at |ang| >= 64: "
          f"{float((err / ang.abs().clamp_min(1))[far].max()):.2f} e |ang| (allowed {P.POW_E + 2:g}: powf {P.POW_E:g}, the division, the product)")
    hold("rope_table", case, got, ref)


@pytest.mark.parametrize("case", P.ROPE_FWD_CASES, ids=P.case_id)
def test_rope_fwd(hip, fake, case):
    d = P.rope_fwd_inputs(case)
    hold("rope_fwd", case, P.run_rope_fwd(hip, d, cuda), P.rope_fwd_reference(d), P.run_rope_fwd(fake, d))


@pytest.mark.parametrize("case", P.ROPE_BWD_CASES, ids=P.case_id)
def test_rope_bwd(hip, fake, case):
    d = P.rope_bwd_inputs(case)
    hold("rope_bwd", case, P.run_rope_bwd(hip, d, cuda), P.rope_bwd_reference(d), P.run_rope_bwd(fake, d))


@pytest.mark.parametrize("case", [c for c in G.QKV_CASES if c.bias], ids=G.case_id)
def test_qkv_rope_epilogue_has_the_bits_of_gemm_then_rope_fwd(hip, case):
    """common.h: tasu_rope_fwd and the tasu_gemm_qkv_rope epilogue share rope_pair_f -- the same bits"""
    c = case
    d = G.make_inputs(c, "exact")
    a, w, bias, cs, sn = (d[k].cuda() for k in ("a", "w", "bias", "cos", "sin"))
    fused, two = nan(c.M + 2, c.N, dtype=BF), nan(c.M + 2, c.N, dtype=BF)
    hip.gemm_qkv_rope(a, w, bias, fused, cs, sn, c.M, c.H, c.G, c.K)
    hip.gemm(a, w, two, c.M, c.N, c.K, bias=bias)
    hip.rope_fwd(two, cs, sn, None, None, None, 1, c.M, c.H, c.G)
    torch.cuda.synchronize()
    fused, two = fused.cpu(), two.cpu()
    assert P.untouched(fused[c.M:]) and P.untouched(two[c.M:]) and not bool(torch.isnan(two[:c.M]).any())
    P.same_bits(fused[:c.M], two[:c.M], f"gemm_qkv_rope against gemm + rope_fwd {G.case_id(c)}")


# ------------------------------------------------------------------------------------------------ csrc/elementwise.hip
@pytest.mark.parametrize("case", P.UNARY_CASES, ids=P.case_id)
def test_silu_and_relu(hip, fake, case):
    d = P.unary_inputs(case)
    hold(case.op, case, P.run_unary(hip, d, cuda), P.unary_reference(d), P.run_unary(fake, d, again=False))


@pytest.mark.parametrize("case", P.SWIGLU_CASES, ids=P.case_id)
def test_swiglu(hip, fake, case):
    d = P.swiglu_inputs(case)
    hold(case.op, case, P.run_swiglu(hip, d, cuda), P.swiglu_reference(d), P.run_swiglu(fake, d, again=False))


@pytest.mark.parametrize("case", P.CAST_CASES, ids=P.case_id)
def test_cast_f32_bf16(hip, case):
    d = P.cast_inputs(case)
    hold("cast_f32_bf16", case, P.run_cast(hip, d, cuda), P.cast_reference(d))


def test_cast_serves_an_output_that_is_8_byte_aligned_only(hip):
    d = P.cast_inputs(P.CastCase(1003))
    y = nan(1003 + 4 + P.GE, dtype=BF)
    hip.cast_bf16(d["x"].cuda()[:1003], y[4:1007])
    torch.cuda.synchronize()
    y = y.cpu()
    assert P.untouched(y[:4]) and P.untouched(y[1007:])
    P.same_bits(y[4:1007], P.cast_reference(d).exact["y"], "cast_f32_bf16 into an 8-byte aligned output")


@pytest.mark.parametrize("case", [c for c in G.DSWIGLU_CASES if c.M <= 300], ids=G.case_id)
def test_dswiglu_has_the_bits_of_swiglu_bwd_on_its_dact(hip, case):
    """common.h: tasu_swiglu_bwd and the tasu_gemm_dswiglu epilogue share swiglu_bwd_f -- the same bits"""
    c = case
    d = G.make_inputs(c, "exact")
    a, w, gu = d["a"].cuda(), d["w"].cuda(), d["gu"].cuda()
    dgu, dact, again = nan(c.M + 2, 2 * c.N, dtype=BF), nan(c.M + 2, c.N, dtype=BF), nan(c.M + 2, 2 * c.N, dtype=BF)
    hip.gemm_dswiglu(a, w, gu, dgu, dact, c.M, c.N, c.K)
    hip.swiglu_bwd(dact, gu, again, c.M, c.N)
    torch.cuda.synchronize()
    dgu, again = dgu.cpu(), again.cpu()
    assert P.untouched(dgu[c.M:]) and P.untouched(again[c.M:]) and not bool(torch.isnan(again[:c.M]).any())
    P.same_bits(dgu[:c.M], again[:c.M], f"gemm_dswiglu's dgu against swiglu_bwd of its dact {G.case_id(c)}")


# ------------------------------------------------------------------------------------------------ csrc/encoder_aux.hip
@pytest.mark.parametrize("case", P.PE_CASES, ids=P.case_id)
def test_sinusoid_pe(hip, case):
    d = P.pe_inputs(case)
    got, ref = P.run_pe(hip, d, cuda), P.pe_reference(d)
    if case.profile == "zero":                                   # y is the PE alone
        T, D = case.T, case.D
        ang, _ = P.pe_angles(T, D)
        err = ((got["y"].double() - ref.tol["y"][0]).abs() / P.e).view(case.B, T, 2, D // 2).amax((0, 2))
        far = ang.abs() >= 64
        far[:, 0] = False
        chain = float((err / ang.abs().clamp_min(1))[far].max()) if bool(far.any()) else 0.0
        print(f"F64LIB sinusoid_pe {P.case_id(case)}: sinf / cosf on the integer angles of k = 0: {float(err[:, 0].max()):.2f} e = "
              f"{float(err[:, 0].max()) / 2:.2f} ulp of 1 (allowed {P.SINCOS_E:g} e); the chain at |ang| >= 64: {chain:.2f} e |ang| "
              f"(allowed 2 arg + {P.EXP_E + 4:g}, arg up to {math.log(10000.0):.1f})")
    hold("sinusoid_pe", case, got, ref)


@pytest.mark.parametrize("case", P.FSMN_CASES, ids=P.case_id)
def test_fsmn_fwd(hip, case):
    d = P.fsmn_inputs(case)
    hold(f"fsmn_fwd[{P.fsmn_route(case.D, case.ks, d['ldv'])}]", case, P.run_fsmn(hip, d, cuda), P.fsmn_reference(d))


@pytest.mark.parametrize("case", P.FSMN_LN_CASES, ids=P.case_id)
def test_fsmn_ln_fwd(hip, fake, case):
    d = P.fsmn_ln_inputs(case)
    got, dbl = P.run_fsmn_ln(hip, d, cuda), P.run_fsmn_ln(fake, d)
    if case.profile == "exact":
        P.same_bits(got["x"], P.fsmn_reference(d).exact["out"], "fsmn_ln_fwd x on the exact profile")
    hold("fsmn_ln_fwd", case, {"xn": got["xn"]}, P.fsmn_ln_reference(d, got["x"]), {"xn": dbl["xn"]})


# ------------------------------------------------------------------------------------------------ bad arguments
def refused(call, *outs):
    from ps_slm_amd.ops import TasuOpError
    with pytest.raises(TasuOpError, match="bad argument"):
        call()
    torch.cuda.synchronize()
    for o in outs:
        assert P.untouched(o.cpu()), "a refused call wrote to its output"


def off(t, k):
    """a copy of t whose first element sits k elements behind an allocation's start (the allocator aligns that to 256 bytes)"""
    buf = torch.empty(t.numel() + k + 8, dtype=t.dtype, device="cuda")
    assert buf.data_ptr() % 256 == 0
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def each_misaligned(args, which, k=4):
    """the argument lists with one of the tensors `which` moved k elements off its 16-byte boundary"""
    for i in which:
        yield [off(a, k) if j == i else a for j, a in enumerate(args)], i


def test_rope_refuses_what_it_does_not_serve(hip):
    M, H, G = 4, 4, 2
    LD, Spad = (H + 2 * G) * 128, 64
    pos = torch.arange(M, dtype=I32, device="cuda")
    cs, sn = nan(M, 64), nan(M, 64)
    refused(lambda: hip.rope_table(pos, cs, sn, 64, 1e6), cs, sn)                                                # head_dim != 128
    refused(lambda: hip.rope_table(pos, None, sn, 128, 1e6), sn)
    refused(lambda: hip.rope_table(pos[:0], cs, sn, 128, 1e6), cs, sn)                                           # M = 0
    one, zero = torch.ones(M, 64, device="cuda"), torch.zeros(M, 64, device="cuda")
    qkv = nan(M, LD, dtype=BF)
    qt, kt, vt = nan(H * 128 * Spad, dtype=BF), nan(G * 128 * Spad, dtype=BF), nan(G * 128 * Spad, dtype=BF)
    refused(lambda: hip.rope_fwd(None, one, zero, qt, kt, vt, 1, M, H, G), qt, kt, vt)
    refused(lambda: hip.rope_fwd(qkv, None, zero, qt, kt, vt, 1, M, H, G), qkv, qt, kt, vt)
    refused(lambda: hip.rope_fwd(qkv, one, zero, qt, kt, vt, 1, 0, H, G), qkv, qt, kt, vt)
    for args, i in each_misaligned([qkv, one, zero, qt, kt, vt], (0, 3, 4, 5)):                                  # 16-byte vectors
        args = [a.fill_(P.NAN) if j in (0, 3, 4, 5) else a for j, a in enumerate(args)]
        refused(lambda: hip.rope_fwd(*args, 1, M, H, G), args[0], *args[3:])
    np_ = H // P.dkv_hpb(H // G)
    dqkv, dk, dv = nan(M, LD, dtype=BF), torch.ones(M, np_ * 128, device="cuda"), torch.ones(M, np_ * 128, device="cuda")
    refused(lambda: hip.rope_bwd(dqkv, dk, dv, one, zero, 1, M, 5, 2), dqkv)                                     # H % G
    refused(lambda: hip.rope_bwd(dqkv, None, dv, one, zero, 1, M, H, G), dqkv)
    refused(lambda: hip.rope_bwd(dqkv, dk, dv, one, None, 1, M, H, G), dqkv)
    base = [dqkv, dk, dv, one, zero]
    for i in range(5):                                           # each pointer 8 bytes off a 16-byte boundary: bf16x8 / f32x4 accesses
        args = [off(a, 4 if a.dtype == BF else 2) if j == i else a for j, a in enumerate(base)]
        args[0].fill_(P.NAN)
        refused(lambda: hip.rope_bwd(*args, 1, M, H, G), args[0])


def test_pointwise_refuses_what_it_does_not_serve(hip):
    M, I = 2, 16
    gu, dact = torch.ones(M, 2 * I, dtype=BF, device="cuda"), torch.ones(M, I, dtype=BF, device="cuda")
    act, dgu = nan(M, I, dtype=BF), nan(M, 2 * I, dtype=BF)
    refused(lambda: hip.swiglu_fwd(None, act, M, I), act)
    refused(lambda: hip.swiglu_fwd(gu, None, M, I))
    refused(lambda: hip.swiglu_fwd(gu, act, M, 12), act)                                                         # I % 8
    refused(lambda: hip.swiglu_fwd(gu, act, 0, I), act)
    refused(lambda: hip.swiglu_bwd(dact, gu, dgu, M, 12), dgu)
    refused(lambda: hip.swiglu_bwd(None, gu, dgu, M, I), dgu)
    for args, i in each_misaligned([gu, act], (0, 1)):
        args[1].fill_(P.NAN)
        refused(lambda: hip.swiglu_fwd(*args, M, I), args[1])
    for args, i in each_misaligned([dact, gu, dgu], (0, 1, 2)):
        args[2].fill_(P.NAN)
        refused(lambda: hip.swiglu_bwd(*args, M, I), args[2])
    x, dy, y = torch.ones(40, dtype=BF, device="cuda"), torch.ones(40, dtype=BF, device="cuda"), nan(40, dtype=BF)
    for name in ("silu_fwd", "relu_fwd"):
        op = getattr(hip, name)
        refused(lambda: op(x[:0], y[:0]), y)                                                                     # n = 0
        refused(lambda: op(x, None))
        for args, i in each_misaligned([x, y], (0, 1)):
            args[1].fill_(P.NAN)
            refused(lambda: op(*args), args[1])
    for name in ("silu_bwd", "relu_bwd"):
        op = getattr(hip, name)
        refused(lambda: op(dy[:0], x[:0], y[:0]), y)
        refused(lambda: op(None, x, y), y)
        for args, i in each_misaligned([dy, x, y], (0, 1, 2)):
            args[2].fill_(P.NAN)
            refused(lambda: op(*args), args[2])
    xf = torch.ones(40, device="cuda")
    refused(lambda: hip.cast_bf16(xf[:0], y[:0]), y)
    refused(lambda: hip.cast_bf16(xf, None))
    refused(lambda: hip.cast_bf16(off(xf, 2), y), y)                                                             # f32x4 loads: 16 bytes
    y2 = off(y, 2).fill_(P.NAN)
    refused(lambda: hip.cast_bf16(xf, y2), y2)                                                                   # bf16x4 stores: 8 bytes


def test_sinusoid_pe_refuses_what_it_does_not_serve(hip):
    x, y = torch.ones(2 * 3 * 6, device="cuda"), nan(2 * 3 * 6)
    refused(lambda: hip.sinusoid_pe(x, y, 2, 3, 5, 1.0), y)                                                      # D % 2
    refused(lambda: hip.sinusoid_pe(x, y, 2, 3, 2, 1.0), y)                                                      # D < 4
    refused(lambda: hip.sinusoid_pe(x, y, 2, 0, 6, 1.0), y)                                                      # T = 0
    refused(lambda: hip.sinusoid_pe(None, y, 2, 3, 6, 1.0), y)
