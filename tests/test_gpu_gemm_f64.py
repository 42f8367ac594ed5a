"""The bf16 NT GEMMs of the training step and the prefill against float64 references, element by element (tests/gemm_ref64.py; its
own checks: tests/test_gemm_ref64_cpu.py), through HipOps like tests/test_gpu_ops.py:

  dispatcher        ops.gemm with the workspace: one case or more per TASU_GEMM_PLAN_* value (the 128-row tiles with both widths,
                    the three loader-wave tiles, whole 256 x 256 tiles, the column split over two kernels with either tail,
                    stream-K, the 256 x 192 split-K with its last arriver)
  named kernels     ops.gemm_on: pp256 / pipe128 / pipe192 / pipe96 x the three public modes x the store paths of store_tile
                    (interior, edge, ldc no multiple of 8 / 4, C and R 8 bytes off a 16-byte boundary, N no multiple of 4), lda = ldb > K
  stream-K          ops.gemm_streamk at shapes chosen from the host schedule: whole / producer / owner items, 4 and 16 ranges per
                    tile, snapped range ends, more than one round with and without whole tiles behind the cut ones
  slabs             ops.gemm_splitk / gemm_slabs / sum_slabs: ksplit 1, 3, 5, 16; every slab, then the sum
  fused epilogues   gate|up + SwiGLU on each of its four routes, q|k|v + bias + RoPE at H / G = 2/1, 12/2, 28/4, dswiglu, bias + ReLU

The exact profile's BITS for every linear output (all fp32-mode results and every slab included), 1.0 x E for SwiGLU, bias + RoPE
and dswiglu on exact accumulations; on the N(0, 1) profile (K <= 512) E = u |c| + the rigorous fp32 allowance per element and
rms(err / (u |c|)) at most 1.5 x the torch double's.  Operand guards are NaN; every output buffer holds a sentinel pattern before
the launch and must keep it, bit for bit, outside [M, N].  Cases that go through the workspace run twice (equal bits) and leave
its flag and counter words zero.  The launch is the plan: every dispatched case launches as many GEMM kernels
(tasu_gemm_launch_count) as the plan the library names for it (tasu_gemm_plan, tasu_gemm_gate_up_plan) stands for -- two for a
column split, else one -- and no epilogue option (ReLU, act's leading dimension) outlives the call it was given to.

Measured on an MI355X (the F64RATIO / F64EXACT / F64N01 lines this file prints): 118 tests, 12 s (the four option tests came later).  Every exact-bits check
holds on every route.  Largest kernel rms / double rms over the 73 statistics taken: 1.000 (every family and output).  Largest
|err| / E per family, equal to the double's to three digits: exact accumulations -- SwiGLU 0.961, bias + RoPE 0.996, dswiglu 0.996;
N(0, 1) -- gemm 0.991, bias + ReLU 0.983, gate|up 0.985, q|k|v 0.989, dswiglu (dact) 0.985, split-K 0.981, slabs 0.967.  No kernel
needed a fix."""
import pytest
import torch

import gemm_ref64 as G
from fake_ops import FakeOps

pytestmark = pytest.mark.gpu
HD = G.HD
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64


@pytest.fixture(scope="module")
def hip():
    from ps_slm_amd.ops import HipOps
    return HipOps()


@pytest.fixture(scope="module")
def fake():
    return FakeOps()


def dev(t):
    return None if t is None else t.cuda()


_ratios, _worst = {}, {}


def report(family, name, kernel, double, case):
    ratio = kernel / double if double > 0 else 0.0
    _ratios[(family, name)] = max(_ratios.get((family, name), 0.0), ratio)
    print(f"F64RATIO {family} {name} {ratio:.3f} kernel {kernel:.5f} double {double:.5f} {case} (largest so far {_ratios[(family, name)]:.3f})")
    assert kernel <= G.RMS_RATIO * double, (f"{family} {name} {case}: rms {kernel:.5f} is {ratio:.2f} x the double's {double:.5f} "
                                            f"(at most {G.RMS_RATIO} x: a systematic error, not rounding)")


def planned_launches(hip, c):
    """GEMM kernel launches behind the case's call, from the plan the LIBRARY names for it (which must be the list's); None where
    the case is not dispatched"""
    if c.op == "swiglu":
        assert hip.lib.tasu_gemm_gate_up_plan(c.M, c.N, c.K, 1) == G.GU_PLAN[c.via], G.case_id(c)
        return 2 if c.via == "pp+pipe" else 1
    if c.plan is None:
        return None
    assert hip.lib.tasu_gemm_plan(c.M, c.N, c.K, c.mode if c.op == "plain" else 0, 1) == c.plan, G.case_id(c)
    return 2 if c.plan in (G.PP_P128, G.PP_P192) else 1


def run_case(hip, c, d):
    """One case through HipOps: name -> CPU result [M, N] (the names of gemm_ref64.reference).  Operands carry their NaN guards,
    every output starts as the sentinel pattern; OutBuf.check holds the guard rows, columns and margins to it."""
    M, N, K = c.M, c.N, c.K
    a, w, bias = d["a"].cuda(), d["w"].cuda(), dev(d["bias"])
    what = G.case_id(c)
    outs = {}

    def buf(name, rows, cols, ld, dtype, off=0):
        b = G.OutBuf(rows, cols, ld, dtype, off)
        flat = b.flat.cuda()
        outs[name] = (b, flat)
        return b.view(flat)

    launches, before = planned_launches(hip, c), hip.lib.tasu_gemm_launch_count()
    if c.op in ("plain", "relu"):
        cv = buf("c", M, N, N + c.pad, BF if c.mode == 0 else F32, c.coff)
        R = None if d["resid"] is None else d["resid_buf"].view(d["resid"].cuda())
        if c.op == "relu":
            hip.gemm_bias_relu(a, w, cv, M, N, K, bias)
        elif c.via == "policy":
            hip.gemm(a, w, cv, M, N, K, bias=bias, resid=R, mode=c.mode)
        elif c.via == "streamk":
            hip.gemm_streamk(a, w, cv, M, N, K, bias=bias, resid=R, mode=c.mode)
        else:
            hip.gemm_on(c.via, a, w, cv, M, N, K, bias=bias, resid=R, mode=c.mode)
    elif c.op == "swiglu":
        gu, act = buf("gu", M, 2 * N, 2 * N, BF, c.coff), buf("act", M, N, N + c.pad, BF, c.coff)
        hip.gemm_gate_up_swiglu(a, w, gu, act, M, N, K)
    elif c.op == "qkv":
        qkv = buf("qkv", M, N, N, BF)
        hip.gemm_qkv_rope(a, w, bias, qkv, d["cos"].cuda(), d["sin"].cuda(), M, c.H, c.G, K)
    elif c.op == "dswiglu":
        dgu, dact = buf("dgu", M, 2 * N, 2 * N, BF), buf("dact", M, N, N, BF)
        hip.gemm_dswiglu(a, w, d["gu"].cuda(), dgu, dact, M, N, K)
    else:
        ws, cv = buf("slabs", c.ks * M, N, N, F32), buf("c", M, N, N, BF)
        if c.op == "splitk":
            hip.gemm_splitk(a, w, cv, M, N, K, c.ks, ws)
        else:
            hip.gemm_slabs(a, w, ws, M, N, K, c.ks)
            hip.sum_slabs(ws, c.ks, cv, M * N)
    if launches is not None:
        got = hip.lib.tasu_gemm_launch_count() - before
        assert got == launches, f"{what}: {got} GEMM launches, the plan stands for {launches}"
    torch.cuda.synchronize()
    res = {name: b.check(flat, f"{what} {name}") for name, (b, flat) in outs.items()}
    if c.op == "qkv":
        q = res.pop("qkv")
        res["qk"], res["v"] = q[:, :(c.H + c.G) * HD], q[:, (c.H + c.G) * HD:]
    if "slabs" in res:
        s = res.pop("slabs")
        for i in range(c.ks):
            res[f"slab{i}"] = s[i * M:(i + 1) * M]
    if G.needs_workspace(c):
        assert int(hip.gemm_ws[:4096 * 4].view(torch.int32).abs().sum()) == 0, f"{what}: flag / counter words of the workspace left set"
    return res


@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_gemm_against_float64(hip, fake, case):
    family, what = G.FAMILY[case.op], G.case_id(case)
    d = G.make_inputs(case, "exact")
    ref = G.reference(case, d)
    out = run_case(hip, case, d)
    worst = G.check_case(case, d, ref, out, what)
    _worst[family] = max(_worst.get(family, 0.0), worst)
    print(f"F64EXACT {family} {what}: bits {sorted(ref.exact)} equal, worst |err| / E {worst:.3f} (family so far {_worst[family]:.3f}), "
          f"rounded {ref.frac_rounded:.2f}")
    if G.needs_workspace(case):
        again = run_case(hip, case, d)
        for name in out:
            assert torch.equal(G._bits(out[name]), G._bits(again[name])), f"{what}: {name} differs between two runs"
    if not case.n01:
        return
    dn = G.make_inputs(case, "n01")
    refn = G.reference(case, dn)
    out_n = run_case(hip, case, dn)
    worst_n = G.check_case(case, dn, refn, out_n, f"{what} N(0, 1)")
    _worst[family + " n01"] = max(_worst.get(family + " n01", 0.0), worst_n)
    print(f"F64N01 {family} {what}: worst |err| / E {worst_n:.3f} (family so far {_worst[family + ' n01']:.3f})")
    double_n = G.run_double(fake, case, dn)
    want_rms = {name: G.rms_ulp(got, want, mag) for name, got, want, mag in G.rms_pairs(case, dn, refn, double_n)}
    for name, got, want, mag in G.rms_pairs(case, dn, refn, out_n):
        assert bool(torch.isfinite(got).all()), f"{what}: {name} is not finite on the N(0, 1) profile"
        if got.numel() >= 4096:                                  # (fewer elements: the statistic is noise)
            report(family, name, G.rms_ulp(got, want, mag), want_rms[name], what)


@pytest.mark.parametrize("relu_first", [True, False], ids=["relu-then-plain", "plain-then-relu"])
def test_relu_does_not_outlive_its_call(hip, relu_first):
    """bias + ReLU on a fused plan, and the plain GEMM with bias on the same operands, in either order: each gives its own exact
    bits -- the plain result keeps its negative values"""
    cr = [c for c in G.RELU_CASES if (c.M, c.N, c.K) == (300, 520, 256)][0]
    cp = cr._replace(op="plain")
    assert hip.lib.tasu_gemm_plan(cr.M, cr.N, cr.K, 0, 1) not in (G.TILES, G.SPLITK), "not a fused plan"
    d = G.make_inputs(cp, "exact")
    want = {True: G.reference(cr, d).exact["c"], False: G.reference(cp, d).exact["c"]}
    assert bool((want[False] < 0).any()) and not torch.equal(want[True], want[False])
    a, w, bias = d["a"].cuda(), d["w"].cuda(), d["bias"].cuda()
    bufs = {}
    for relu in (relu_first, not relu_first):
        b = G.OutBuf(cr.M, cr.N, cr.N + cr.pad, BF)
        flat = b.flat.cuda()
        (hip.gemm_bias_relu if relu else hip.gemm)(a, w, b.view(flat), cr.M, cr.N, cr.K, bias=bias)
        bufs[relu] = (b, flat)
    torch.cuda.synchronize()
    for relu, (b, flat) in bufs.items():
        what = f"{'bias + ReLU' if relu else 'plain'} ({'first' if relu == relu_first else 'second'} call)"
        G.assert_bits(b.check(flat, what), want[relu], what, cr.K)
    assert bool((bufs[False][0].check(bufs[False][1], "plain") < 0).any())


@pytest.mark.parametrize("ld_first", [True, False], ids=["ld-then-dense", "dense-then-ld"])
def test_act_leading_dimension_does_not_outlive_its_call(hip, ld_first):
    """gate|up + SwiGLU with act inside a wider buffer (the _ld form), and the dense form at the same shape, in either order.  The
    dense act sits at the head of a buffer as large as the padded one, so that a leading dimension carried over from the other call
    would land inside it: everything behind the dense [M, I] keeps the sentinel."""
    cl = [c for c in G.SWIGLU_CASES if c.pad == 64][0]
    cd = cl._replace(pad=0)
    M, I, K, ld = cl.M, cl.N, cl.K, cl.N + cl.pad
    d = G.make_inputs(cd, "exact")
    ref = G.reference(cd, d)
    a, w = d["a"].cuda(), d["w"].cuda()
    res = {}
    for padded in (ld_first, not ld_first):
        gu, act = G.OutBuf(M, 2 * I, 2 * I, BF), G.OutBuf(M, I, ld, BF)
        gflat, aflat = gu.flat.cuda(), act.flat.cuda()
        hip.gemm_gate_up_swiglu(a, w, gu.view(gflat), act.view(aflat) if padded else aflat[:M * I].view(M, I), M, I, K)
        res[padded] = (gu, gflat, act, aflat)
    torch.cuda.synchronize()
    for padded, (gu, gflat, act, aflat) in res.items():
        what = f"{'_ld' if padded else 'dense'} form ({'first' if padded == ld_first else 'second'} call)"
        if padded:
            got = act.check(aflat, f"{what} act")
        else:
            flat = aflat.cpu()
            assert torch.equal(G._bits(flat[M * I:]), G._bits(act.flat[M * I:])), f"{what}: act was written behind its dense [M, I]"
            got = flat[:M * I].view(M, I)
            assert not bool(torch.isnan(got).any())
        G.check_case(cd, d, ref, dict(gu=gu.check(gflat, f"{what} gu"), act=got), what)


def test_gemm_entry_points_refuse_what_they_do_not_serve(hip):
    """refused before any launch: the outputs keep their sentinel"""
    from ps_slm_amd.ops import TasuOpError
    M, N = 300, 520
    out, outf = G.OutBuf(M, N, N, BF), G.OutBuf(M, N, N, F32)
    c, cf = out.flat.cuda(), outf.flat.cuda()
    cv, cfv = out.view(c), outf.view(cf)
    z = lambda r, k: torch.zeros(r, k, dtype=BF, device="cuda")
    ws = torch.zeros(16 * M * N, device="cuda")
    with pytest.raises(TasuOpError, match="bad argument"):       # K no multiple of 64
        hip.gemm(z(M, 96), z(N, 96), cv, M, N, 96)
    with pytest.raises(TasuOpError, match="bad argument"):
        hip.gemm_on("pipe128", z(M, 160), z(N, 160), cv, M, N, 160)
    with pytest.raises(TasuOpError, match="bad argument"):       # the 256 x 256 kernel: K >= 256, a multiple of 128
        hip.gemm_on("pp256", z(M, 192), z(N, 192), cv, M, N, 192)
    with pytest.raises(TasuOpError, match="bad argument"):
        hip.gemm_streamk(z(M, 192), z(N, 192), cv, M, N, 192)
    with pytest.raises(TasuOpError, match="bad argument"):       # slabs: K / ksplit >= 256
        hip.gemm_slabs(z(M, 1024), z(N, 1024), ws, M, N, 1024, 8)
    with pytest.raises(TasuOpError, match="bad argument"):       # ... and K a multiple of 128 ksplit
        hip.gemm_slabs(z(M, 1024), z(N, 1024), ws, M, N, 1024, 3)
    with pytest.raises(TasuOpError, match="bad argument"):       # split-K: at most 16 ranges of whole K-tiles
        hip.gemm_splitk(z(M, 1024), z(N, 1024), cv, M, N, 1024, 32, ws)
    a, b = z(M, 1024), z(N, 1024)
    rc = hip.lib.tasu_gemm_nt_bf16_splitk(a.data_ptr(), 1024, b.data_ptr(), 1024, ws.data_ptr(), N - 8, M, N, 1024, 4, hip._stream())
    assert rc == 1, "split-K took ldc < N"
    for mode_call in (lambda: hip.gemm(a, b, cfv, M, N, 1024, mode=2), lambda: hip.gemm_on("pipe192", a, b, cfv, M, N, 1024, mode=2),
                      lambda: hip.gemm_streamk(a, b, cfv, M, N, 1024, mode=2)):
        with pytest.raises(TasuOpError, match="bad argument"):   # residual mode without R
            mode_call()
    torch.cuda.synchronize()
    out.check(c, "refused calls")
    outf.check(cf, "refused calls")
    assert torch.equal(G._bits(out.view(c.cpu())), G._bits(out.view())) and torch.equal(G._bits(outf.view(cf.cpu())), G._bits(outf.view()))
    assert int(ws.abs().sum()) == 0
