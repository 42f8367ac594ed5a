"""The bf16 decode-step kernels against float64 references, element by element (tests/decode_ref64.py; its own checks:
tests/test_decode_ref64_cpu.py), through HipOps like tests/test_gpu_ops.py:

  cache attention   tasu_attn_decode (csrc/attn_decode_body.h): every instantiated group size, both output layouts, with and
                    without the row index, M = 1 / 9 / 64, visible lengths on every switch of the kernel, ragged kstart, N(0, 1)
                    and peaked inputs, the longest context.  The caches are poisoned: a physical row M of NaN that every index
                    entry outside the visible range points at, NaN in every cell no visible key refers to.  Finite and within
                    1.1 x E on every element; rms(err / E) at most 1.5 x the torch double's.
  decode GEMMs      csrc/gemm_skinny.hip (unsplit, BN = 96, split K through each finish kernel) and csrc/gemm_stream.hip (every
                    K range, slabs, row-major and fragment-order operands, every epilogue, the one-launch norm), the `hip_both`
                    pattern: the exact profile's BITS for the linear epilogues, 1.0 x E for SwiGLU, bias + RoPE and the residual
                    RMSNorm on exact accumulations, the appended cache cells on a patterned cache; on the N(0, 1) profile
                    rms(err / (u |c|)) at most 1.5 x the double's.  Then the forms with a norm inside its neighbours, held to
                    their own definition.

Every output and scratch buffer starts as NaN; row-major outputs have guard rows past M and guard columns past N that must keep
their bits.

Largest ratios measured over the case lists (MI355X), kernel rms / double rms (the F64RATIO lines this file prints):
    attention           row-major 1.002    fragment order 1.002 (the same bits)
    gemm_skinny.hip     c 1.000   act 1.000   y 1.000   q | k 1.000   v 1.000
    gemm_stream.hip     c 1.000   act 1.0003  y 1.000   q | k 1.000   v 1.000      (every layout and route)
The largest |err| / E per case equals the double's to three digits (SwiGLU 0.92, RMSNorm 0.99, bias + RoPE 0.996; the forms with
a norm inside: SwiGLU 0.81, q | k 0.92, v 0.98).  No kernel needed a fix."""
import contextlib

import pytest
import torch

import decode_ref64 as D
from fake_ops import FakeOps
from test_gpu_ops import ao_frag, unfrag

pytestmark = pytest.mark.gpu
HD = D.HD
BF, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32
NAN = float("nan")
WS_FLOATS = 4 << 20            # split-K / slab scratch: the largest plan of the case lists needs under 1 M floats


@pytest.fixture(scope="module")
def hip():
    from ps_slm_amd.ops import HipOps
    return HipOps()


@pytest.fixture(params=["stream", "skinny"])
def hip_both(hip, request):
    """as in tests/test_gpu_ops.py: the streaming kernels where they serve the shape, or the split-K + finish kernels"""
    hip.use_stream = hip.dec_down_slabs = request.param == "stream"
    yield hip
    hip.use_stream, hip.dec_down_slabs = True, True


@pytest.fixture(scope="module")
def fake():
    return FakeOps()


def nan(*shape, dtype):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def untouched(t):
    """every element still holds the NaN bits it was filled with"""
    it = torch.int16 if t.dtype == BF else torch.int32
    return torch.equal(t.contiguous().view(it), torch.full_like(t, NAN).contiguous().view(it))


def dev(t):
    return None if t is None else t.cuda()


@contextlib.contextmanager
def layout(hip, frag=False, frag_act=False, **attrs):
    """fragment-order operands / other HipOps attributes for the calls inside; a failure cannot leave them on"""
    keep = {k: getattr(hip, k) for k in attrs}
    hip.dec_frag, hip.dec_frag_act = frag, frag_act
    for k, v in attrs.items():
        setattr(hip, k, v)
    try:
        yield
    finally:
        hip.dec_frag = hip.dec_frag_act = False
        for k, v in keep.items():
            setattr(hip, k, v)


_ratios = {}


def report(family, name, kernel, double, case):
    ratio = kernel / double if double > 0 else 0.0
    _ratios[(family, name)] = max(_ratios.get((family, name), 0.0), ratio)
    print(f"F64RATIO {family} {name} {ratio:.3f} kernel {kernel:.5f} double {double:.5f} {case} (largest so far {_ratios[(family, name)]:.3f})")
    assert kernel <= D.RMS_RATIO * double, (f"{family} {name} {case}: rms {kernel:.5f} is {ratio:.2f} x the double's {double:.5f} "
                                            f"(at most {D.RMS_RATIO} x: a systematic error, not rounding)")


# ------------------------------------------------------------------------------------------------ cache attention
def run_attention(hip, c, dv, frag):
    """out [M, H, 128] (CPU) of tasu_attn_decode in one output layout; NaN beforehand, the guard rows checked"""
    M, H, G, ctx = c.M, c.H, c.G, c.ctx
    rows = (M + 63) // 64 * 64 if frag else M + 3
    out = nan(rows, H * HD, dtype=BF)
    with layout(hip, frag=frag):
        hip.attn_decode(dv["qkv"], dv["kc"], dv["vc"], dv["index"], dv["kstart"], dv["lens"], out, M, H, G, ctx, HD ** -0.5)
        torch.cuda.synchronize()
    got = out.cpu()
    if frag:
        got = unfrag(got, H * HD)
    assert untouched(got[M:]), f"attn_decode ({'fragment order' if frag else 'row-major'}): rows past M = {M} were written"
    return got[:M].reshape(1, M, H, HD)


@pytest.mark.parametrize("case", D.ATTN_CASES, ids=D.attn_case_id)
def test_attention_against_float64(hip, fake, case):
    inp = D.attn_inputs(case)
    ref, E = D.attn_reference_of(inp)
    want_rms = D.check_within(D.attn_double(fake, inp), ref, E, D.ATTN_LIMIT).rms
    dv = {k: dev(v) for k, v in inp.items() if isinstance(v, torch.Tensor) or v is None}
    outs = []
    for frag in (False, True):
        what = "fragment order" if frag else "row-major"
        out = run_attention(hip, case, dv, frag)
        rms = D.assert_within(out, ref, E, D.ATTN_LIMIT, f"attn_decode, {what}")
        report("attention", what.replace(" ", "-"), rms, want_rms, D.attn_case_id(case))
        outs.append(out)
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), "the two output layouts hold different bits"


@pytest.mark.parametrize("H,G,ctx,why", [(3, 1, 64, "REP 3"), (5, 1, 64, "REP 5"), (10, 2, 64, "REP 5"), (2, 1, 2049, "ctx > 2048"),
                                         (12, 2, 2049, "ctx > 2048")] +
                         [(rep, 1, D.attn_first_refused_ctx(rep), "LDS > 160 KB") for rep in (1, 2, 4, 6, 7, 8)])
def test_attention_refuses_what_it_does_not_serve(hip, H, G, ctx, why):
    """refused before any launch (the buffers are full-sized all the same)"""
    from ps_slm_amd.ops import TasuOpError
    M, W = 1, G * HD
    qkv, kc, vc = (torch.zeros(n, dtype=BF, device="cuda") for n in (M * (H + 2 * G) * HD, M * ctx * W, M * ctx * W))
    one = torch.ones(M, dtype=I32, device="cuda")
    out = nan(64, H * HD, dtype=BF)
    assert (D.attn_lds_floats(H // G, ctx) * 4 > D.LDS_BYTES) == (why == "LDS > 160 KB")
    with pytest.raises(TasuOpError, match="bad argument"):
        hip.attn_decode(qkv, kc, vc, None, one - 1, one, out, M, H, G, ctx, HD ** -0.5)
    torch.cuda.synchronize()
    assert untouched(out)


# ------------------------------------------------------------------------------------------------ decode GEMMs
def ranges_of(hip, K):
    ks = hip._stream_split(K)
    """for a failure message: how the current family cuts this K (an epilogue gemm_stream.hip does not serve, such as the fp32
    output, takes gemm_skinny.hip's split whatever the family)"""
    return f"(streaming kernels' plan: {ks} K range{'s' if ks != 1 else ''})" if ks else "(split-K kernels of gemm_skinny.hip)"


def variants(hip, c):
    """the operand layouts / routes one case runs on under the current family: dicts of run_gemm's keywords"""
    out = [dict()]
    if not hip.use_stream:
        return out
    ks = hip._stream_split(c.K)
    if c.op == "plain" and c.mode == 0 and ks == 1:
        out.append(dict(frag=True))
    if c.op == "swiglu" and ks == 1 and c.N % 8 == 0:
        out.append(dict(frag=True))
        if c.N % 32 == 0:
            out.append(dict(frag=True, frag_act=True))
    if c.op == "qkv" and ks == 1:
        out.append(dict(frag=True))
    if c.op == "norm" and c.N % 16 == 0 and ks >= 1:
        served = ks == 1 or hip._slab_finish_serves(c.N)
        if served and c.N % 32 == 0:
            out.append(dict(frag=True, frag_act=ks > 1))
        if served and c.N in (256, 1536) and c.K % ks == 0:          # (the one-launch form takes equal K ranges only)
            out.append(dict(fused=True))
            out.append(dict(fused=True, frag=True, frag_act=ks > 1))
        if c.K == 8960:                                          # 5 x 1792 instead of 7 x 1280
            out.append(dict(order=(1, 5, 7, 2, 3, 4, 6, 8, 13)))
    return out


def run_gemm(hip, c, d, frag=False, frag_act=False, fused=False, order=None):
    """One case on the current family and layout: name -> CPU result (the names of decode_ref64.gemm_reference).  Every output and
    the scratch start as NaN; guard rows / columns are checked here."""
    M, N, K, ldc = c.M, c.N, c.K, d["ldc"]
    w = d["w"].cuda()
    a = ao_frag(d["a"], K).cuda()[:M] if frag else d["a"].cuda()
    ws = nan(WS_FLOATS, dtype=F32)
    attrs = dict(dec_fused_norm=fused)
    if order is not None:
        attrs["dec_split_order"] = order
    res = {}
    try:
        with layout(hip, frag=frag, frag_act=frag_act, **attrs):
            if frag:
                kind = {"plain": "plain", "norm": "plain", "swiglu": "swiglu", "qkv": "qkv"}[c.op]
                hip.register_decode_weight(w, kind, N, c.H, c.G, slabs_ok=True)
                assert w.data_ptr() in hip._frag, "no fragment-order copy was made"
            if c.op == "plain":
                cb = nan(M + 2, ldc, dtype=BF if c.mode == 0 else F32)
                hip.gemm_skinny(a, w, cb, M, N, K, ws, bias=dev(d["bias"]), resid=dev(d["resid"]), mode=c.mode)
                torch.cuda.synchronize()
                cb = cb.cpu()
                assert untouched(cb[M:]) and untouched(cb[:M, N:]), "gemm_skinny wrote past M rows / N columns"
                res["c"] = cb[:M, :N]
            elif c.op == "swiglu":
                rows = 64 if frag_act else M + 2
                act = nan(rows, N, dtype=BF)
                hip.gemm_skinny_swiglu(a, w, act[:M], M, N, K, ws)
                torch.cuda.synchronize()
                act = act.cpu()
                if frag_act:
                    act = unfrag(act, N)
                else:
                    assert untouched(act[M:]), "gemm_skinny_swiglu wrote past M rows"
                res["act"] = act[:M]
            elif c.op == "norm":
                cb, y = nan(M + 2, N, dtype=F32), nan(64 if frag else M + 2, N, dtype=BF)
                hip.gemm_skinny_norm(a, w, cb, dev(d["resid"]), M, N, K, dev(d["norm_w"]), y[:M], D.EPS, ws)
                torch.cuda.synchronize()
                assert int(hip.norm_sync.abs().sum()) == 0
                cb, y = cb.cpu(), y.cpu()
                if frag:
                    y = unfrag(y, N)
                assert untouched(cb[M:]) and untouched(y[M:]), "gemm_skinny_norm wrote past M rows"
                res["c"], res["y"] = cb[:M], y[:M]
            else:
                W = c.G * HD
                kc0, vc0 = D.cache_pattern(M + 1, c.ctx, W, 1), D.cache_pattern(M + 1, c.ctx, W, 2)
                kc, vc, qkv = kc0.cuda(), vc0.cuda(), nan(M + 2, N, dtype=BF)
                hip.gemm_skinny_qkv_rope(a, w, dev(d["bias"]), qkv, M, c.H, c.G, K, dev(d["cos"]), dev(d["sin"]), kc, vc, dev(d["pos"]),
                                         c.ctx, ws)
                torch.cuda.synchronize()
                qkv, kc, vc = qkv.cpu(), kc.cpu(), vc.cpu()
                n1 = M * c.ctx * W
                assert untouched(qkv[M:]), "gemm_skinny_qkv_rope wrote past M rows"
                assert torch.equal(kc[n1:].view(torch.int16), kc0[n1:].view(torch.int16)) and \
                    torch.equal(vc[n1:].view(torch.int16), vc0[n1:].view(torch.int16)), "a cache row past M was written"
                res.update(qk=qkv[:M, :(c.H + c.G) * HD], v=qkv[:M, (c.H + c.G) * HD:], kc=kc[:n1], vc=vc[:n1], kc0=kc0[:n1], vc0=vc0[:n1])
    finally:
        hip.forget_decode_weights([w.data_ptr()])
    return res


def name_of(v):
    return "+".join(f"{k}" for k, x in v.items() if x) or "row-major"


@pytest.mark.parametrize("case", D.GEMM_CASES, ids=D.gemm_case_id)
def test_gemm_against_float64(hip_both, fake, case):
    hip = hip_both
    family = "stream" if hip.use_stream else "skinny"
    exact, n01 = D.gemm_inputs(case, "exact"), D.gemm_inputs(case, "n01")
    ref, refn = D.gemm_reference(case, exact), D.gemm_reference(case, n01)
    double_n = D.gemm_double(fake, case, n01)
    want_rms = {name: D.rms_ulp(got, want, mag) for name, got, want, mag in D.rms_pairs(case, n01, refn, double_n)}
    first = None
    for v in variants(hip, case):
        what = f"{family} {D.gemm_case_id(case)} [{name_of(v)}]"
        order = v.get("order")
        with layout(hip, **({"dec_split_order": order} if order else {})):
            rng = ranges_of(hip, case.K)
        out = run_gemm(hip, case, exact, **v)
        worst = D.check_gemm_case(case, exact, ref, out, D.GEMM_LIMIT, what, rng)
        print(f"F64EXACT {what} {rng}: bits {sorted(ref.exact)} equal, worst |err| / E {worst:.3f}")
        if first is None:
            first = out
        elif not order:                                          # layouts and the one-launch norm change no bit
            for name in ("c", "act", "y", "qk", "v"):
                if name in out:
                    assert torch.equal(out[name], first[name]), f"{what}: {name} differs from the row-major run"
        out_n = run_gemm(hip, case, n01, **v)
        for name, got, want, mag in D.rms_pairs(case, n01, refn, out_n):
            assert bool(torch.isfinite(got).all()), f"{what}: {name} is not finite on the N(0, 1) profile"
            if case.M * case.N >= 4096:                          # (fewer elements: the statistic is noise)
                report(family, name, D.rms_ulp(got, want, mag), want_rms[name], f"{D.gemm_case_id(case)} [{name_of(v)}]")
        if case.op == "qkv":
            D.check_appended(out_n, case, n01, what)


def test_gemm_fragment_route_that_cannot_run_is_refused(hip):
    """N = 4352 behind two K ranges: the slab finish does not serve it, so a fragment-order activation has no reader -- an error,
    not a row-major kernel misreading it"""
    from ps_slm_amd.ops import TasuOpError
    case = [c for c in D.NORM_CASES if c.N == 4352][0]
    hip.use_stream = hip.dec_down_slabs = True
    with pytest.raises(TasuOpError, match="fragment order"):
        run_gemm(hip, case, D.gemm_inputs(case, "exact"), frag=True, frag_act=True)


@pytest.mark.parametrize("M,K,why", [(65, 256, "M > 64"), (64, 96, "K no multiple of 64"), (64, 2080, "K no multiple of 64")])
def test_gemm_refuses_bad_arguments(hip_both, M, K, why):
    from ps_slm_amd.ops import TasuOpError
    hip = hip_both
    N = 64
    a, w = torch.zeros(M, K, dtype=BF, device="cuda"), torch.zeros(N, K, dtype=BF, device="cuda")
    ws = nan(WS_FLOATS, dtype=F32)
    c, cf, y = nan(M, N, dtype=BF), nan(M, N, dtype=F32), nan(M, N, dtype=BF)
    r, nw = torch.zeros(M, N, device="cuda"), torch.ones(N, device="cuda")
    with pytest.raises(TasuOpError, match="bad argument"):
        hip.gemm_skinny(a, w, c, M, N, K, ws)
    with pytest.raises(TasuOpError, match="bad argument"):
        hip.gemm_skinny_swiglu(a, w, c[:, :N // 2], M, N // 2, K, ws)
    with pytest.raises(TasuOpError, match="bad argument"):
        hip.gemm_skinny_norm(a, w, cf, r, M, N, K, nw, y, D.EPS, ws)
    torch.cuda.synchronize()
    assert untouched(c) and untouched(cf) and untouched(y)


# ------------------------------------------------------------------------------------------------ cache append kernels
def test_cache_append_kernels_write_exactly_their_slots(hip):
    """tasu_kv_append and tasu_rope_append on patterned caches: exactly the cells [m, pos[m]] change, to the bits of the k and v
    blocks the call leaves in qkv[m]; the rotation within u |y| + 2^-22 (|x1 c| + |x2 s|)"""
    case = D.GemmCase("qkv", 9, 8 * HD, 0, 0, False, 4, 2, 16)
    M, H, G, ctx, W = case.M, case.H, case.G, case.ctx, case.G * HD
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(M, case.N, generator=g).to(BF)
    ang = torch.randn(M, 64, generator=g)
    d = dict(pos=torch.tensor([3, 0, 15, 7, 7, 1, 15, 0, 8], dtype=I32), cos=torch.cos(ang), sin=torch.sin(ang))
    for op in ("kv_append", "rope_append"):
        kc0, vc0 = D.cache_pattern(M, ctx, W, 3), D.cache_pattern(M, ctx, W, 4)
        kc, vc, q = kc0.cuda(), vc0.cuda(), qkv.cuda()
        if op == "kv_append":
            hip.kv_append(q, kc, vc, dev(d["pos"]), M, H, G, ctx)
        else:
            hip.rope_append(q, dev(d["cos"]), dev(d["sin"]), kc, vc, dev(d["pos"]), M, H, G, ctx)
        torch.cuda.synchronize()
        q = q.cpu()
        out = dict(qk=q[:, :(H + G) * HD], v=q[:, (H + G) * HD:], kc=kc.cpu(), vc=vc.cpu(), kc0=kc0, vc0=vc0)
        D.check_appended(out, case, d, op)
        assert torch.equal(out["v"], qkv[:, (H + G) * HD:])
        if op == "kv_append":
            assert torch.equal(q, qkv)
        else:
            x = qkv[:, :(H + G) * HD].to(F64).view(M, H + G, HD)
            cs, sn = d["cos"].to(F64)[:, None], d["sin"].to(F64)[:, None]
            x1, x2 = x[..., :64], x[..., 64:]
            rot = torch.cat([x1 * cs - x2 * sn, x2 * cs + x1 * sn], -1)
            E = D.U * rot.abs() + 2.0 ** -22 * torch.cat([(x1 * cs).abs() + (x2 * sn).abs(), (x2 * cs).abs() + (x1 * sn).abs()], -1)
            D.assert_gemm_within(out["qk"], rot.reshape(M, -1), E.reshape(M, -1), D.GEMM_LIMIT, "rope_append q | k", 0)


# ------------------------------------------------------------------------------------------------ the norm inside its neighbours
@pytest.mark.parametrize("M,Dm,I,H,G", [(64, 256, 1024, 2, 1), (23, 512, 2560, 4, 2)])
def test_prenorm_forms_against_their_definition(hip, M, Dm, I, H, G):
    """o projection -> [post-attention norm] -> gate|up + SwiGLU (tasu_gemm_stream_resid_prenorm + _swiglu_rstd) and down-projection
    slabs -> [input norm] -> q|k|v (tasu_stream_finish_prenorm + tasu_gemm_stream_qkv_rope_rstd), fragment order, exact profile
    with a norm weight of powers of two: the residual stream C and yw = bf16(norm_w C) are exact BITS, the per-tile sums of
    squares hold to 20 . 2^-24, and the consumers are held to the float64 value of their definition on the yw and sums of squares
    they were given (decode_ref64.rstd_consumer_reference)."""
    HHD, LD, ctx, W = H * HD, (H + 2 * G) * HD, 12, G * HD
    g = torch.Generator().manual_seed(Dm + I + M)
    ri = lambda lo, hi, *sh: torch.randint(lo, hi + 1, sh, generator=g).to(F32)
    s_o, s_d, s_c = (2.0 ** -D.exact_shift(k) for k in (HHD, I, Dm))
    ao, act = ri(-4, 4, M, HHD).to(BF), ri(-4, 4, M, I).to(BF)
    wo, wd = (ri(-4, 4, Dm, HHD) * s_o).to(BF), (ri(-4, 4, Dm, I) * s_d).to(BF)
    wgu, wqkv = (ri(-4, 4, 2 * I, Dm) * s_c).to(BF), (ri(-4, 4, LD, Dm) * s_c).to(BF)
    bq = (ri(-8, 8, LD) * 2.0 ** -4).to(BF)
    x_o, x_d = ri(-64, 64, M, Dm) * s_o, ri(-64, 64, M, Dm) * s_d
    ln2, ln1 = D.prenorm_weight(Dm, 1), D.prenorm_weight(Dm, 2)
    ang = torch.randn(M, 64, generator=g)
    cos, sin = torch.cos(ang), torch.sin(ang)
    pos = (torch.arange(M) * 5 % ctx).to(I32)
    wts = {k: v.cuda() for k, v in dict(wo=wo, wd=wd, wgu=wgu, wqkv=wqkv).items()}
    hip.use_stream = hip.dec_down_slabs = True
    try:
        hip.register_decode_weight(wts["wqkv"], "qkv", LD, H, G)
        hip.register_decode_weight(wts["wo"], "plain", Dm)
        hip.register_decode_weight(wts["wgu"], "swiglu", I)
        hip.register_decode_weight(wts["wd"], "plain", Dm, slabs_ok=True)
        assert hip.begin_decode(Dm, HHD, I)
        assert hip.prenorm_ok(Dm, HHD, I) and hip.prenorm_in_ok(Dm, I)
        ws = nan(WS_FLOATS, dtype=F32)
        # post-attention norm inside the o projection and gate|up
        c2, yw, a2 = nan(M + 2, Dm, dtype=F32), nan(64, Dm, dtype=BF), nan(64, I, dtype=BF)
        hip.dec_sumsq.fill_(NAN)
        ssq = hip.gemm_skinny_prenorm(ao_frag(ao, HHD).cuda()[:M], wts["wo"], c2, x_o.cuda(), M, Dm, HHD, ln2.cuda(), yw[:M])
        hip.gemm_skinny_swiglu(yw[:M], wts["wgu"], a2[:M], M, I, Dm, None, sumsq=ssq, eps=D.EPS)
        torch.cuda.synchronize()
        act_frag = bool(hip.dec_frag_act)
        post = (c2.cpu(), unfrag(yw.cpu(), Dm), ssq.cpu().clone(), unfrag(a2.cpu(), I) if act_frag else a2.cpu())
        # input norm inside the slab finish and q|k|v
        c3, xn, qkv = nan(M + 2, Dm, dtype=F32), nan(64, Dm, dtype=BF), nan(M + 2, LD, dtype=BF)
        kc0, vc0 = D.cache_pattern(M, ctx, W, 5), D.cache_pattern(M, ctx, W, 6)
        kc, vc = kc0.cuda(), vc0.cuda()
        hip.dec_sumsq_in.fill_(NAN)
        ssq_in = hip.gemm_skinny_norm(ao_frag(act, I).cuda()[:M], wts["wd"], c3, x_d.cuda(), M, Dm, I, ln1.cuda(), xn[:M], D.EPS, ws, prenorm_slot=0)
        assert ssq_in is not None
        hip.gemm_skinny_qkv_rope(xn[:M], wts["wqkv"], bq.cuda(), qkv, M, H, G, Dm, cos.cuda(), sin.cuda(), kc, vc, pos.cuda(), ctx, ws,
                                 sumsq=ssq_in, eps=D.EPS)
        torch.cuda.synchronize()
        pre = (c3.cpu(), unfrag(xn.cpu(), Dm), ssq_in.cpu().clone(), qkv.cpu(), kc.cpu(), vc.cpu())
    finally:
        hip.end_decode()
        hip.forget_decode_weights([w.data_ptr() for w in wts.values()])
        hip.dec_sumsq.zero_()
        hip.dec_sumsq_in.zero_()
    for what, (c, y, q), a, w, x, ln, K in (("o projection", post[:3], ao, wo, x_o, ln2, HHD), ("down projection", pre[:3], act, wd, x_d, ln1, I)):
        C = x.to(F64) + D._bf64(a.to(F64) @ w.to(F64).t())
        D.assert_bits(c[:M], C.to(F32), f"{what}: residual stream", K, ranges_of(hip, K))
        assert untouched(c[M:]) and untouched(y[M:]), f"{what}: rows past M were written"
        D.assert_bits(y[:M], (ln.to(F64) * C).to(F32).to(BF), f"{what}: yw = bf16(norm_w C)", K)
        D.check_sumsq(q.view(-1, 64), c, M, Dm, what)
    tol = D.rstd_consumer_reference("swiglu", post[1], wgu, post[2].view(-1, 64), M, Dm, D.EPS, unit=0.5 * s_o * s_c)
    ref, E = tol["act"]
    cw = D.assert_gemm_within(post[3][:M], ref, E, D.GEMM_LIMIT, "gate|up + SwiGLU with rstd", Dm)
    print(f"F64PRENORM swiglu_rstd M={M} D={Dm} I={I}: worst |err| / E {cw.worst:.3f}, rms {cw.rms:.4f}")
    tol = D.rstd_consumer_reference("qkv", pre[1], wqkv, pre[2].view(-1, 64), M, Dm, D.EPS, unit=0.5 * s_d * s_c, bias=bq, cos=cos, sin=sin,
                                    H=H, G=G)
    got = pre[3]
    assert untouched(got[M:])
    for name, blk in (("qk", got[:M, :(H + G) * HD]), ("v", got[:M, (H + G) * HD:])):
        ref, E = tol[name]
        cw = D.assert_gemm_within(blk, ref, E, D.GEMM_LIMIT, f"q|k|v with rstd, {name}", Dm)
        print(f"F64PRENORM qkv_rope_rstd {name} M={M} D={Dm}: worst |err| / E {cw.worst:.3f}, rms {cw.rms:.4f}")
    case = D.GemmCase("qkv", M, LD, Dm, 0, True, H, G, ctx)
    D.check_appended(dict(qk=got[:M, :(H + G) * HD], v=got[:M, (H + G) * HD:], kc=pre[4], vc=pre[5], kc0=kc0, vc0=vc0), case, dict(pos=pos),
                     "q|k|v with rstd")
