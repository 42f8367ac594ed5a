"""Qwen3's per-head q/k RMSNorm kernels (csrc/qk_norm.hip: tasu_qk_norm_rope_fwd, tasu_qk_norm_bwd, tasu_qk_norm_rope_append) against
the float64 reference, element by element (tests/qk_norm_ref64.py; its own checks: tests/test_qk_norm_ref64_cpu.py), through HipOps.

Shapes (M, H, G) = (5, 2, 1), (64, 12, 2), (67, 16, 8): an odd row count, one whole 64-row chunk and one row past it, both head
ratios, more than one workgroup.  Positions include 0, 1 and 4095.  Inputs: N(0, 1) heads, heads scaled by 1e-3 (eps decides the
result), one all-zero head (0, not NaN), negative weights.  Every output starts as NaN with guard rows that must keep their bits,
every operand has NaN behind what the kernel is owed; every case runs twice and must give equal bits.  Every element within 1.0 x E
of the float64 value; the v heads keep the projection's / the gradient's bits, forward and backward; out == pre gives the bits of
the separate output; rstd NULL gives the same output.  The append kernel: qkv in place, the key and the value at pos -- first slot,
last slot of ctx, a different pos per row -- carry the bits of the forward kernel's output on the same rows, and no other cache cell
is written.  Bad arguments return the error code and leave the outputs untouched.

Measured on MI355X (16 tests, under a second for the file): every check passes; largest |err| / E (the F64WORST lines): forward
0.996 on all three shapes, backward 0.978 / 0.995 / 0.996."""
import pytest
import torch

import qk_norm_ref64 as Q

pytestmark = pytest.mark.gpu
F32, BF, I32 = torch.float32, torch.bfloat16, torch.int32
CTX = 9


@pytest.fixture(scope="module")
def hip():
    from ps_slm_amd.ops import HipOps
    return HipOps()


def cuda(t):
    return t.cuda()


@pytest.fixture(scope="module", params=Q.CASES, ids=Q.case_id)
def case(request):
    d = Q.inputs(request.param)
    return d, Q.fwd_reference(d), Q.bwd_reference(d)


def test_forward_against_float64(hip, case):
    d, ref, _ = case
    out = Q.run_fwd(hip, d, cuda)
    w = Q.check(out, ref, "qk_norm_rope_fwd")
    print(f"F64WORST qk_norm_rope_fwd {Q.case_id((d['M'], d['H'], d['G']))}: {w:.3f}")
    zero = (ref.tol["qk"][1] == 0)
    assert bool(zero.any()) and bool((out["qk"].float()[zero] == 0).all())                       # the all-zero head: 0, not NaN
    assert torch.equal(out["v"], ref.exact["v"])
    alias = Q.run_fwd(hip, d, cuda, alias=True)
    Q.same_bits(alias["qk"], out["qk"], "out == pre against a separate output")
    Q.same_bits(alias["rstd"], out["rstd"], "out == pre: rstd")
    assert torch.equal(alias["v"], ref.exact["v"])
    nor = Q.run_fwd(hip, d, cuda, want_rstd=False)
    Q.same_bits(nor["qk"], out["qk"], "rstd NULL against rstd kept")
    assert torch.equal(nor["v"], ref.exact["v"])


def test_backward_against_float64(hip, case):
    d, _, ref = case
    out = Q.run_bwd(hip, d, cuda)
    w = Q.check(out, ref, "qk_norm_bwd")
    print(f"F64WORST qk_norm_bwd {Q.case_id((d['M'], d['H'], d['G']))}: {w:.3f}")
    assert torch.equal(out["v"], ref.exact["v"])


@pytest.mark.parametrize("kind", ["first", "last", "mixed"])
def test_append_carries_the_forward_kernels_bits(hip, case, kind):
    d, _, _ = case
    fwd = Q.run_fwd(hip, d, cuda, again=False)
    Q.run_append(hip, d, fwd, CTX, kind, cuda)


def test_bad_arguments_return_the_error_code(hip):
    from ps_slm_amd.ops import TasuOpError
    M, H, G = 3, 2, 1
    LD = (H + 2 * G) * Q.HD
    pre, out, dq = (Q.nan(M, LD + 8, dtype=BF).cuda() for _ in range(3))
    wq, wk = torch.ones(Q.HD + 4).cuda(), torch.ones(Q.HD + 4).cuda()
    cs, sn, rstd = torch.ones(M, 64).cuda(), torch.zeros(M, 64).cuda(), Q.nan(M, H + G).cuda()
    kc, vc = Q.nan(M, CTX, G * Q.HD + 8, dtype=BF).cuda(), Q.nan(M, CTX, G * Q.HD + 8, dtype=BF).cuda()
    pos = torch.zeros(M, dtype=I32).cuda()
    flat = lambda t, off=0: t.view(-1)[off:off + M * LD].view(M, LD)            # noqa: E731  (off = 1: 2 bytes past a 16-byte boundary)
    w = lambda t, off=0: t[off:off + Q.HD]                                      # noqa: E731  (off = 1: 4 bytes past one)

    def refused(fn):
        with pytest.raises(TasuOpError):
            fn()
        torch.cuda.synchronize()
        for t in (out, dq, rstd, kc, vc):
            assert Q.untouched(t.cpu()), "a refused call wrote an output"

    fwd = lambda **k: hip.qk_norm_rope_fwd(k.get("pre", flat(pre)), k.get("wq", w(wq)), k.get("wk", w(wk)), cs, sn, k.get("out", flat(out)), rstd,  # noqa: E731
                                           k.get("M", M), k.get("H", H), k.get("G", G), k.get("eps", 1e-6))
    bwd = lambda **k: hip.qk_norm_bwd(k.get("dq", flat(dq)), k.get("pre", flat(pre)), k.get("wq", w(wq)), w(wk), rstd, k.get("M", M), k.get("H", H),  # noqa: E731
                                      k.get("G", G))
    app = lambda **k: hip.qk_norm_rope_append(k.get("qkv", flat(out)), w(wq), k.get("wk", w(wk)), cs, sn, k.get("kc", kc), vc, k.get("pos", pos),  # noqa: E731
                                              k.get("M", M), H, k.get("G", G), k.get("ctx", CTX), 1e-6)
    for call in (fwd, bwd, app):
        refused(lambda: call(M=0))
        refused(lambda: call(G=0))
    refused(lambda: fwd(H=3, G=2))                                              # H % G
    refused(lambda: fwd(pre=None))
    refused(lambda: fwd(eps=-1.0))
    refused(lambda: fwd(pre=flat(pre, 1)))                                      # misaligned pointers
    refused(lambda: fwd(out=flat(out, 1)))
    refused(lambda: fwd(wq=w(wq, 1)))
    refused(lambda: fwd(pre=flat(out), out=flat(out, 8)))                       # overlapping, not equal
    refused(lambda: bwd(dq=flat(dq, 1)))
    refused(lambda: bwd(dq=flat(pre)))                                          # dqkv == pre
    refused(lambda: bwd(wq=None))
    refused(lambda: app(qkv=flat(out, 1)))
    refused(lambda: app(wk=w(wk, 1)))
    refused(lambda: app(pos=None))
    refused(lambda: app(ctx=0))
    refused(lambda: app(kc=kc.view(-1)[1:]))
