"""The q_norm / k_norm weight-gradient kernels (csrc/qk_norm.hip: tasu_qk_norm_wgrad, tasu_f32_qk_norm_wgrad) against the float64
reference, element by element (tests/qk_wgrad_ref64.py; its own checks: tests/test_qk_wgrad_ref64_cpu.py), through HipOps.

Shapes M in {1, 5, 67, 300} x (H, G) in {(2, 1), (4, 4), (16, 8)}, and (700, 16, 8), where every group of both kernels walks more
than one unit and the last sweep is ragged.  Exact profile (integers, rstd a power of two): the float64 sum's value, both
families, accumulate 0 and 1.  General profile: every element within E = (N - 1) 2^-24 sum |g xn| (fp32 family: N + 2 - 1) of the
float64 value.  The v block of both operands is NaN and must not matter; dwq, dwk and ws sit between NaN guards and, without
accumulate, start as NaN; every run is made twice and must give equal bits.  Bad arguments return the error code and leave the
outputs untouched.

Measured on MI355X (54 tests, 2 s for the file): every check passes; largest |err| / E (the F64WORST lines): bf16 family 0.993 at
(1, 2, 1) with accumulate (two terms: ONE rounded addition against half an ulp of the magnitudes), 0.25 and below elsewhere; fp32
family 0.711 at (1, 2, 1), 0.32 and below elsewhere; 0.0004 and below at 300 x 16 and 700 x 16 rows x heads."""
import pytest
import torch

import qk_wgrad_ref64 as Q

pytestmark = pytest.mark.gpu
F32, BF = torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def hip():
    from ps_slm_amd.ops import HipOps
    return HipOps()


def cuda(t):
    return t.cuda()


@pytest.mark.parametrize("family", Q.FAMILIES)
@pytest.mark.parametrize("c", Q.CASES, ids=Q.case_id)
def test_exact_profile_gives_the_float64_sum(hip, c, family):
    d = Q.inputs(c, family, "exact")
    for acc in (False, True):
        got, ref = Q.run(hip, d, acc, cuda), Q.reference(d, acc)
        assert Q.exact(got, ref), (acc, float((got.double() - ref[0]).abs().max()))


@pytest.mark.parametrize("family", Q.FAMILIES)
@pytest.mark.parametrize("c", Q.CASES, ids=Q.case_id)
def test_general_profile_within_the_derived_bound(hip, c, family):
    d = Q.inputs(c, family, "general")
    for acc in (False, True):
        w = Q.ratio(Q.run(hip, d, acc, cuda), Q.reference(d, acc))
        print(f"F64WORST qk_norm_wgrad {family} {Q.case_id(c)} accumulate={int(acc)}: {w:.4f}")
        assert w <= 1.0, (acc, w)


@pytest.mark.parametrize("family", Q.FAMILIES)
def test_bad_arguments_return_the_error_code(hip, family):
    from ps_slm_amd.ops import TasuOpError
    M, H, G = 3, 2, 1
    LD = (H + 2 * G) * Q.HD
    dt = BF if family == "bf16" else F32
    step = 16 // torch.empty(0, dtype=dt).element_size()           # elements per 16 bytes
    dq, pre = torch.zeros(M * LD + 2 * step, dtype=dt).cuda(), torch.zeros(M * LD + 2 * step, dtype=dt).cuda()
    rstd = torch.ones(M, H + G).cuda()
    dwq, dwk, ws = Q.nan(Q.HD).cuda(), Q.nan(Q.HD).cuda(), Q.nan(Q.WS_FLOATS + 8).cuda()
    flat = lambda t, off=0: t[off:off + M * LD].view(M, LD)                    # noqa: E731  (off = 1: off a 16-byte boundary)
    op = hip.qk_norm_wgrad if family == "bf16" else hip.f32_qk_norm_wgrad

    def call(**k):
        return op(k.get("dq", flat(dq)), k.get("pre", flat(pre)), k.get("rstd", rstd), k.get("dwq", dwq), k.get("dwk", dwk),
                  k.get("ws", ws[:Q.WS_FLOATS]), k.get("M", M), k.get("H", H), k.get("G", G))

    def refused(**k):
        with pytest.raises(TasuOpError):
            call(**k)
        torch.cuda.synchronize()
        for t in (dwq, dwk, ws):
            assert Q.untouched(t.cpu()), "a refused call wrote an output"

    for name in ("dq", "pre", "rstd", "dwq", "dwk", "ws"):
        refused(**{name: None})
    refused(dq=flat(dq, 1))
    refused(pre=flat(pre, 1))
    refused(ws=ws[1:1 + Q.WS_FLOATS])
    refused(ws=ws[:Q.WS_FLOATS - 1])                                           # one float short
    refused(H=3, G=2)                                                          # H % G
    refused(M=0)
    refused(G=0)
    refused(M=(0x7fffffff // (16 if family == "bf16" else 32)) // (H + 2 * G) + 1)      # over the sibling kernels' unit limit
    refused(pre=flat(dq))                                                      # dqkv == pre
    call()                                                                     # ... and the same buffers are served
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dwq).all()) and bool(torch.isfinite(dwk).all())
