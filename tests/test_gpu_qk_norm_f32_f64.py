"""Qwen3's per-head q/k RMSNorm in the fp32 family -- tasu_f32_qk_norm_rope, tasu_f32_qk_norm_bwd (csrc/qk_norm.hip) and
tasu_f32_gemm_qkv_norm_rope (csrc/fp32.hip) -- through HipOps against the float64 statements of tests/qk_norm_f32_ref64.py, element
by element (|err| <= 1.0 x E; the statements' own checks and the mutants: tests/test_qk_norm_f32_ref64_cpu.py).

  forward / backward   M in {1, 3, 17, 64, 65} x (H, G) in {(2, 1), (3, 3), (12, 2), (16, 8)} -- (row, head) counts that are no
                       multiple of a block's 8 heads among them -- on N(0, 1) heads, heads scaled by 1e4 and 1e-4, an all-zero head
                       (r = rsqrt(eps), zeros out) and a one-hot head; out != pre with rstd and out == pre without; the v block bit
                       for bit; every call twice, equal bits
  append               with a cache the cells [m, slot[m]] hold the bits of out's k and v, every other cell keeps its NaN pattern,
                       and out (the appended k with it) has the bits of the call without a cache; in-range slots only (the guard for
                       a slot outside [0, ctx) is reviewed by reading: `slot_ok` in both kernels)
  fused                tasu_f32_gemm_qkv_norm_rope bit for bit against tasu_f32_gemm_nt + tasu_f32_qk_norm_rope, qkv and cache: on the
                       K-split route (M = 1, 5, 64 at K = 256: the tile kernel's slabs, asserted through the restated split), unsplit
                       (M = 80, no workspace) and once on the streaming kernel with fragment-order weights (K = 2048, (16, 8), M = 16,
                       tasu_f32_gemm_streams == 1); within E of the float64 statement

Every output, workspace and cache starts as NaN, every operand has NaN guard rows behind it; everything outside what a call owes
must keep its bits.

Measured on MI355X (25 tests, 1.4 s for the file; the F64WORST lines), largest |err| / E, kernel / the torch fp32 restatement on the
CPU: f32_qk_norm_rope 0.350 / 0.402, f32_qk_norm_bwd 0.894 / 0.894, f32_gemm_qkv_norm_rope 0.018 / 0.046."""
import pytest
import torch

import qk_norm_f32_ref64 as R
from f32_ref64 import tile_ksplit

pytestmark = pytest.mark.gpu
HD = R.HD


@pytest.fixture(scope="module")
def hip():
    from ps_slm_amd.ops import HipOps
    return HipOps()


def cuda(t):
    return t.cuda()


def sync():
    torch.cuda.synchronize()


_worst = {}


def hold(op, case, got, ref):
    w = R.check(got, ref, f"{op} {R.case_id(case)}")
    _worst[op] = max(_worst.get(op, 0.0), w)
    print(f"F64WORST {op} {R.case_id(case)} |err| / E {w:.3f} (largest so far for {op}: {_worst[op]:.3f})")


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_forward_backward_and_append(hip, shape):
    for p in R.PROFILES:
        c = R.Case(*shape, p)
        d = R.inputs(c)
        plain = R.run_fwd(hip, d, cuda, sync, alias=False, want_rstd=True)
        hold("f32_qk_norm_rope", c, plain, R.fwd_reference(d))
        inplace = R.run_fwd(hip, d, cuda, sync, alias=True, want_rstd=False)
        hold("f32_qk_norm_rope", c, inplace, R.fwd_reference(d, want_rstd=False))
        hold("f32_qk_norm_bwd", c, R.run_bwd(hip, d, cuda, sync), R.bwd_reference(d))
        # the append: run_fwd checks the caches cell by cell against out; out itself against the calls without a cache
        for alias in (False, True):
            cached = R.run_fwd(hip, d, cuda, sync, alias=alias, want_rstd=not alias, cache=True)
            for k in ("qk", "v"):
                R.same_bits(cached[k], plain[k], f"f32_qk_norm_rope {R.case_id(c)}: {k} with a cache against without")
                R.same_bits(inplace[k], plain[k], f"f32_qk_norm_rope {R.case_id(c)}: {k} in place against out of place")
        if p == "special":
            M = c.M
            assert bool((plain["qk"].view(M, -1, HD)[M - 1, 0] == 0).all())


@pytest.mark.parametrize("M", [1, 5, 64])
def test_fused_against_unfused_on_the_k_split_route(hip, M):
    c = R.Fused(M, 2, 1, 256, M == 5, True, True)
    N = (c.H + 2 * c.G) * HD
    assert tile_ksplit(M, N, c.K, 16 * 64 * N) > 1 and hip.lib.tasu_f32_gemm_streams(M, N, c.K, 16 * 64 * N) == 0      # the slab route
    d = R.fused_inputs(c)
    one, again, two = R.run_fused(hip, d, cuda, sync), R.run_fused(hip, d, cuda, sync), R.run_fused(hip, d, cuda, sync, unfused=True)
    for k in one:
        R.same_bits(one[k], two[k], f"fused against unfused {R.case_id(c)}, {k}")
        R.same_bits(one[k], again[k], f"fused {R.case_id(c)} second run, {k}")
    hold("f32_gemm_qkv_norm_rope", c, {"qkv": one["qkv"]}, R.fused_reference(d))


def test_fused_against_unfused_on_the_unsplit_route(hip):
    c = R.Fused(80, 2, 1, 256, False, False, True)
    N = (c.H + 2 * c.G) * HD
    assert tile_ksplit(c.M, N, c.K, 0) == 1
    d = R.fused_inputs(c)
    one, two = R.run_fused(hip, d, cuda, sync), R.run_fused(hip, d, cuda, sync, unfused=True)
    for k in one:
        R.same_bits(one[k], two[k], f"fused against unfused {R.case_id(c)}, {k}")
    hold("f32_gemm_qkv_norm_rope", c, {"qkv": one["qkv"]}, R.fused_reference(d))


def test_fused_against_unfused_on_the_streaming_kernel(hip):
    """K = 2048, (H, G) = (16, 8): the 32 MB q|k|v matrix of Qwen3-1.7B at 16 rows, fragment-order weights"""
    M, H, G, K = 16, 16, 8, 2048
    N = (H + 2 * G) * HD
    assert hip.lib.tasu_f32_gemm_streams(M, N, K, 16 * 64 * N) == 1
    c = R.Fused(M, H, G, K, False, True, True)
    g = R.gen(31, M, N, K)
    d = dict(a=torch.randn(M, K, generator=g), w=torch.randn(N, K, generator=g) * K ** -0.5, bias=None, M=M, H=H, G=G, eps=R.EPS, fused=c)
    d["wq"], d["wk"] = 1.0 + 0.5 * torch.randn(HD, generator=g), 1.0 + 0.5 * torch.randn(HD, generator=g)
    d["cos"], d["sin"] = R.rope_tables(M, g)
    d["slot"] = ((torch.arange(M) * 3 + 1) % R.CTX).to(R.I32)
    frag = hip.f32_to_fragments(d["w"].cuda())
    res = {name: R.run_fused(hip, d, cuda, sync, unfused=unfused, w=w)
           for name, unfused, w in (("fused", False, frag), ("fused rows", False, None), ("unfused", True, frag))}
    for k in res["fused"]:
        R.same_bits(res["fused"][k], res["unfused"][k], f"streamed: fused against unfused, {k}")
        R.same_bits(res["fused"][k], res["fused rows"][k], f"streamed: fragment-order against row-major weights, {k}")
    assert bool(torch.isfinite(res["fused"]["qkv"]).all())
