"""tests/qk_norm_f32_ref64.py against itself on the CPU: the fp32 torch restatement (F32QkTorch) stays within 1.0 x E of the float64
statement of tasu_f32_qk_norm_rope / _bwd / tasu_f32_gemm_qkv_norm_rope on every case the GPU file runs, and each mutant of the
restatement leaves the bound -- the bound is tight enough to see a wrong formula, loose enough for a correct fp32 evaluation in
another summation order."""
import pytest
import torch

import qk_norm_f32_ref64 as R

OPS = R.F32QkTorch()
_worst = {}


def hold(op, case, got, ref):
    w = R.check(got, ref, f"{op} {R.case_id(case)}")
    _worst[op] = max(_worst.get(op, 0.0), w)
    print(f"F64WORST {op} {R.case_id(case)} |err| / E {w:.3f} (largest so far for {op}: {_worst[op]:.3f})")


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_restatement_within_the_bound(shape):
    for p in R.PROFILES:
        c = R.Case(*shape, p)
        d = R.inputs(c)
        hold("f32_qk_norm_rope", c, R.run_fwd(OPS, d, alias=False, want_rstd=True), R.fwd_reference(d))
        hold("f32_qk_norm_rope", c, R.run_fwd(OPS, d, alias=True, want_rstd=False, cache=True), R.fwd_reference(d, want_rstd=False))
        hold("f32_qk_norm_bwd", c, R.run_bwd(OPS, d), R.bwd_reference(d))
        if p == "special":
            got = R.run_fwd(OPS, d)
            M, H = c.M, c.H
            assert bool((got["qk"].view(M, -1, R.HD)[M - 1, 0] == 0).all())                 # the all-zero head: zeros, r = rsqrt(eps)
            assert abs(float(got["rstd"][M - 1, 0]) - R.EPS ** -0.5) <= R.R_E * R.e * R.EPS ** -0.5


FUSED = [R.Fused(5, 2, 1, 256, False, True, True), R.Fused(17, 12, 2, 128, True, True, True), R.Fused(3, 3, 3, 64, False, False, False)]


@pytest.mark.parametrize("case", FUSED, ids=R.case_id)
def test_fused_restatement_within_the_bound(case):
    d = R.fused_inputs(case)
    got = R.run_fused(OPS, d)
    hold("f32_gemm_qkv_norm_rope", case, {"qkv": got["qkv"]}, R.fused_reference(d))
    two = R.run_fused(OPS, d, unfused=True)
    for k in got:
        R.same_bits(got[k], two[k], f"fused against unfused, {k}")


# ------------------------------------------------------------------------------------------------ mutants
class Swapped(R.F32QkTorch):
    def _w(self, wq, wk, H, G):
        return super()._w(wk, wq, H, G)


class NoEps(R.F32QkTorch):
    def _stat(self, x, eps):
        return super()._stat(x, 0.0)


class NormAfterRope(R.F32QkTorch):
    def _head(self, x, w, cos, sin, eps):
        return self._norm(R.rope_eager(x, cos, sin), w, eps)


class MeanOver64(R.F32QkTorch):
    def _stat(self, x, eps):
        return torch.rsqrt(x[..., :64].pow(2).mean(-1, keepdim=True) + eps)


class NoMeanTerm(R.F32QkTorch):
    def _dpre(self, wg, xn, r):
        return r * wg


class WeightAfterProjection(R.F32QkTorch):
    def f32_qk_norm_bwd(self, dqkv, pre, wq, wk, rstd, M, H, G):
        x = pre[:M].view(M, H + 2 * G, R.HD)[:, :H + G]
        g = dqkv[:M].view(M, H + 2 * G, R.HD)
        r = rstd[:M].view(M, H + G, 1)
        g[:, :H + G] = self._w(wq, wk, H, G) * self._dpre(g[:, :H + G].clone(), x * r, r)


MUTANT_CASE = R.Case(17, 12, 2, "scales")                       # (the 1e-4 heads: where eps decides the result)


@pytest.mark.parametrize("mutant", [Swapped, NoEps, NormAfterRope, MeanOver64], ids=lambda m: m.__name__)
def test_forward_mutants_leave_the_bound(mutant):
    d = R.inputs(MUTANT_CASE)
    assert R.worst_of(R.run_fwd(OPS, d), R.fwd_reference(d)) <= 1.0
    w = R.worst_of(R.run_fwd(mutant(), d), R.fwd_reference(d))
    print(f"mutant {mutant.__name__}: {w:.3g} E")
    assert w > 1.0


@pytest.mark.parametrize("mutant", [NoMeanTerm, WeightAfterProjection], ids=lambda m: m.__name__)
def test_backward_mutants_leave_the_bound(mutant):
    d = R.inputs(MUTANT_CASE)
    assert R.worst_of(R.run_bwd(OPS, d), R.bwd_reference(d)) <= 1.0
    w = R.worst_of(R.run_bwd(mutant(), d), R.bwd_reference(d))
    print(f"mutant {mutant.__name__}: {w:.3g} E")
    assert w > 1.0
