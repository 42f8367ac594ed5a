"""tests/qk_norm_ref64.py before a GPU sees it: the float32 torch restatement of the three operators (tests/qwen3_ops.py) stays
inside the float64 reference's per-element bound on every case, and each of four mistakes leaves it -- eps omitted, the rounding of
xh omitted, the q and k weights exchanged, RoPE before the norm -- so the bound means something."""
import pytest
import torch

import qk_norm_ref64 as Q
from fake_ops import _bf
from qwen3_ops import Qwen3FakeOps

HD = Q.HD


class Mutant(Qwen3FakeOps):
    """the double's forward with one mistake"""

    def __init__(self, kind):
        super().__init__()
        self.kind = kind

    def qk_norm_rope_fwd(self, pre, wq, wk, cos, sin, out, rstd, M, H, G, eps):
        kind = self.kind
        if kind == "swap":
            wq, wk = wk, wq
        x = pre[:M].view(M, H + 2 * G, HD)[:, :H + G].float()
        c, s = cos[:M].view(M, 1, 64), sin[:M].view(M, 1, 64)
        if kind == "rope-first":
            x = self._rot(x, c, s)
        r = torch.rsqrt(x.pow(2).mean(-1) + (0.0 if kind == "no-eps" else eps))
        t = x * r[..., None]
        w = torch.cat([wq.view(1, HD).expand(H, HD), wk.view(1, HD).expand(G, HD)])[None]
        y = w * (t if kind == "no-round" else _bf(t).float())
        o = out[:M].view(M, H + 2 * G, HD)
        o[:, H + G:] = pre[:M].view(M, H + 2 * G, HD)[:, H + G:]
        o[:, :H + G] = _bf(y if kind == "rope-first" else self._rot(y, c, s))
        if rstd is not None:
            rstd[:M].view(M, H + G).copy_(r)


@pytest.fixture(scope="module", params=Q.CASES, ids=Q.case_id)
def case(request):
    d = Q.inputs(request.param)
    return d, Q.fwd_reference(d), Q.bwd_reference(d)


def test_inputs_hold_what_the_reference_is_owed(case):
    d, ref, _ = case
    M, H, G = d["M"], d["H"], d["G"]
    heads = d["pre"].view(M, H + 2 * G, HD)[:, :H + G].double()
    ms = heads.pow(2).mean(-1)
    assert bool((ms == 0).any()) and bool(((ms > 0) & (ms < 10 * d["eps"])).any()) and bool((ms > 0.5).any())      # zero, eps-sized, N(0, 1)
    assert {0, 1, 4095} <= set(d["pos"].tolist()) and float(d["wq"].min()) < 0 and float(d["wk"].min()) < 0
    qk, E = ref.tol["qk"]
    zero = (ms == 0)[..., None].expand(M, H + G, HD).reshape(M, -1)
    assert bool((qk[zero] == 0).all()) and bool((E[zero] == 0).all()) and bool((E[~zero] > 0).all())
    tie = E > Q.U * qk.abs() * 1.5                               # elements granted the one-ulp move of xh: few
    assert 0 < int(tie.sum()) or M < 64
    assert int(tie.sum()) < 0.01 * E.numel()


def test_float32_restatement_stays_inside_the_bound(case):
    d, fref, bref = case
    ops = Qwen3FakeOps()
    out = Q.run_fwd(ops, d)
    w = Q.check(out, fref, "qk_norm_rope_fwd")
    assert 0 < w <= Q.LIMIT
    Q.check(Q.run_fwd(ops, d, alias=True), fref, "qk_norm_rope_fwd (out == pre)")
    nor = Q.run_fwd(ops, d, want_rstd=False)
    Q.same_bits(nor["qk"], out["qk"], "qk_norm_rope_fwd without rstd")
    assert 0 < Q.check(Q.run_bwd(ops, d), bref, "qk_norm_bwd") <= Q.LIMIT
    for kind in ("first", "last", "mixed"):
        Q.run_append(ops, d, out, 7, kind)


@pytest.mark.parametrize("kind", ["no-eps", "no-round", "swap", "rope-first"])
def test_each_mistake_leaves_the_bound(case, kind):
    d, fref, _ = case
    got = Q.run_fwd(Mutant(kind), d, again=False)
    got = {k: v for k, v in got.items() if k != "rstd" or kind == "no-eps"}
    ref = Q.Ref({k: v for k, v in fref.tol.items() if k in got}, fref.exact)
    assert Q.worst_of(got, ref) > 2 * Q.LIMIT, kind


def test_backward_mistakes_leave_the_bound(case):
    """the weights exchanged, and the projection term left out"""
    d, _, bref = case

    class Swapped(Qwen3FakeOps):
        def qk_norm_bwd(self, dqkv, pre, wq, wk, rstd, M, H, G):
            super().qk_norm_bwd(dqkv, pre, wk, wq, rstd, M, H, G)

    class NoProjection(Qwen3FakeOps):
        def qk_norm_bwd(self, dqkv, pre, wq, wk, rstd, M, H, G):
            g = dqkv[:M].view(M, H + 2 * G, HD)
            w = torch.cat([wq.view(1, HD).expand(H, HD), wk.view(1, HD).expand(G, HD)])[None]
            g[:, :H + G] = _bf(rstd[:M].view(M, H + G, 1) * w * g[:, :H + G].float())

    for ops in (Swapped(), NoProjection()):
        assert Q.worst_of(Q.run_bwd(ops, d, again=False), bref) > 2 * Q.LIMIT, type(ops).__name__
