"""CPU checks of the float64 attention reference and its elementwise bound (tests/attn_ref64.py), which
tests/test_gpu_attention_f64.py holds the HIP kernels to:

* the reference is right: its gradients agree with torch.autograd on an explicit float64 softmax attention to 1e-12;
* the reference's bound holds for the torch double alone: tests/fake_ops.py restates the kernels' rounding points in fp32 and
  stays within 1.0 x E on every case of the GPU list with S <= 1100;
* the check has teeth: a backward that loses the last live key, one that loses the last live query row and a double that
  truncates to bf16 instead of rounding are all rejected -- and the first of them passes the tensor-wide
  max|a-b| / max|b| < 2e-2 of tests/test_gpu_ops.py, which is why the elementwise metric exists."""
import pytest
import torch

import attn_ref64 as R
import fake_ops
from fake_ops import FakeOps

HD = R.HD
F64 = torch.float64


@pytest.fixture(scope="module")
def fake():
    return FakeOps()


def rel_err(a, b):
    """the tensor-wide metric of tests/test_gpu_ops.py"""
    a, b = a.float(), b.float()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


# ------------------------------------------------------------------------------------------------ the reference is right
def autograd_attention(inp):
    """explicit float64 softmax attention with the rotated q | k | v as leaves: (out [B, S, H, 128], lse [B, S, H, 1], grad)"""
    B, S, H, G = inp["B"], inp["S"], inp["H"], inp["G"]
    rep = H // G
    x = inp["qkv"].view(B, S, H + 2 * G, HD).to(F64).requires_grad_(True)
    q = x[:, :, :H].permute(0, 2, 1, 3)
    k = x[:, :, H:H + G].permute(0, 2, 1, 3).repeat_interleave(rep, 1)
    v = x[:, :, H + G:].permute(0, 2, 1, 3).repeat_interleave(rep, 1)
    allow = inp["km"][:, :S].bool()[:, None, None, :].expand(B, 1, S, S)
    if inp["causal"]:
        allow = allow & torch.tril(torch.ones(S, S, dtype=torch.bool))
    sc = (q @ k.transpose(-1, -2)) * inp["scale"]
    m = sc.masked_fill(~allow, -1e300).amax(-1, keepdim=True).detach()
    e = torch.where(allow, torch.exp(torch.where(allow, sc - m, torch.zeros_like(sc))), torch.zeros_like(sc))
    l = e.sum(-1, keepdim=True)
    some = l > 0
    out = (e / torch.where(some, l, torch.ones_like(l))) @ v
    lse = torch.where(some, m + torch.log(torch.where(some, l, torch.ones_like(l))), torch.zeros_like(l))
    (out * inp["dout"].view(B, S, H, HD).to(F64).permute(0, 2, 1, 3)).sum().backward()
    return out.detach().permute(0, 2, 1, 3), lse.detach().permute(0, 2, 1, 3), x.grad


@pytest.mark.parametrize("case", [R.Case(2, 100, 4, 2, "right", True, "n01", False), R.Case(3, 65, 16, 2, "left", True, "peaked", False),
                                  R.Case(2, 130, 10, 2, "holes", False, "n01", False), R.Case(2, 63, 8, 2, "empty0", True, "n01", False),
                                  R.Case(1, 70, 28, 4, "none", False, "peaked", False), R.Case(2, 1, 4, 2, "holes", True, "n01", False),
                                  R.Case(1, 257, 4, 2, "left", True, "n01", True)], ids=R.case_id)
def test_reference_agrees_with_autograd(case):
    """cos = 1, sin = 0: the rotated q | k | v ARE the leaves (un-rotating and re-rotating through the fp32 tables would cost
    1e-7: they are orthonormal only to fp32)"""
    inp = R.make_inputs(case)
    inp["cos"], inp["sin"] = torch.ones_like(inp["cos"]), torch.zeros_like(inp["sin"])
    ref = R.reference_of(inp)
    out, lse, grad = autograd_attention(inp)
    for name, a, b in (("out", ref.out, out), ("lse", ref.lse, lse), ("dqkv", ref.dqkv, grad)):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), name
    # rows nobody may touch have a zero bound: masked keys' dk / dv under live-only dout, rows without a visible key
    dead = ref.E_out.amax((-1, -2)) == 0
    assert bool((ref.out[dead] == 0).all()) and bool((ref.lse[dead] == 0).all())
    assert bool((ref.dqkv[ref.E_dqkv == 0] == 0).all())


def test_reference_unrotates_with_the_fp32_table():
    """with the real fp32 table the reference's dq / dk are the un-rotated gradients: rotating them forward again gives the
    rotated-space gradients back (to the table's own orthonormality, 1e-6 relative)"""
    inp = R.make_inputs(R.Case(2, 100, 4, 2, "right", True, "n01", False))
    ref = R.reference_of(inp)
    plain = dict(inp, cos=torch.ones_like(inp["cos"]), sin=torch.zeros_like(inp["sin"]))
    rot = R.reference_of(plain)
    B, S, H, G = inp["B"], inp["S"], inp["H"], inp["G"]
    c, s = inp["cos"].view(B, S, 1, 64).double(), inp["sin"].view(B, S, 1, 64).double()
    x = ref.dqkv[:, :, :H + G]
    back = torch.cat([x[..., :64] * c - x[..., 64:] * s, x[..., 64:] * c + x[..., :64] * s], -1)
    assert float((back - rot.dqkv[:, :, :H + G]).abs().max()) < 1e-5 * float(rot.dqkv.abs().max())
    assert torch.equal(ref.dqkv[:, :, H + G:], rot.dqkv[:, :, H + G:]) and torch.equal(ref.out, rot.out)
    assert bool((ref.E_dqkv[:, :, :H] >= R.U * ref.dqkv[:, :, :H].abs()).all())


# ------------------------------------------------------------------------------------------------ the double inside the bound
CPU_CASES = [c for c in R.CASES if c.S <= 1100]


@pytest.mark.parametrize("case", CPU_CASES, ids=R.case_id)
def test_double_stays_inside_the_bound(fake, case):
    """forward -> attn_bwd_fused of the double, at limit 1.0 (the kernels get 1.1) on every row < S, dead rows included"""
    inp = R.make_inputs(case)
    ref = R.reference_of(inp)
    B, S, H, G = case.B, case.S, case.H, case.G
    out, lse, dqkv = R.run_double(fake, inp)
    R.assert_within(out.view(B, S, H, HD), ref.out, ref.E_out, 1.0, "out")
    R.assert_within(R.lse_rows(lse, B, S, H), ref.lse, ref.E_lse, 1.0, "lse")
    for name, got, want, E in R.blocks(dqkv, ref, B, S, H, G):
        R.assert_within(got, want, E, 1.0, name)


# ------------------------------------------------------------------------------------------------ the check has teeth
MUTANT_CASES = [R.Case(2, 256, 12, 2, "none", True, "n01", False), R.Case(1, 628, 12, 2, "none", True, "n01", False),
                R.Case(2, 256, 12, 2, "right", True, "n01", False), R.Case(1, 628, 12, 2, "right", True, "n01", False)]


@pytest.fixture(scope="module")
def mutant_refs(fake):
    """case -> (inputs, reference, the unmutated double's results)"""
    res = {}
    for c in MUTANT_CASES:
        inp = R.make_inputs(c)
        res[c] = (inp, R.reference_of(inp), R.run_double(fake, inp))
    return res


@pytest.mark.parametrize("case", MUTANT_CASES, ids=R.case_id)
def test_a_backward_that_drops_the_last_live_key_is_rejected(fake, mutant_refs, case):
    inp, ref, good = mutant_refs[case]
    B, S, H, G = case.B, case.S, case.H, case.G
    km = inp["km"].clone()
    last = int(torch.nonzero(km[0, :S])[-1])
    km[0, last] = 0
    _, _, dqkv = R.run_double(fake, inp, km_bwd=km)
    res = {name: R.check_within(got, want, E, R.LIMIT, name) for name, got, want, E in R.blocks(dqkv, ref, B, S, H, G)}
    for name in ("dk", "dv"):
        assert not res[name].ok and res[name].worst > 5.0, res[name].message
        assert f"(b=0, s={last}, " in res[name].message and f"tile {last // 64} " in res[name].message     # ... and names the lost row
    # why the elementwise metric exists: a whole dK / dV row gone, and the old tensor-wide metric stays inside its 2e-2
    lo = 0
    for name, hi in (("dq", H * HD), ("dk", (H + G) * HD), ("dv", (H + 2 * G) * HD)):
        old = rel_err(dqkv[:, lo:hi], good[2][:, lo:hi])
        print(f"{R.case_id(case)} {name}: old metric {old:.4f}, worst err / E {res[name].worst:.1f}")
        assert old < 2e-2, (name, old)
        lo = hi


@pytest.mark.parametrize("case", MUTANT_CASES, ids=R.case_id)
def test_a_backward_that_drops_the_last_live_query_row_is_rejected(fake, mutant_refs, case):
    """the row's dO zeroed for the backward: ds and P^T dO lose the row, so dq of the row and its share of dk / dv are gone"""
    inp, ref, _ = mutant_refs[case]
    B, S, H, G = case.B, case.S, case.H, case.G
    last = int(torch.nonzero(inp["km"][0, :S])[-1])
    dout = inp["dout"].clone()
    dout[last] = 0                                               # batch 0
    _, _, dqkv = R.run_double(fake, inp, dout_bwd=dout)
    for name, got, want, E in R.blocks(dqkv, ref, B, S, H, G):
        c = R.check_within(got, want, E, R.LIMIT, name)
        print(f"{R.case_id(case)} {name}: worst err / E {c.worst:.1f}")
        assert not c.ok and c.worst > 5.0, c.message
        if name == "dq":
            assert f"(b=0, s={last}, " in c.message


def _truncate(x):
    """fp32 -> bf16 by dropping the low 16 bits (round toward zero)"""
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


@pytest.mark.parametrize("case", [R.Case(2, 256, 12, 2, "none", True, "n01", False), R.Case(1, 628, 12, 2, "right", True, "n01", False),
                                  R.Case(2, 130, 10, 2, "left", False, "peaked", False)], ids=R.case_id)
def test_a_double_that_truncates_instead_of_rounding_is_rejected(fake, monkeypatch, case):
    """both checks of the GPU file see it: elements beyond 1.1 x E, and rms(err / E) far beyond 1.5 x the rounding double's"""
    inp = R.make_inputs(case)
    ref = R.reference_of(inp)
    B, S, H, G = case.B, case.S, case.H, case.G
    want_rms = R.double_rms(fake, inp, ref)
    monkeypatch.setattr(fake_ops, "_bf", _truncate)
    out, _, dqkv = R.run_double(fake, inp)
    res = {"out": R.check_within(out.view(B, S, H, HD), ref.out, ref.E_out, R.LIMIT, "out")}
    res.update({name: R.check_within(got, want, E, R.LIMIT, name) for name, got, want, E in R.blocks(dqkv, ref, B, S, H, G)})
    for name, c in res.items():
        print(f"{R.case_id(case)} {name}: worst err / E {c.worst:.2f}, rms {c.rms:.4f} = {c.rms / want_rms[name]:.2f} x the double's")
        assert c.rms > 2.0 * want_rms[name], (name, c.rms, want_rms[name])
    assert not all(c.ok for c in res.values())
