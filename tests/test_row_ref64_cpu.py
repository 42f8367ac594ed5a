"""CPU checks of the float64 references of the row-reduction kernels and their bounds (tests/row_ref64.py), which
tests/test_gpu_row_f64.py holds the HIP kernels to:

* the bounds are honest: the torch double (tests/fake_ops.py, fp32 torch on the CPU) stays within 1.0 x E on every case of the
  shared lists and gives the bits of the exact-integer profiles.  Largest |err| / E of the double: RMSNorm forward 0.996, backward
  0.996, LayerNorm 0.995, layernorm_bwd_params 0.16, colsum 0.003, cross-entropy 0.991, ce_reduce 0.74, scale_softmax_rows 0.995,
  softmax_bwd_rows 0.84, softmax_rows 0.49, psd_logit_stats 0.13, psd_gather_softmax 0.71 (a bf16 rounding alone reaches
  1.0 x u |y| just above a power of two);
* the references are the operations: each agrees with a plain torch.float64 (autograd) formulation at 1e-12 relative;
* the checks have teeth.  Mutants through the double, each with its score under the tensor-wide metric of tests/test_gpu_ops.py
  (max|a-b| / max|b|) against that test's limit, then its worst |err| / E (MUTANT lines of this file; `inf`: a wrong integer or a
  non-zero where the result is exactly 0):

      sum of squares without the last 4 columns, D = 3584     y 0.0063 (passes 1e-2), rstd 1.7e-3 (FAILS 1e-5)   new 816 x E (rstd)
          -- no blind spot of the old suite where rstd is returned; the decode norm returns y alone:             new 1.45 x E (y)
      bf16 truncation instead of rounding in y, D = 512       0.0066 (passes 1e-2)                                new 1.98 x E, rms 2.00 x
      one-pass LayerNorm variance, offset rows, D = 512 / 1028 0.087 / 0.049 (FAILS 1e-2)                          new 67 / 40 x E
          -- on the old test's posterior-like rows it scores 0.0 and 0.95 x E: those rows cannot show it, offset rows show it
             to either metric; recorded as caught by both
      cross-entropy sum over ldv columns, (1000, 1024)         loss 3.1e-5 (passes 1e-4), dlogits 6.1e-4 (passes)  new 80 x E
      argmax takes the last index on ties                      equal on N(0, 1) rows (passes)                       new: 6 of 6 wrong integers
      dx ignores accumulate, base 2^-16 N(0, 1)                1.6e-5 (passes 1e-4)                                 new 523 x E
      scale_softmax rounds s / denom after the subtraction     0.0051 (passes 1e-2)                                 new 14.6 x E
      PSD rescale without sum *= exp(best - cm), V = 25055     1 / sum 0.89 on late-maximum rows, 0.80 on N(0, 1)
                                                               rows (FAILS any limit): caught by both               new 8e4 x E"""
import pytest
import torch
import torch.nn.functional as F

import fake_ops
import row_ref64 as R
from fake_ops import FakeOps

F64, F32, BF, I32 = torch.float64, torch.float32, torch.bfloat16, torch.int32


@pytest.fixture(scope="module")
def fake():
    return FakeOps()


def rel_err(a, b):
    """the tensor-wide metric of tests/test_gpu_ops.py"""
    a, b = a.float(), b.float()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _truncate(x):
    """fp32 -> bf16 by dropping the low 16 bits (round toward zero)"""
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def close(a, b, what):
    err = float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
    assert err < 1e-12, (what, err)


# ------------------------------------------------------------------------------------------------ 1. the double inside the bounds
FAMILIES = {
    "rmsnorm_fwd": (R.RMS_FWD_CASES, R.rms_fwd_inputs, R.rms_fwd_reference, R.run_rms_fwd),
    "rmsnorm_bwd": (R.RMS_BWD_CASES, R.rms_bwd_inputs, R.rms_bwd_reference, R.run_rms_bwd),
    "layernorm_fwd": (R.LN_CASES, R.ln_inputs, R.ln_reference, R.run_ln),
    "layernorm_bwd_params": (R.LNB_CASES, R.col_inputs, R.col_reference, R.run_col),
    "colsum": (R.COLSUM_CASES, R.col_inputs, R.col_reference, R.run_col),
    "ce_fwd_bwd": (R.CE_CASES, R.ce_inputs, R.ce_reference, R.run_ce),
    "ce_reduce": ([c for c in R.CE_REDUCE_CASES if c.profile != "ignored"], R.red_inputs, R.red_reference, R.run_red),
    "scale_softmax_rows": (R.SM_CASES, R.sm_inputs, lambda d: R.sm_reference(d)[0], R.run_sm_fwd),
    "softmax_bwd_rows": (R.SM_CASES, R.sm_inputs, lambda d: R.sm_reference(d)[1], R.run_sm_bwd),
    "softmax_rows": (R.SR_CASES, R.sr_inputs, R.sr_reference, R.run_sr),
    "psd_logit_stats": (R.PSD_CASES, R.psd_inputs, lambda d: R.psd_reference(d)[0], R.run_psd_stats),
    "psd_gather_softmax": (R.PSD_CASES, R.psd_inputs, lambda d: R.psd_reference(d)[1], R.run_psd_gather),
}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_double_stays_inside_the_bound_on_every_case(fake, family):
    cases, inputs, reference, run = FAMILIES[family]
    worst = 0.0
    for c in cases:
        d = inputs(c)
        ref, out = reference(d), run(fake, d)
        if "y_raw" in out:                                       # the double writes the fragment-order form row-major
            assert R.untouched(out["y_raw"][d["n"]:])
            out, ref = {"y": out["y_raw"][:d["n"]]}, R.Ref({"y": ref.tol["y"]}, {})
        worst = max(worst, R.check(out, ref, f"double {family} {R.case_id(c)}"))
    print(f"DOUBLE {family}: {len(cases)} cases, largest |err| / E {worst:.3f}")
    assert worst <= R.LIMIT


def test_ce_reduce_over_nothing_is_nan(fake):
    d = R.red_inputs(R.RedCase(257, "ignored"))
    out = R.run_red(fake, d)
    assert float(out["count"]) == 0.0 and bool(torch.isnan(out["out"]).all())


def test_case_lists_sit_on_the_kernels_switches():
    assert {c.D for c in R.RMS_FWD_CASES} >= {4, 252, 256, 260, 512, 1028, 1536, 3584}
    assert {c.M for c in R.RMS_FWD_CASES if c.form == "plain"} >= {1, 64, 65, 67} and {c.M for c in R.RMS_BWD_CASES} >= {1, 5, 64, 65, 67}
    assert {(c.acc, c.bf) for c in R.RMS_BWD_CASES if c.form == "plain"} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    kern = {(c.V, c.ldv, R.ce_kernel_of(c)) for c in R.CE_CASES}
    assert {(8192, 8192, "reg"), (163840, 163840, "reg"), (163841, 163848, "online"), (8200, 8200, "online"), (8200, 8200, "reg"),
            (9001, 9088, "online"), (9001, 9088, "reg"), (151936, 151936, "online"), (151936, 151936, "reg")} <= kern
    assert all(c.M <= 3 for c in R.CE_CASES if c.V >= 151936)
    assert 163840 // 8 == R.REG_CHUNKS                            # all 20 chunks of every thread
    assert R.walk_columns(3584) == [0, 1, 3, 4, 255, 256, 257, 3324, 3580, 3583]
    assert R.tie_pairs(9001, 1024)[-1] == (59, 8251) and R.tie_pairs(8200, 256)[-1] == (59, 2107)


# ------------------------------------------------------------------------------------------------ 2. the references are the operations
def test_rmsnorm_reference_is_the_autograd_formula():
    d = R.rms_bwd_inputs(R.BwdCase("plain", 5, 260, 1, 1, "n01"))
    x = d["x"].to(F64).requires_grad_()
    w = d["w"].to(F64)
    y = w * x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + R.EPS_RMS)
    (g,) = torch.autograd.grad(y, x, d["dy"].to(F64))
    ref = R.rms_bwd_reference(dict(d, rstd=torch.rsqrt(d["x"].to(F64).pow(2).mean(-1) + R.EPS_RMS)))     # the unrounded rstd
    close(ref.tol["dx"][0], d["base"].to(F64) + g, "rmsnorm dx")
    f = R.rms_fwd_inputs(R.RmsCase("plain", 5, 260, "scaled"))
    xf = f["x"].to(F64)
    close(R.rms_fwd_reference(f).tol["y"][0], f["w"].to(F64) * xf / (xf.pow(2).mean(-1, keepdim=True) + R.EPS_RMS).sqrt(), "rmsnorm y")


def test_layernorm_reference_is_layer_norm():
    for c in (R.LnCase(5, 203, 256, 256, 0, 1, 1, "offset"), R.LnCase(5, 1028, 1028, 1028, 0, 0, 1, "posterior")):
        d = R.ln_inputs(c)
        ref = R.ln_reference(d)
        xs = d["x"][:, :c.D].to(F64)
        want = F.layer_norm(xs, (c.D,), d["gamma"].to(F64), d["beta"].to(F64), R.EPS_LN)
        close(ref.tol["y"][0][:, :c.D], want, "layernorm y")
        assert float(ref.tol["y"][0][:, c.D:].abs().sum()) == 0.0
    d = R.col_inputs(R.ColCase("lnb", 17, 203, "n01"))
    ga, be = torch.ones(203, dtype=F64, requires_grad=True), torch.zeros(203, dtype=F64, requires_grad=True)
    xs = d["x"][:, :203].to(F64)
    xh = (xs - d["mean"].to(F64)[:, None]) * d["rstd"].to(F64)[:, None]
    dg, db = torch.autograd.grad(xh * ga + be, (ga, be), d["dy"][:, :203].to(F64))
    ref = R.col_reference(d)
    close(ref.tol["dgamma"][0][0], dg, "dgamma")
    close(ref.tol["dbeta"][0][0], db, "dbeta")


def test_cross_entropy_reference_is_cross_entropy():
    for c in (R.CeCase(6, 1000, 1024, 1, "two", "n01"), R.CeCase(6, 9001, 9088, 0, "two", "peak")):
        d = R.ce_inputs(c)
        ref = R.ce_reference(d)
        x = d["logits"][:, :c.V].to(F64).requires_grad_()
        rows = F.cross_entropy(x, d["labels"].long(), ignore_index=-100, reduction="none")
        close(ref.tol["row_loss"][0][:, 0], rows.detach(), "row_loss")
        (g,) = torch.autograd.grad(F.cross_entropy(x, d["labels"].long(), ignore_index=-100, reduction="sum") * float(d["inv"][0]), x)
        close(ref.tol["dlogits"][0][:, :c.V], g, "dlogits")
        assert float(ref.tol["dlogits"][0][:, c.V:].abs().sum()) == 0.0


def test_softmax_references_are_softmax():
    d = R.sm_inputs(R.SmCase(5, 1003, 1008, 0, R.SQ96, 1, "n01"))
    fwd, bwd = R.sm_reference(d)
    t = d["t"].to(F64).requires_grad_()
    P = torch.softmax(t, -1)
    close(fwd.tol["p"][0][:, :1003], P.detach(), "p")
    ref_stats = dict(d, stats_in=fwd.tol["stats"][0])                                                     # the unrounded statistics
    (g,) = torch.autograd.grad(P, t, d["dp"][:, :1003].to(F64))
    close(R.sm_reference(ref_stats)[1].tol["ds"][0][:, :1003], g / d["denom32"], "ds")
    s = R.sr_inputs(R.SrCase(5, 257, 260, 0, "n01"))
    close(R.sr_reference(s).tol["y"][0][:, :257], torch.softmax(s["x"][:, :257].to(F64), -1), "softmax_rows")
    p = R.psd_inputs(R.PsdCase(203, "n01"))
    x3 = p["logits"].view(R.PSD_B, R.PSD_BSTRIDE, -1)[:, :R.PSD_T, :203].to(F64)
    post = torch.softmax(x3, -1)
    m = x3.amax(-1)
    stats, gather = R.psd_reference(dict(p, fstat_in=torch.stack([m, 1 / torch.exp(x3 - m[..., None]).sum(-1)], -1)))   # unrounded
    close(gather.tol["out"][0][1, :203], post[0, 1:3].mean(0), "psd gather")
    close(stats.tol["fblank"][0][:9, 0], post[0, :, 0], "fblank")


# ------------------------------------------------------------------------------------------------ 3. mutants
def _report(name, old, limit, new):
    print(f"MUTANT {name}: old metric {old:.2e} against {limit:g} ({'passes' if old < limit else 'FAILS'}), worst |err| / E {new:.3g}")


def test_mutant_sum_of_squares_without_the_last_four_columns(fake):
    c = R.RmsCase("plain", 67, 3584, "n01")
    d = R.rms_fwd_inputs(c)
    ref = R.rms_fwd_reference(d)
    good = R.run_rms_fwd(fake, d)
    x, w = d["x"], d["w"]
    r = torch.rsqrt(x[:, :-4].pow(2).sum(-1) / 3584 + R.EPS_RMS)
    bad = {"y": (w * (x * r[:, None])).to(BF), "rstd": r[:, None]}
    old_y, old_r = rel_err(bad["y"], good["y"]), rel_err(bad["rstd"], good["rstd"])
    new_r = R.worst_of({"rstd": bad["rstd"]}, R.Ref({"rstd": ref.tol["rstd"]}, {}))
    new_y = R.worst_of({"y": bad["y"]}, R.Ref({"y": ref.tol["y"]}, {}))
    _report("ss without the last 4 columns, y", old_y, 1e-2, new_y)
    _report("ss without the last 4 columns, rstd", old_r, 1e-5, new_r)
    assert old_y < 1e-2 and old_r > 1e-5                         # the old suite sees it where rstd is returned, through rstd alone
    assert new_r > 100 and new_y > R.LIMIT


def test_mutant_truncating_pack(fake, monkeypatch):
    d = R.rms_fwd_inputs(R.RmsCase("plain", 67, 512, "n01"))
    ref = R.rms_fwd_reference(d)
    good = R.run_rms_fwd(fake, d)
    monkeypatch.setattr(fake_ops, "_bf", _truncate)
    bad = R.run_rms_fwd(fake, d)
    old, new = rel_err(bad["y"], good["y"]), R.worst_of(bad, ref)
    r_good, r_bad = R.rms_stat(good["y"], *ref.tol["y"])[0], R.rms_stat(bad["y"], *ref.tol["y"])[0]
    _report("truncating y", old, 1e-2, new)
    print(f"MUTANT truncating y: rms {r_bad:.3f} = {r_bad / r_good:.2f} x the double's {r_good:.3f}")
    assert old < 1e-2 and new > 1.5 and r_bad > R.RMS_RATIO * r_good


def test_mutant_one_pass_variance_on_offset_rows(fake):
    olds, news = [], []
    for D in (512, 1028):
        d = R.ln_inputs(R.LnCase(5, D, D, D, 0, 0, 1, "offset"))
        ref = R.ln_reference(d)
        good = R.run_ln(fake, d)
        x = d["x"][:, :D]
        mu = x.mean(-1, keepdim=True)
        r = torch.rsqrt((x * x).mean(-1, keepdim=True) - mu * mu + R.EPS_LN)
        bad = {"y": ((x - mu) * r * d["gamma"] + d["beta"]).to(BF), "mean": mu, "rstd": r}
        olds.append(rel_err(bad["y"], good["y"]))
        news.append(R.worst_of(bad, ref))
        _report(f"one-pass variance, offset rows, D = {D}", olds[-1], 1e-2, news[-1])
    assert min(news) > 3.0
    p = R.ln_inputs(R.LnCase(5, 512, 512, 512, 0, 0, 1, "posterior"))   # the old test's rows: the one-pass form passes there
    x = p["x"]
    mu = x.mean(-1, keepdim=True)
    y1 = ((x - mu) * torch.rsqrt((x * x).mean(-1, keepdim=True) - mu * mu + R.EPS_LN) * p["gamma"] + p["beta"]).to(BF)
    old = rel_err(y1, R.run_ln(fake, p)["y"])
    _report("one-pass variance, posterior rows", old, 1e-2, R.worst_of({"y": y1}, R.Ref({"y": R.ln_reference(p).tol["y"]}, {})))
    assert old < 1e-2


def test_mutant_cross_entropy_sums_the_pad_columns(fake):
    c = R.CeCase(6, 1000, 1024, 0, "two", "n01")
    d = R.ce_inputs(c)
    ref = R.ce_reference(d)
    good = R.run_ce(fake, d)
    lg0 = d["logits"].clone()
    lg0[:, c.V:] = 0                                             # the pad of tests/test_gpu_ops.py::test_cross_entropy
    rl, rh, dl = torch.zeros(6), torch.zeros(6, dtype=I32), torch.zeros(6, 1024, dtype=BF)
    fake.ce_fwd_bwd(lg0, d["labels"], 6, 1024, rl, rh, None, dl, d["inv"])
    dl[:, c.V:] = 0
    bad = {"row_loss": rl[:, None], "row_hit": rh, "dlogits": dl}
    old_l, old_d = rel_err(bad["row_loss"], good["row_loss"]), rel_err(bad["dlogits"], good["dlogits"])
    new = R.worst_of(bad, ref)
    _report("CE sum over ldv columns, row_loss", old_l, 1e-4, new)
    _report("CE sum over ldv columns, dlogits", old_d, 1e-2, new)
    assert old_l < 1e-4 and old_d < 1e-2 and new > 5.0


def test_mutant_argmax_takes_the_last_index_on_ties(fake):
    last = lambda x: x.shape[-1] - 1 - x.flip(-1).argmax(-1)
    n = R.ce_inputs(R.CeCase(6, 2056, 2056, 1, "two", "n01"))
    xn = n["logits"][:, :2056].float()
    assert torch.equal(last(xn).to(I32), R.ce_reference(n).exact["row_argmax"])          # no ties on N(0, 1) rows: the old check passes
    t = R.ce_inputs(R.CeCase(6, 2056, 2056, 1, "two", "ties"))
    ref = R.ce_reference(t)
    bad = last(t["logits"][:, :2056].float()).to(I32)
    wrong = int((bad != ref.exact["row_argmax"]).sum())
    print(f"MUTANT argmax takes the last index: equal on the N(0, 1) rows, {wrong} of 6 wrong on the tie profile")
    assert wrong == 6 and int(ref.exact["row_argmax"][5]) == 0
    with pytest.raises(AssertionError, match="differ from the exact result"):
        R.same_bits(bad, ref.exact["row_argmax"], "argmax")


def test_mutant_dx_ignores_accumulate(fake):
    d = R.rms_bwd_inputs(R.BwdCase("plain", 5, 256, 1, 1, "n01"))
    d["base"] = d["base"] * 2.0 ** -16                           # small against dx
    ref = R.rms_bwd_reference(d)
    good = R.run_rms_bwd(fake, d)
    assert R.worst_of(good, ref) <= R.LIMIT
    bad = R.run_rms_bwd(fake, dict(d, acc=0))
    old, new = rel_err(bad["dx"], good["dx"]), R.worst_of(bad, ref)
    _report("dx ignores accumulate", old, 1e-4, new)
    assert old < 1e-4 and new > 10


def test_mutant_scale_softmax_rounds_after_the_subtraction(fake):
    d = R.sm_inputs(R.SmCase(5, 1003, 1008, 0, R.SQ96, 1, "n01"))
    fwd, _ = R.sm_reference(d)
    good = R.run_sm_fwd(fake, d)
    z = R._sm_view(d["sbuf"], d)[:, :1003].float() / d["denom"]
    m = z.max(-1, keepdim=True).values
    ex = torch.exp((z - m).to(BF).float())
    bad = torch.zeros(5, 1008, dtype=BF)
    bad[:, :1003] = (ex / ex.sum(-1, keepdim=True)).to(BF)
    old, new = rel_err(bad, good["p"]), R.worst_of({"p": bad}, R.Ref({"p": fwd.tol["p"]}, {}))
    _report("scale_softmax rounds after the max subtraction", old, 1e-2, new)
    assert old < 1e-2 and new > R.LIMIT


def _psd_one_pass(x, rescale):
    """the per-thread running (max, sum) of psd_logit_stats_kernel on fp32 rows [n, V], V % 8 == 0 or with a scalar tail folded
    into 8-wide steps of -inf padding; `rescale` False: the mutant that keeps the old sum when the max moves.  Returns 1 / sum."""
    n, V = x.shape
    steps = R.cdiv(V, 2048)
    xp = torch.full((n, steps * 2048), -float("inf"))
    xp[:, :V] = x
    xp = xp.view(n, steps, 256, 8)
    best, s = torch.full((n, 256), -float("inf")), torch.zeros(n, 256)
    for k in range(steps):
        f = xp[:, k]
        cm = f.amax(-1)
        up = cm > best
        if rescale:
            s = torch.where(up & torch.isfinite(best), s * torch.exp(best - cm), s)
        best = torch.where(up, cm, best)
        s = s + torch.where(torch.isfinite(f), torch.exp(f - best[..., None]), torch.zeros_like(f)).sum(-1)
    m = best.amax(-1, keepdim=True)
    return 1 / torch.where(torch.isfinite(best), s * torch.exp(best - m), torch.zeros_like(s)).sum(-1)


def test_mutant_psd_rescale_forgotten():
    for profile in ("late", "n01"):
        d = R.psd_inputs(R.PsdCase(25055, profile))
        stats, _ = R.psd_reference(d)
        live = d["live"].reshape(-1)
        x = d["logits"].view(R.PSD_B, R.PSD_BSTRIDE, -1)[:, :R.PSD_T, :25055].reshape(-1, 25055)[live].float()
        want, E = stats.tol["fstat"][0][live, 1], stats.tol["fstat"][1][live, 1]
        good, bad = _psd_one_pass(x, True), _psd_one_pass(x, False)
        assert float(((good.to(F64) - want).abs() / E).max()) <= R.LIMIT            # the restated one-pass form is inside the bound
        old, new = rel_err(bad, want), float(((bad.to(F64) - want).abs() / E).max())
        _report(f"PSD rescale forgotten, {profile} rows", old, 1e-4, new)
        assert new > 100 and old > 1e-2                                          # caught by both: recorded, not a blind spot
