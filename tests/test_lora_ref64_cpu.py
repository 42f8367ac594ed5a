"""CPU checks of the float64 references of the LoRA kernels and the AdamW update and of their bounds (tests/lora_ref64.py), which
tests/test_gpu_lora_f64.py holds the HIP kernels to:

* the bounds are honest: the torch double (tests/fake_ops.py, fp32 torch on the CPU) gives the bits of every exact profile, stays
  within 1.0 x E and inside every interval on every case of the shared lists (the F64WORST lines this file prints), and the caps
  on the share of interval elements hold on the reference alone;
* the references are the operations: the GEMM references equal an explicit sum of products, the AdamW reference (with the
  constants left in float64) equals torch.optim.AdamW in float64 fed the same constants, at 1e-12 relative; the one-rounding bf16
  conversion is checked against torch on fp32 values and on a value that `double -> float -> bf16` rounds wrongly;
* the case lists reach what they claim: 0, 1 and 2 chunks per wave, one to four 16-column groups, a last tile of 1 and 15 rows;
* the checks have teeth: mutants through the double, each with its verdict under the older test's own check and under the new
  one (the MUTANT lines of this file; `inf`: wrong bits, an element outside its interval or another mask):

      rank GEMM without wave 7's partial, K = 8960             0.32 of max|ref| (FAILS 2e-3)                       new 53 x E
      rank GEMM without the ninth chunk, K = 576               0.35 (FAILS 2e-3)                                   new 2890 x E
      truncating bf16 store                                    FAILS torch.equal with the rounded fp32 output      new 1.82 x E, rms 1.99 x
      lora_apply without the intermediate bf16(s v)            equal bits at s = 1, 0.25, 2 (passes)               new: wrong bits at s = 0.3
      lora_apply, last row of a tile from row M - 2, M = 4096  2.4e-4 of the elements (passes 2e-3), by 0.59 max|y|
                                                               (FAILS 2^-6)                                        new: outside the interval
      the mask indexed with ldy in place of N                  37 % of the elements differ (FAILS 2e-3)            new: not lora_dropout's mask
      AdamW without decay                                      p 4.8e-7 (passes 1e-5)                              new 4.5 x E
      AdamW with eps inside the root                           p 3.4e-8 (passes 1e-5)                              new 1.37 x E
      AdamW with 1 - beta from the double (0.1, 0.001)         m 8.2e-8, v 7.4e-8 (passes 1e-5)                    new 41 x E

Largest |err| / E of the double: gemm_rank NT 0.978, group 0.982, TN 0.016, AdamW m 0.963, v 0.995, p 0.959."""
import math

import numpy as np
import pytest
import torch

import lora_ref64 as L
from fake_ops import FakeOps, _bf
from oracle.lora_oracle import lora_keep_scale

F64, F32, BF, I32, I64 = torch.float64, torch.float32, torch.bfloat16, torch.int32, torch.int64
e, U = L.e, L.U


@pytest.fixture(scope="module")
def fake():
    return FakeOps()


def rel_err(a, b):
    """the tensor-wide metric of tests/test_gpu_ops.py"""
    a, b = a.float(), b.float()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def close(a, b, what):
    err = float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
    assert err < 1e-12, (what, err)


def _truncate(x):
    """fp32 -> bf16 by dropping the low 16 bits (round toward zero)"""
    return (x.float().contiguous().view(torch.int32) & -65536).view(F32).to(BF)


# ------------------------------------------------------------------------------------------------ the roundings
def test_bf16r_rounds_once_to_nearest_even():
    x = torch.randn(100000, generator=L.gen(1)) * torch.exp2(torch.randint(-20, 20, (100000,), generator=L.gen(2)).float())
    assert torch.equal(L.to_bf(L.bf16r(x.to(F64))), x.to(BF))                       # on fp32 values: torch's single rounding
    ties = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 0.0, 2.0 ** -100], dtype=F64)
    assert L.bf16r(ties).tolist() == [1.0, 1 + 2.0 ** -6, -1.0, 0.0, 2.0 ** -100]   # ties go to the even neighbour
    twice = torch.tensor([1 + 2.0 ** -8 + 2.0 ** -40], dtype=F64)                   # fl32 drops 2^-40, then the tie goes DOWN to 1
    assert float(L.bf16r(twice)) == 1 + 2.0 ** -7 and float(twice.to(F32).to(BF)) == 1.0
    assert float(L.fl32(torch.tensor([1 + 2.0 ** -24 + 2.0 ** -50], dtype=F64))) == 1 + 2.0 ** -23


# ------------------------------------------------------------------------------------------------ the lists reach their branches
def test_case_lists_reach_every_branch():
    per_wave = {n for c in L.NT_CASES for n in L.nt_chunks_per_wave(c.K)}
    assert {0, 1, 2} <= per_wave
    assert L.nt_chunks_per_wave(64) == [1, 0, 0, 0, 0, 0, 0, 0] and L.nt_chunks_per_wave(448)[6:] == [1, 0]
    assert L.nt_chunks_per_wave(512) == [1] * 8 and L.nt_chunks_per_wave(576) == [2] + [1] * 7
    assert {(c.N + 15) // 16 for c in L.NT_CASES} == {1, 2, 3, 4} == {(c.N + 15) // 16 for c in L.TN_CASES}
    last = {c.M - (c.M - 1) // 16 * 16 for c in L.NT_CASES}
    assert {1, 15, 16} <= last                                   # M = 1 / 17: one row; M = 15: fifteen; M = 16: a full tile
    assert {c.M for c in L.NT_CASES} == {1, 15, 16, 17, 141, 333} and {c.N for c in L.NT_CASES} == {8, 16, 24, 40, 48, 64}
    assert {c.K for c in L.NT_CASES} == {64, 448, 512, 576, 1536, 8960} and any(c.lead for c in L.NT_CASES)
    assert {c.M for c in L.TN_CASES} == {64, 192, 1536} and {c.N for c in L.TN_CASES} == {8, 16, 24, 40, 64}
    assert {c.K for c in L.TN_CASES} == {64, 448, 512, 576, 4096}
    assert {c.members for c in L.GROUP_CASES} == {1, 2, 3, 4} and {c.M for c in L.GROUP_CASES} == {100, 333}
    assert {c.M for c in L.APPLY_CASES} >= {1, 63, 64, 65, 141, 333} and {c.N for c in L.APPLY_CASES} >= {8, 248, 256, 264, 520, 1536}
    assert {c.members for c in L.APPLY_CASES} == {0, 1, 2, 3, 4} and {c.R for c in L.APPLY_CASES} == {64, 128}
    assert L.ELEM_CASES[-1].M * L.ELEM_CASES[-1].D // 4 > 4096 * 256 and L.ELEM_CASES[-1].M * L.ELEM_CASES[-1].D > 2 ** 22
    assert L.ELEM_BIG8.M * L.ELEM_BIG8.D // 8 > 4096 * 256
    assert L.ADAM_BIG // 4 == 4096 * 256 + 1                     # the second pass of the grid-stride loop is its last vector
    assert {c.step for c in L.ADAM_CASES} == {1, 3, 100000} and {c.wd for c in L.ADAM_CASES} == {0.0, 0.01, 0.1}
    assert {c.n for c in L.ADAM_CASES} == {4, 4160, L.ADAM_BIG} and {c.pb for c in L.ADAM_CASES} == {0, 1}


# ------------------------------------------------------------------------------------------------ rank GEMMs
def hold_gemm(got, ref, what, transposed=("c_t", "cb_t")):
    w = L.check(got, L.Ref({k: v for k, v in ref.tol.items() if k in got}, {k: v for k, v in ref.exact.items() if k in got}), what)
    for k in transposed:
        if k in got:
            L.same_bits(got[k], got[k[:-2]], f"{what}: the transposed store against the plain one, {k}")
    return w


@pytest.mark.parametrize("family", ["nt", "tn", "group"])
def test_double_gemms_inside_the_bound_on_every_case(fake, family):
    worst = 0.0
    if family == "group":
        for c in L.GROUP_CASES:
            d = L.group_inputs(c)
            got = L.run_group(fake, d)
            for t, m in enumerate(d["members"]):
                worst = max(worst, hold_gemm({"cb": got[f"cb{t}"]}, L.gemm_reference(m), f"group {L.case_id(c)} member {t}"))
    else:
        cases, inputs, run = (L.NT_CASES, L.nt_inputs, L.run_nt) if family == "nt" else (L.TN_CASES, L.tn_inputs, L.run_tn)
        for c in cases:
            d = inputs(c)
            worst = max(worst, hold_gemm(run(fake, d), L.gemm_reference(d), f"{family} {L.case_id(c)}"))
    print(f"F64WORST double gemm_rank {family} |err| / E {worst:.3f}")
    assert worst <= 1.0


def test_gemm_reference_is_the_sum_of_products():
    for c in (L.NtCase(17, 40, 576, "n01", 0), L.NtCase(15, 16, 448, "exact", 0)):
        d = L.nt_inputs(c)
        ref = L.gemm_reference(d)
        plain = (d["a"].to(F64)[:, None, :] * d["b"].to(F64)[None]).sum(-1)
        close(ref.tol["c"][0] if c.profile == "n01" else ref.exact["c"].to(F64), plain, c)
    d = L.tn_inputs(L.TnCase(64, 16, 448, "n01"))
    at = d["At"].view(d["At"].buf).to(F64)                         # [K, M] as the kernel reads it
    close(L.gemm_reference(d).tol["c"][0], torch.einsum("km,nk->mn", at, d["b"].to(F64)), "tn")


# ------------------------------------------------------------------------------------------------ lora_apply
def apply_worst(fake, cases, profile):
    shares = {}
    for c in cases:
        if profile == "exact":
            d = L.apply_inputs(c, "exact")
            for s, p, resid in L.EXACT_SETTINGS:
                if c.members and resid:
                    continue
                lo, hi = L.apply_reference(d, s, p, True)
                y, x = L.run_apply(fake, d, s, p, resid)
                L.same_bits(y, L.to_bf(lo), f"apply exact {L.case_id(c)} s={s} p={p} y")
                L.check_apply(y, x, d, (lo, hi), resid, f"apply exact {L.case_id(c)} s={s} p={p}")
        else:
            for y_zero in (True, False):
                d = L.apply_inputs(c, "n01", y_zero)
                for s, p, resid in L.N01_SETTINGS:
                    resid = resid and not c.members
                    lo, hi = L.apply_reference(d, s, p, False)
                    y, x = L.run_apply(fake, d, s, p, resid)
                    L.check_apply(y, x, d, (lo, hi), resid, f"apply n01 {L.case_id(c)} y_zero={y_zero} s={s} p={p}")
                    n_open, n = int((lo != hi).sum()), lo.numel()
                    cap = L.share_cap(c.R, y_zero)
                    if n >= L.CAP_MIN:
                        assert n_open <= cap * n, (c, y_zero, s, p, n_open / n, cap)
                    k = (c.R, y_zero, max(c.members, 1))
                    a, b, m = shares.get(k, (0, 0, 0.0))
                    shares[k] = (a + n_open, b + n, max(m, n_open / n if n >= L.CAP_MIN else 0.0))
    return shares


def test_double_apply_has_the_bits_of_the_exact_profile(fake):
    apply_worst(fake, L.APPLY_CASES, "exact")


def test_double_apply_inside_every_interval_and_the_caps_hold(fake):
    shares = apply_worst(fake, L.APPLY_CASES, "n01")
    for (R, y_zero, members), (n_open, n, largest) in sorted(shares.items()):
        print(f"F64SHARE lora_apply R {R} y {'0' if y_zero else 'n01'} members {members}: ends differ on {n_open / n:.4f} of {n} elements "
              f"(largest case {largest:.4f}, cap {L.share_cap(R, y_zero):.2f})")
        assert n_open <= L.share_cap(R, y_zero) * n


def mask_check(ops, c, s, p, to=None):
    """v = 1 everywhere: lora_apply's result against lora_dropout of a bf16(s)-filled matrix and against lora_keep_scale; returns the
    members' results"""
    d = L.apply_inputs(c, "mask")
    out = []
    for t in range(max(c.members, 1)):                          # member t alone (the group's earlier members would add to y)
        one = dict(d, members=0, sids=[d["sids"][t]], us=[d["us"][t]], ws=[d["ws"][t]], U=[d["U"][t]], W=[d["W"][t]])
        y, _ = L.run_apply(ops, one, s, p, False, to)
        filled = dict(M=c.M, D=c.N, xb=torch.full((c.M, c.N), s).to(BF), rng=d["rng"])
        L.same_bits(y, L.run_dropout(ops, filled, p, d["sids"][t], to), f"mask {L.case_id(c)} member {t}: lora_apply against lora_dropout")
        L.same_bits(y, L.dropout_reference(filled, p, d["sids"][t]), f"mask {L.case_id(c)} member {t}: against lora_keep_scale")
        out.append(y)
    if c.members > 1:                                           # the group launch: the members' masks add up, and differ
        lo, hi = L.apply_reference(d, s, p, True)
        y, _ = L.run_apply(ops, d, s, p, False, to)
        L.same_bits(y, L.to_bf(lo), f"mask {L.case_id(c)}: the group launch")
        assert all(not torch.equal(out[0], o) for o in out[1:]), "two members of a group drew the same mask"
    return out


MASK_CASES = [c for c in L.APPLY_CASES if (c.M, c.N) in ((65, 264), (333, 1536), (141, 520), (333, 248), (64, 1536))]


def test_double_mask_is_the_dropout_kernels_mask(fake):
    for c in MASK_CASES:
        for s, p in ((1.0, 0.25), (0.3, 0.05)):
            mask_check(fake, c, s, p)


# ------------------------------------------------------------------------------------------------ elementwise, refresh, transpose
def elementwise_check(ops, c, to=None, big8=False):
    d = L.elem_inputs(c)
    what = f"elementwise {L.case_id(c)}"
    if c.D % 8 == 0:
        for s in ((0.3,) if big8 else (0.25, 0.3)):
            L.same_bits(L.run_scale(ops, d, s, to), L.scale_reference(d, s), f"{what} scale_bf16 s={s}")
        for p, sid in (((0.25, 13),) if big8 else ((0.05, 0), (0.25, 13))):
            L.same_bits(L.run_dropout(ops, d, p, sid, to), L.dropout_reference(d, p, sid), f"{what} lora_dropout p={p}")
    if big8:
        return
    for p, sids in ((0.05, [3]), (0.25, [5, 13, 21])):
        refs = [L.dropout_norm_reference(d, p, sid) for sid in sids]
        for group in (False, True):
            got = L.run_dropout_norm(ops, d, p, sids if group else sids[:1], group, to)
            for g, r in zip(got, refs):
                L.same_bits(g, r, f"{what} lora_dropout_norm{'_group' if group else ''} p={p}")


def test_double_elementwise_refresh_transpose_bits(fake):
    for c in L.ELEM_CASES[:-1] + [L.ElemCase(37, 4096)]:
        elementwise_check(fake, c)
    d = L.refresh_inputs()
    for got, want, ent in zip(L.run_refresh(fake, d), L.refresh_reference(d), L.REFRESH_ENTRIES):
        L.same_bits(got, want, f"refresh {ent}")
    for c in L.TR_CASES:
        transpose_check(fake, c)


def transpose_check(ops, c, to=None):
    got, src = L.run_transpose(ops, c, to)
    want = torch.zeros(c.Cpad, c.Rpad, dtype=BF)
    want[:c.C, :c.R] = src.t()
    L.same_bits(got, want, f"transpose {L.case_id(c)}")


# ------------------------------------------------------------------------------------------------ AdamW
def adam_check(ops, c, to=None):
    d = L.adam_inputs(c)
    ref, k = L.adam_reference(d)
    got = L.run_adam(ops, d, to)
    w = L.check(got, ref, f"adamw {L.case_id(c)}")
    if c.profile == "decay":
        L.check_decay(got["p"][0], d, k, f"adamw {L.case_id(c)}")
    per = {n: L.worst_of({n: got[n]}, L.Ref({n: ref.tol[n]}, {})) for n in ref.tol}
    return w, per


def test_adam_constants_the_two_forms_of_the_decay_factor_agree():
    for c in L.ADAM_CASES:
        k = L.adam_constants(c.step, c.wd)
        assert k["k_wd"] == k["k_wd_fused"], (c, k)
        assert k["c1"] == float(np.float32(1) - np.float32(L.BETA1)) and k["c2"] == float(np.float32(1) - np.float32(L.BETA2))


def test_double_adamw_inside_the_bound_on_every_case(fake):
    worst = {}
    for c in L.ADAM_CASES:
        _, per = adam_check(fake, c)
        for n, w in per.items():
            worst[n] = max(worst.get(n, 0.0), w)
    print("F64WORST double adamw |err| / E " + " ".join(f"{n} {w:.3f}" for n, w in sorted(worst.items())))
    assert max(worst.values()) <= 1.0


def test_adam_reference_is_torch_adamw_in_float64():
    for c in (L.AdamCase("n01", 4160, 3, 0.01, 0.125, 0), L.AdamCase("first", 4160, 1, 0.1, 1.0, 0), L.AdamCase("n01", 4160, 100000, 0.0, 1.0, 0)):
        d = L.adam_inputs(c)
        ref, k = L.adam_reference(d, kernel=False)
        p = torch.nn.Parameter(d["p"].to(F64))
        opt = torch.optim.AdamW([p], lr=L.f32c(L.LR), betas=(k["b1"], k["b2"]), eps=k["eps"], weight_decay=L.f32c(c.wd))
        opt.state[p] = dict(step=torch.tensor(float(c.step - 1)), exp_avg=d["m"].to(F64), exp_avg_sq=d["v"].to(F64))
        p.grad = d["g"].to(F64) * L.f32c(c.gscale)
        opt.step()
        close(ref.tol["p"][0][0] - d["p"].to(F64), p.data - d["p"].to(F64), ("the update", c))     # the update itself, not p + update
        close(ref.tol["m"][0][0], opt.state[p]["exp_avg"], ("m", c))
        close(ref.tol["v"][0][0], opt.state[p]["exp_avg_sq"], ("v", c))


# ------------------------------------------------------------------------------------------------ mutants through the double
def old_gemm_check(c, a, b):
    """test_gemm_rank_vs_fp32's: max |c - ref| < 2e-3 max |ref| + 1e-6 against an fp32 product"""
    ref = a.float() @ b.float().t()
    return float((c - ref).abs().max()) < 2e-3 * float(ref.abs().max()) + 1e-6, float((c - ref).abs().max() / ref.abs().max())


def chunked(a, b, drop):
    """fp32 A B^T summed chunk by chunk, without the chunks `drop` selects"""
    acc = torch.zeros(a.shape[0], b.shape[0])
    for ch in range(a.shape[1] // 64):
        if not drop(ch):
            acc += a[:, ch * 64:ch * 64 + 64].float() @ b[:, ch * 64:ch * 64 + 64].float().t()
    return acc


def old_apply_check(a, b):
    """test_lora_apply_bit_exact_vs_double's: fewer than 0.2 % of the elements differ, by at most 2^-6 max |y|"""
    diff = (a.float() - b.float()).abs()
    return float((diff > 0).float().mean()) < 2e-3 and float(diff.max()) <= 2.0 ** -6 * float(b.float().abs().max()), \
        (float((diff > 0).float().mean()), float(diff.max() / b.float().abs().max()))


def apply_mutant(d, s, p, kind, ldy=None):
    """FakeOps.lora_apply with one thing wrong"""
    M, N, R = d["M"], d["N"], d["R"]
    u, w = d["us"][0].float(), d["ws"][0].float()
    if kind == "row":                                            # the last row of the last 64-row tile from row M - 2
        u = u.clone()
        u[M - 1] = u[M - 2]
    v = _bf(u @ w.t()).float()
    dlt = v * float(np.float32(s)) if kind == "noround" else _bf(v * float(np.float32(s))).float()
    if p > 0:
        if kind == "ldy":
            keep = lora_keep_scale(L.RNG, d["sids"][0], (M, ldy), p)[:, :N]
        else:
            keep = lora_keep_scale(L.RNG, d["sids"][0], (M, N), p)
        dlt = _bf(dlt * keep).float()
    return _bf(d["y"].float() + dlt)


def adam_mutant(d, kind):
    """FakeOps.adamw (the corrected one) with one thing wrong; returns {p, m, v} [1, n]"""
    b1, b2 = float(np.float32(L.BETA1)), float(np.float32(L.BETA2))
    c1, c2 = (1 - L.BETA1, 1 - L.BETA2) if kind == "double_c" else (1 - b1, 1 - b2)      # double_c: 0.1 and 0.001, from Python's double betas
    lr = float(np.float32(L.LR))
    p, m, v = d["p"].clone(), d["m"].clone(), d["v"].clone()
    gr = d["g"] * d["gscale"]
    m.mul_(L.BETA1).add_(gr, alpha=c1)
    v.mul_(L.BETA2).addcmul_(gr, gr, value=c2)
    bc1, bc2 = 1 - b1 ** d["step"], 1 - b2 ** d["step"]
    den = (v / bc2 + L.EPS).sqrt() if kind == "eps_in_root" else v.sqrt() / math.sqrt(bc2) + L.EPS
    if kind != "no_decay":
        p.mul_(1 - lr * d["wd"])
    p.addcdiv_(m, den, value=-lr / bc1)
    return {"p": p[None], "m": m[None], "v": v[None]}


def test_mutants_the_old_checks_and_the_new(fake):
    """every mutant fails the new check; `old` records what the older test's own check says of it (True: it passes that check)"""
    rec = {}
    # --- rank GEMMs, K = 8960 without wave 7's partial / K = 576 without the ninth chunk, fp32 out
    for name, K, drop in (("gemm: wave 7's partial lost, K = 8960", 8960, lambda ch: ch % 8 == 7), ("gemm: ninth chunk lost, K = 576", 576, lambda ch: ch == 8)):
        d = L.nt_inputs(L.NtCase(333, 64, K, "n01", 0))
        ref = L.gemm_reference(d)
        got = chunked(d["a"], d["b"], drop)
        ok_old, score = old_gemm_check(got, d["a"], d["b"])
        rec[name] = (ok_old, f"{score:.2e} of max|ref| (limit 2e-3)", L.worst_of({"c": got}, L.Ref({"c": ref.tol["c"]}, {})))
    # --- a truncating bf16 store: the old test compares the bf16 output with the rounded fp32 output, bit for bit
    d = L.nt_inputs(L.NtCase(333, 64, 576, "n01", 0))
    ref = L.gemm_reference(d)
    c32 = d["a"].float() @ d["b"].float().t()
    got = _truncate(c32)
    k, n = L.rms_u(got, ref.tol["cb"][0])
    kd, _ = L.rms_u(c32.to(BF), ref.tol["cb"][0])
    assert n >= 4096 and k > L.RMS_RATIO * kd
    rec["gemm: truncating bf16 store"] = (torch.equal(got, c32.to(BF)), f"torch.equal with bf16(fp32 out); rms ratio {k / kd:.2f}",
                                          L.worst_of({"cb": got}, L.Ref({"cb": ref.tol["cb"]}, {})))
    # --- lora_apply without the intermediate bf16(s v): invisible at the dyadic scales the old test uses (1, 0.25, 2)
    c = L.ApplyCase(333, 512, 64, 0)
    d = L.apply_inputs(c, "n01")
    ok_old = all(old_apply_check(apply_mutant(d, s, 0.0, "noround"), apply_mutant(d, s, 0.0, None))[0] for s in (1.0, 0.25, 2.0))
    dx = L.apply_inputs(c, "exact")
    lo, _ = L.apply_reference(dx, 0.3, 0.0, True)
    wrong = int((apply_mutant(dx, 0.3, 0.0, "noround").to(F64) != lo).sum())
    assert torch.equal(apply_mutant(dx, 0.3, 0.0, None), L.to_bf(lo))
    rec["lora_apply: no bf16(s v)"] = (ok_old, "equal bits at s = 1, 0.25, 2", math.inf if wrong else 0.0)
    # --- the last row of a 64-row tile from row M - 2, M = 4096
    c = L.ApplyCase(4096, 512, 64, 0)
    d = L.apply_inputs(c, "n01")
    good, bad = apply_mutant(d, 1.0, 0.0, None), apply_mutant(d, 1.0, 0.0, "row")
    ok_old, score = old_apply_check(bad, good)
    lo, hi = L.apply_reference(d, 1.0, 0.0, False)
    outside = int((~((bad.to(F64) >= lo) & (bad.to(F64) <= hi))).sum())
    assert int((~((good.to(F64) >= lo) & (good.to(F64) <= hi))).sum()) == 0
    rec["lora_apply: last row from row M - 2, M = 4096"] = (ok_old, f"{score[0]:.1e} of the elements differ, by {score[1]:.2f} max|y| (limits 2e-3, 2^-6)",
                                                            math.inf if outside else 0.0)
    # --- the mask indexed with ldy in place of N
    c = L.ApplyCase(141, 520, 64, 0)
    d = L.apply_inputs(c, "mask")
    good, bad = apply_mutant(d, 1.0, 0.25, None), apply_mutant(d, 1.0, 0.25, "ldy", ldy=c.N + 16)
    dn = L.apply_inputs(c, "n01")
    ok_old, score = old_apply_check(apply_mutant(dn, 1.0, 0.25, "ldy", ldy=c.N + 16), apply_mutant(dn, 1.0, 0.25, None))
    filled = dict(M=c.M, D=c.N, xb=torch.ones(c.M, c.N, dtype=BF))
    assert torch.equal(good, L.dropout_reference(filled, 0.25, d["sids"][0]))
    rec["lora_apply: mask indexed with ldy"] = (ok_old, f"{score[0]:.2f} of the elements differ (limit 2e-3)",
                                                math.inf if not torch.equal(bad, good) else 0.0)
    # --- AdamW: the old test's case (N(0, 1) state, step 3, wd 0.01, grad_scale 0.125) and rel_err < 1e-5
    c = L.AdamCase("n01", 4160, 3, 0.01, 0.125, 0)
    d = L.adam_inputs(c)
    ref, _ = L.adam_reference(d)
    good = adam_mutant(d, None)
    assert L.worst_of(good, ref) <= 1.0
    for name, kind in (("adamw: no weight decay", "no_decay"), ("adamw: eps inside the root", "eps_in_root"), ("adamw: 1 - beta from the double", "double_c")):
        bad = adam_mutant(d, kind)
        scores = [rel_err(bad[n], good[n]) for n in "pmv"]
        rec[name] = (max(scores) < 1e-5, "rel_err p / m / v " + " / ".join(f"{s:.1e}" for s in scores) + " (limit 1e-5)", L.worst_of(bad, ref))
    for name, (ok_old, how, new) in rec.items():
        print(f"MUTANT {name}: old check {'PASSES' if ok_old else 'fails'} ({how}); new {new:.3g} x E")
        assert new > 1.0, name
    old_blind = {n for n, r in rec.items() if r[0]}
    assert old_blind == {"lora_apply: no bf16(s v)", "adamw: no weight decay", "adamw: eps inside the root", "adamw: 1 - beta from the double"}, old_blind
