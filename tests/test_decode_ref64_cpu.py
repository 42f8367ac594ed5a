"""CPU checks of the float64 decode-step references and their bounds (tests/decode_ref64.py), which
tests/test_gpu_decode_f64.py holds the HIP kernels to:

* the attention reference is right: it agrees with an explicit per-head torch.softmax in float64 to 1e-13;
* the bounds are honest: the torch double (tests/fake_ops.py restates the kernels' rounding points in fp32) stays within
  1.0 x E on every case of the GPU lists, and gives the exact profile's bits where float64 names them.  Largest |err| / E of the
  double: attention 0.67 (on the older test's inputs; 0.62 on the case list), SwiGLU 0.92, RMSNorm 0.99, bias + RoPE 0.996 (one
  bf16 rounding alone reaches 1.0 x u |y| just above a power of two);
* the checks have teeth.  Mutants through the double, each with its score under the tensor-wide metric of tests/test_gpu_ops.py
  (max|a-b| / max|b|, limits 1e-2 to 2e-2) and its worst |err| / E -- or its count of wrong bits -- under the new one, on the
  inputs of test_attn_decode_long_ragged_contexts, (H, G, ctx) = (12, 2, 1100) / (28, 4, 530):

      newest key dropped on rows with more than 384 visible keys        old 0.0034 / 0.0057 (passes 2e-2)   new 3.2 / 6.3 x E
      newest key through the neighbouring beam's index entry, same rows old 0.0064 / 0.0087 (passes)        new 6.0 / 8.3 x E
      the whole-context row's output zeroed                             old 0.044 / 0.061                   new 36 / 49 x E
      kstart ignored                                                    old 0.25 / 0.95                     new 265 / 37000 x E
      a pack that truncates to bf16 (256 x 384 x 128, 512 x 256 x 8960) old 0.0065 / 0.0068 (passes 1e-2)   new: wrong bits on
                                                                        the exact profile, rms 2.0 x the double's on N(0, 1)
      bias added after the bf16 rounding                                old 0.004-0.005 (passes)            new: wrong bits
      newest k / v appended at pos + 1                                  the k != 0 masks of a patterned cache agree
                                                                                                            new: named slots"""
import pytest
import torch

import decode_ref64 as D
import fake_ops
from fake_ops import FakeOps

HD = D.HD
F64, BF = torch.float64, torch.bfloat16


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


# ------------------------------------------------------------------------------------------------ cache attention
def test_attention_reference_is_softmax_attention():
    c = D.AttnCase(9, 28, 4, 530, True, "peaked")
    inp = D.attn_inputs(c)
    ref, E = D.attn_reference_of(inp)
    M, H, G, ctx = c.M, c.H, c.G, c.ctx
    k3, v3 = inp["kc"].view(-1, ctx, G, HD), inp["vc"].view(-1, ctx, G, HD)
    for r in range(M):
        a, b = int(inp["kstart"][r]), int(inp["lens"][r])
        for h in (0, 6, 7, H - 1):
            rows = inp["index"][r, a:b].long()
            k, v = k3[rows, torch.arange(a, b), h // (H // G)].to(F64), v3[rows, torch.arange(a, b), h // (H // G)].to(F64)
            q = inp["qkv"][r, h * HD:(h + 1) * HD].to(F64)
            want = torch.softmax(k @ q * inp["scale"], 0) @ v
            assert float((ref[0, r, h] - want).abs().max()) < 1e-13
    assert bool((E > 0).all()) and bool(torch.isfinite(ref).all())           # no poisoned cell was read


def test_attention_cases_sit_on_the_kernels_switches():
    """the case list reaches every switch length, group size and the LDS limit the GPU file names"""
    seen, reps = set(), set()
    for c in D.ATTN_CASES:
        inp = D.attn_inputs(c)
        n = (inp["lens"] - inp["kstart"]).tolist()
        seen.update(n)
        reps.add(c.H // c.G)
        assert min(n) >= 1 and int(inp["lens"].max()) <= c.ctx and int(inp["kstart"].min()) >= 0
        assert c.M == 1 or int(inp["kstart"].max()) > 0
        if c.indexed:                                            # every index entry stays inside the allocation
            assert int(inp["index"].min()) >= 0 and int(inp["index"].max()) <= c.M
    assert set(D.SWITCH_LENGTHS) <= seen and 2048 in seen
    assert reps == {1, 2, 4, 6, 7, 8}
    assert D.attn_first_refused_ctx(8) == 1889 and all(D.attn_first_refused_ctx(r) > D.MAX_CTX for r in (1, 2, 4, 6, 7))


@pytest.mark.parametrize("case", D.ATTN_CASES, ids=D.attn_case_id)
def test_attention_double_stays_inside_the_bound(fake, case):
    inp = D.attn_inputs(case)
    ref, E = D.attn_reference_of(inp)
    c = D.check_within(D.attn_double(fake, inp), ref, E, 1.0, "attn_decode double")
    print(f"DOUBLE attn {D.attn_case_id(case)} worst {c.worst:.3f} rms {c.rms:.4f}")
    assert c.ok, c.message


@pytest.mark.parametrize("H,G,ctx,old", [(12, 2, 1100, (0.0034, 0.0064, 0.044)), (28, 4, 530, (0.0057, 0.0087, 0.061))])
def test_attention_mutants_pass_the_old_metric_and_fail_the_new(fake, H, G, ctx, old):
    inp = D.attn_legacy_inputs(H, G, ctx)
    ref, E = D.attn_reference_of(inp)
    good = D.attn_double(fake, inp)
    assert D.check_within(good, ref, E, 1.0).ok
    lens, ks, M = inp["lens"], inp["kstart"], inp["M"]
    long_rows = [r for r in range(M) if int(lens[r] - ks[r]) > 384]
    assert len(long_rows) >= 3
    index = inp["index"].clone()
    for r in long_rows:
        index[r, int(lens[r]) - 1] = inp["index"][(r + 1) % M, int(lens[r]) - 1]
    zeroed = good.clone()
    zeroed[0, 3] = 0                                             # row 3 sees the whole context
    mutants = [("newest key dropped", D.attn_double(fake, inp, lens=torch.where(lens - ks > 384, lens - 1, lens)), old[0], True),
               ("newest key through the neighbour's index entry", D.attn_double(fake, inp, index=index), old[1], True),
               ("whole-context row zeroed", zeroed, old[2], False),
               ("kstart ignored", D.attn_double(fake, inp, kstart=torch.zeros_like(ks)), None, False)]
    for name, out, want_old, passes_old in mutants:
        c = D.check_within(out, ref, E, D.ATTN_LIMIT, name)
        score = rel_err(out, good)
        print(f"MUTANT attn ({H}, {G}, {ctx}) {name}: old metric {score:.4f}, worst |err| / E {c.worst:.1f}")
        assert not c.ok and c.worst > 3.0, c.message
        assert (score < 2e-2) == passes_old, (name, score)
        if want_old is not None:
            assert abs(score - want_old) < 0.06 * want_old, (name, score, want_old)
        if name != "kstart ignored":
            assert any(f"s={r}, " in c.message for r in long_rows), c.message      # names a row that lost its key


# ------------------------------------------------------------------------------------------------ decode GEMMs
check_case = D.check_gemm_case


@pytest.mark.parametrize("case", D.GEMM_CASES, ids=D.gemm_case_id)
def test_gemm_double_gives_the_exact_bits_and_stays_inside_the_bounds(fake, case):
    d = D.gemm_inputs(case, "exact")
    ref = D.gemm_reference(case, d)
    worst = check_case(case, d, ref, D.gemm_double(fake, case, d), 1.0, "double")
    print(f"DOUBLE gemm {D.gemm_case_id(case)} worst {worst:.3f} rounded {ref.frac_rounded:.3f}")
    if case.K >= 1024:
        assert ref.frac_rounded > 0.1                            # the rounding mode is exercised


def test_exact_profile_at_the_longest_k():
    """K = 18944, s = 6 by hand: fp32 matmul == float64 matmul on every element, and most outputs need a bf16 rounding"""
    case = D.GemmCase("plain", 64, 256, 18944, 0, False, 0, 0, 0)
    d = D.gemm_inputs(case, "exact")
    a, w = d["a"], d["w"]
    assert torch.equal((a.float() @ w.float().t()).double(), a.double() @ w.double().t())
    assert D.gemm_reference(case, d).frac_rounded > 0.5


@pytest.mark.parametrize("M,N,K,old", [(256, 384, 128, 0.0065), (512, 256, 8960, 0.0068)])
def test_a_truncating_pack_passes_the_old_metric(fake, monkeypatch, M, N, K, old):
    """the old metric's blind spot, at the shapes it was measured at (the double's gemm takes any M)"""
    g = torch.Generator().manual_seed(1)
    a = torch.randn(M, K, generator=g).to(BF)
    b = (torch.randn(N, K, generator=torch.Generator().manual_seed(2)) * K ** -0.5).to(BF)
    good, bad = torch.zeros(M, N, dtype=BF), torch.zeros(M, N, dtype=BF)
    fake.gemm(a, b, good, M, N, K)
    monkeypatch.setattr(fake_ops, "_bf", _truncate)
    fake.gemm(a, b, bad, M, N, K)
    score = rel_err(bad, good)
    ref = a.double() @ b.double().t()
    r_good, r_bad = D.rms_ulp(good, ref), D.rms_ulp(bad, ref)
    print(f"MUTANT gemm truncating pack {M}x{N}x{K}: old metric {score:.4f}, rms {r_bad:.3f} = {r_bad / r_good:.2f} x the double's {r_good:.3f}")
    assert score < 1e-2 and abs(score - old) < 0.15 * old
    assert r_bad > D.RMS_RATIO * r_good and 0.29 < r_good < 0.58          # 0.29 ulp, an ulp being 1 to 2 x u |c|


MUTANT_CASES = [c for c in D.GEMM_CASES if (c.M, c.N, c.K) in ((17, 64, 1024), (64, 256, 18944), (64, 256, 3584), (64, 64, 8960),
                                                               (64, 1536, 8960), (17, 2048, 1536)) and c.mode != 1]


@pytest.mark.parametrize("case", MUTANT_CASES, ids=D.gemm_case_id)
def test_a_truncating_double_is_rejected_on_both_profiles(fake, monkeypatch, case):
    d, dn = D.gemm_inputs(case, "exact"), D.gemm_inputs(case, "n01")
    ref, refn = D.gemm_reference(case, d), D.gemm_reference(case, dn)
    good_n = D.gemm_double(fake, case, dn)
    monkeypatch.setattr(fake_ops, "_bf", _truncate)
    out, out_n = D.gemm_double(fake, case, d), D.gemm_double(fake, case, dn)
    with pytest.raises(AssertionError, match="16-column tile"):
        check_case(case, d, ref, out, D.GEMM_LIMIT, "truncating double")
    for (name, g0, want, mag), (_, g1, _, _) in zip(D.rms_pairs(case, dn, refn, good_n), D.rms_pairs(case, dn, refn, out_n)):
        r0, r1 = D.rms_ulp(g0, want, mag), D.rms_ulp(g1, want, mag)
        print(f"MUTANT gemm truncating {D.gemm_case_id(case)} {name}: rms {r1:.3f} = {r1 / r0:.2f} x the double's {r0:.3f}")
        assert r1 > D.RMS_RATIO * r0, (name, r0, r1)


@pytest.mark.parametrize("case", [c for c in D.PLAIN_CASES if c.bias and c.mode == 0][:3], ids=D.gemm_case_id)
def test_bias_added_after_the_rounding_is_rejected(fake, case):
    d = D.gemm_inputs(case, "exact")
    ref = D.gemm_reference(case, d)
    good = D.gemm_double(fake, case, d)["c"]
    nob = D.gemm_double(fake, case, d, bias=None)["c"]
    bad = (nob.float() + d["bias"].float()).to(BF)               # bf16(bf16(sum) + bias)
    score = rel_err(bad, good)
    print(f"MUTANT gemm bias after the rounding {D.gemm_case_id(case)}: old metric {score:.4f}, "
          f"{int((bad.view(torch.int16) != ref.exact['c'].view(torch.int16)).sum())} of {bad.numel()} wrong bits")
    assert score < 1e-2
    with pytest.raises(AssertionError, match="differ from the exact result"):
        D.assert_bits(bad, ref.exact["c"], "bias late", case.K)


@pytest.mark.parametrize("case", D.QKV_CASES[:2], ids=D.gemm_case_id)
def test_an_append_at_the_next_slot_is_rejected(fake, case):
    """the old check compares k != 0 masks of zero-filled caches: on a cache that already holds non-zeros it sees nothing"""
    d = D.gemm_inputs(case, "exact")
    good = D.gemm_double(fake, case, d)
    moved = D.gemm_double(fake, case, d, pos=(d["pos"] + 1) % case.ctx)
    assert torch.equal(moved["kc"] != 0, good["kc"] != 0)       # the old mask check passes
    moved["qk"], moved["v"] = good["qk"], good["v"]
    with pytest.raises(AssertionError, match="cache differs"):
        D.check_appended(moved, case, d, "append at pos + 1")
    D.check_appended(good, case, d, "append at pos")


@pytest.mark.parametrize("case", [c for c in D.GEMM_CASES if c.M * c.N >= 4096 and not (c.op == "plain" and c.mode == 1)], ids=D.gemm_case_id)
def test_double_rounds_to_nearest_on_the_n01_profile(fake, case):
    """the yardstick of the GPU file's second check: where ONE rounding separates the result from float64 (the linear epilogues),
    the double's rms(err / (u |c|)) is that of round-to-nearest: 0.29 ulp, an ulp being 1 to 2 x u |c|.  The stacked roundings of
    SwiGLU, RoPE and the norm are recorded only."""
    d = D.gemm_inputs(case, "n01")
    ref = D.gemm_reference(case, d)
    out = D.gemm_double(fake, case, d)
    for name, got, want, mag in D.rms_pairs(case, d, ref, out):
        r = D.rms_ulp(got, want, mag)
        print(f"DOUBLE gemm n01 {D.gemm_case_id(case)} {name} rms {r:.3f}")
        if case.op == "plain" or name in ("c", "v"):
            assert 0.29 < r < 0.58, (name, r)
