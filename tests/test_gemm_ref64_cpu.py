"""CPU checks of the float64 references of the training-step / prefill GEMMs and their bounds (tests/gemm_ref64.py), which
tests/test_gpu_gemm_f64.py holds the HIP kernels to:

* the bounds are honest: the torch double (tests/fake_ops.py) stays within 1.0 x E on every case of the GPU lists and gives the
  exact profile's bits wherever the check is torch.equal.  Neither the double nor a derivation needed a fix.  Largest |err| / E of
  the double: N(0, 1) linear outputs 0.991 (one bf16 rounding alone reaches u |c| just above a power of two), SwiGLU 0.961,
  bias + RoPE 0.996, dswiglu 0.996 on exact accumulations;
* the case lists reach what their comments name: every TASU_GEMM_PLAN_* value through tasu_gemm_plan (host code), every route of
  the gate|up policy through tasu_gemm_gate_up_plan (the planner the entry point launches from; gemm_ref64.gu_route, a hand
  restatement of the policy, is held to it over a grid of 1008 shapes, so an edit of the policy that moves a route IS caught
  here), and the stream-K conditions through tasu_streamk_schedule -- a later edit of the dispatcher's policy or of the
  schedule cannot quietly empty a path of its cases;
* the checks have teeth.  These are mutants of the RESTATED pipeline (fp32 torch, below), each with its score under the
  tensor-wide metric of tests/test_gpu_ops.py (max|a-b| / max|b| < 1e-2, 2e-2 for the fused epilogues, 2e-5 sqrt(K) in fp32 mode)
  and under the new check; scratch mutants of the kernels themselves were not run:

      a truncating pack (300 x 520 x 256)                        old 0.0038 (passes)   new 1.95 x E, rms over 1.5 x the double's on N(0, 1);
                                                                                       593 of 156,000 wrong bits on the exact profile
      bias added after the rounding                              old 0.0075 (passes)   new 26 x E on N(0, 1), 586 wrong bits
      bf16(R + sum) for R + bf16(sum)                            old 0.0037 (passes)   new 59 x E on N(0, 1), 2,369 wrong bits
      fp32 mode, one of two K-range partials through bf16        old 0.0015 at K = 8960 (limit 0.0019: passes)
                                                                                       new: 35 % of the bits wrong
      silu rounded once in act                                   old 0.0053 (passes)   new 0.50 x E: NOT rejected -- the mutant is the more
                                                                                       accurate form and sits inside any honest bound; only
                                                                                       bit identity with the unfused kernels (test_gpu_ops.py) sees it
      rotated v heads at 2^-7 of the q / k magnitude             old 0.012 (passes)    new: wrong bits in v
      a store of 8 columns where 3 remain, last row              old: C has no guard rows   new: named guard element
      a row beyond M written                                     old: not looked at    new: named guard element
      slab 0 summed twice, slab 1 omitted (16 slabs)             old 0.43: the old metric REJECTS it too -- not a mutant, dropped"""
import math

import pytest
import torch

import gemm_ref64 as G
from fake_ops import FakeOps

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
HD = G.HD


@pytest.fixture(scope="module")
def fake():
    return FakeOps()


@pytest.fixture(scope="module")
def lib():
    from ps_slm_amd import _lib
    return _lib.load()


def rel_err(a, b):
    """the tensor-wide metric of tests/test_gpu_ops.py"""
    a, b = a.float(), b.float()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _truncate(x):
    """fp32 -> bf16 by dropping the low 16 bits (round toward zero)"""
    return (x.float().contiguous().view(torch.int32) & -65536).view(F32).to(BF)


def case_named(op, via, M, N, K, mode=0, **kw):
    hits = [c for c in G.CASES if (c.op, c.via, c.M, c.N, c.K, c.mode) == (op, via, M, N, K, mode) and all(getattr(c, k) == v for k, v in kw.items())]
    assert hits, (op, via, M, N, K, mode, kw)
    return hits[0]


# ------------------------------------------------------------------------------------------------ the double inside the bounds
@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_double_gives_the_exact_bits_and_stays_inside_the_bounds(fake, case):
    for profile in ("exact", "n01") if case.n01 else ("exact",):
        d = G.make_inputs(case, profile)
        ref = G.reference(case, d)
        out = G.run_double(fake, case, d)
        worst = G.check_case(case, d, ref, out, f"double {G.case_id(case)} {profile}")
        print(f"DOUBLE {G.FAMILY[case.op]} {G.case_id(case)} {profile}: worst |err| / E {worst:.3f}, rounded {ref.frac_rounded:.3f}")
        if profile == "exact":
            assert ref.exact, "no exact-bits output"
            if case.K >= 8960:
                assert ref.frac_rounded > 0.4                    # the rounding mode is exercised
        else:
            for name, got, want, mag in G.rms_pairs(case, d, ref, out):
                r = G.rms_ulp(got, want, mag)
                print(f"DOUBLE n01 {G.case_id(case)} {name} rms {r:.3f}")
                if name in ("c", "gu", "dact", "v") and got.numel() >= 4096:
                    assert 0.29 < r < 0.58, (name, r)            # round-to-nearest: 0.29 ulp, an ulp being 1 to 2 x u |c|


def test_case_ids_are_unique_and_operands_stay_small():
    ids = [G.case_id(c) for c in G.CASES]
    assert len(set(ids)) == len(ids)
    for c in G.CASES:
        rows = 2 * c.N if c.op == "swiglu" else c.N
        assert max(c.M, rows) * (c.K + c.ldx) * 2 < 100e6, G.case_id(c)
        assert c.K % 64 == 0
    # an offset C / R is 8- but not 16-byte aligned in ITS element size, and every named kernel meets one in every mode
    for c in G.CASES:
        size = 2 if c.op != "plain" or c.mode == 0 else 4
        assert not c.coff or (c.coff * size) % 16 == 8, G.case_id(c)
        assert not c.roff or (c.roff * 4) % 16 == 8, G.case_id(c)
    for k in ("pp256", "pipe128", "pipe192", "pipe96"):
        assert {c.mode for c in G.KERNEL_CASES if c.via == k and c.coff} == {0, 1, 2}
        assert any(c.roff for c in G.KERNEL_CASES if c.via == k and c.mode == 2)


# ------------------------------------------------------------------------------------------------ the lists reach what they name
def test_case_list_reaches_every_plan(lib):
    seen = set()
    for c in G.CASES:
        if c.plan is None:
            continue
        mode = c.mode if c.op == "plain" else 0                  # (dswiglu and bias + ReLU dispatch their GEMM with bf16 output)
        got = lib.tasu_gemm_plan(c.M, c.N, c.K, mode, 1)
        assert got == c.plan, f"{G.case_id(c)}: the dispatcher plans {G.PLAN_NAMES.get(got, got)}, the list names {G.PLAN_NAMES[c.plan]}"
        seen.add(got)
    assert seen == set(G.PLAN_NAMES), f"no case for {[G.PLAN_NAMES[p] for p in set(G.PLAN_NAMES) - seen]}"
    # both pick_bn outcomes below 65 rows (csrc/gemm_dispatch.h, restated): 96 wide where ceil(N / 96) / 1.08 > ceil(N / 128)
    bn = {96 if -(-c.N // 96) / 1.08 > -(-c.N // 128) else 128 for c in G.PLAN_CASES if c.plan == G.TILES}
    assert bn == {96, 128}
    assert any(c.M == 1 and c.N % 16 for c in G.PLAN_CASES if c.plan == G.TILES)
    # the 256 x 192 split-K needs its four conditions, and the workspace
    for c in G.PLAN_CASES:
        if c.plan == G.SPLITK:
            assert c.M > 128 and -(-c.M // 256) * -(-c.N // 96) < 128 and c.K >= 16384
            assert lib.tasu_gemm_plan(c.M, c.N, c.K, c.mode, 0) != G.SPLITK
    # the column split: at least one whole round of 256 tiles of 256 x 256
    for c in G.PLAN_CASES:
        if c.plan in (G.PP_P128, G.PP_P192):
            assert -(-c.M // 256) * -(-c.N // 256) > 256


def test_gate_up_cases_reach_every_route(lib):
    for c in G.SWIGLU_CASES:
        assert G.gu_route(c.M, c.N, c.K) == c.via, (G.case_id(c), G.gu_route(c.M, c.N, c.K))
        assert lib.tasu_gemm_gate_up_plan(c.M, c.N, c.K, 1) == G.GU_PLAN[c.via], G.case_id(c)
    assert {c.via for c in G.SWIGLU_CASES} == {"pipe", "pp", "pp+pipe", "pp-sk"}
    assert any(c.N % 128 for c in G.SWIGLU_CASES) and any(c.N % 8 == 4 for c in G.SWIGLU_CASES)
    assert any(c.coff for c in G.SWIGLU_CASES) and any(c.pad for c in G.SWIGLU_CASES)
    # the restatement on the shapes tests/test_gpu_ops.py documents: the benchmark's gate|up (1120 tiles: 4 rounds + a column tail)
    # and its stream-K case
    assert G.gu_route(4096, 8960, 1536) == "pp+pipe" and G.gu_route(2048, 1536, 16384) == "pp-sk"
    assert G.gu_route(2048, 1536, 16384, have_ws=False) != "pp-sk"
    # the library's planner against the restatement
    seen = {}
    for M in (1, 64, 65, 256, 300, 512, 2048, 4096, 8192):
        for I in (128, 200, 1024, 1536, 8320, 8960, 18944, 32896):
            for K in (64, 128, 256, 1536, 3584, 16384, 17920):
                for ws in (0, 1):
                    want = G.gu_route(M, I, K, have_ws=bool(ws))
                    assert lib.tasu_gemm_gate_up_plan(M, I, K, ws) == G.GU_PLAN[want], (M, I, K, ws, want)
                    seen[want] = seen.get(want, 0) + 1
    print(f"GU ROUTES over the grid: {seen}")
    assert set(seen) == set(G.GU_PLAN)                           # (pipe 752, pp 118, pp+pipe 120, pp-sk 18 of the 1008)


def test_streamk_cases_meet_the_schedule_conditions(lib):
    facts = {}
    for c in G.STREAMK_CASES + [c for c in G.CASES if c.plan == G.SK or c.via == "pp-sk"]:
        tiles = -(-c.M // 256) * -(-c.N // (128 if c.op == "swiglu" else 256))      # (gate|up: 128 act columns per 256 x 256 tile)
        f = G.streamk_facts(lib, tiles, c.K // 128)
        assert f["cut"] > 0, (G.case_id(c), "no tile is cut")
        facts[(tiles, c.K // 128)] = f
    roles = set().union(*(f["roles"] for f in facts.values()))
    assert roles == {0, 1, 2}, roles                             # whole, producer, owner
    assert max(f["max_ranges"] for f in facts.values()) >= 3
    snapped = [k for k, f in facts.items() if f["snapped"]]
    assert snapped and any((t * p) % G.CUS for t, p in snapped), "no range end was moved to a tile boundary"
    more = [(t, p) for (t, p), f in facts.items() if t > G.CUS]
    assert more and all(p >= 8 and facts[(t, p)]["cut"] == t % G.CUS + G.CUS for t, p in more), "no more-than-one-round case"
    few = [(t, p) for (t, p) in facts if t < G.CUS]
    assert few and all(t * p >= 8 * G.CUS for t, p in few)
    assert facts[(16, 128)]["max_ranges"] == 16 and facts[(288, 8)]["roles"] == {0, 1, 2}
    # ... and one shape whose cut tiles are followed by round-robin whole tiles (the form the benchmark's shapes take)
    assert facts[(528, 8)]["cut"] == 272 < 528 and facts[(528, 8)]["whole_after_cut"]


# ------------------------------------------------------------------------------------------------ mutants of the restated pipeline
def pipeline(a, w, bias, R, mode, pack=None, bias_late=False, resid_inside=False):
    """the public modes in fp32 torch with the kernels' rounding points; the keywords are the mutants"""
    pack = pack or (lambda t: t.to(BF))
    acc = a.float() @ w.float().t()
    b = 0.0 if bias is None else bias.float()
    if mode == 1:
        return acc + b
    if mode == 0:
        return pack(pack(acc).float() + b) if bias_late else pack(acc + b)
    return pack(R + acc + b).float() if resid_inside else R + pack(acc + b).float()


def core(c, d):
    R = None if d["resid"] is None else d["resid_buf"].view(d["resid"])[:c.M, :c.N]
    return d["a"][:c.M, :c.K], d["w"][:-G.GUARD, :c.K], None if d["bias"] is None else d["bias"][:c.N], R


def new_scores(c, d, ref, got):
    """(worst |err| / E or None, wrong bits or None) of a [M, N] result under the new check"""
    if "c" in ref.exact:
        return None, int((G._bits(got) != G._bits(ref.exact["c"])).sum())
    want, E = ref.tol["c"]
    return G.check_gemm(got, want, E, G.GEMM_LIMIT, "mutant", c.K).worst, None


@pytest.mark.parametrize("mutant,mode,kw", [("a truncating pack", 0, dict(pack=_truncate)), ("bias after the rounding", 0, dict(bias_late=True)),
                                            ("bf16(R + sum)", 2, dict(resid_inside=True))])
def test_rounding_mutants_pass_the_old_metric_and_fail_the_new(mutant, mode, kw):
    c = case_named("plain", "pipe128", 300, 520, 256, mode, pad=56, roff=0)
    assert c.bias
    for profile in ("n01", "exact"):
        d = G.make_inputs(c, profile)
        ref = G.reference(c, d)
        a, w, bias, R = core(c, d)
        good, bad = pipeline(a, w, bias, R, mode), pipeline(a, w, bias, R, mode, **kw)
        old = rel_err(bad, good)
        g_worst, g_bits = new_scores(c, d, ref, good)
        worst, bits = new_scores(c, d, ref, bad)
        print(f"MUTANT {mutant} {profile}: old metric {old:.4f}, new worst |err| / E {worst}, wrong bits {bits} of {bad.numel()}")
        assert old < 1e-2, "the old metric sees it: not a mutant"
        if profile == "exact":
            assert g_bits == 0 and bits > 0
        else:
            assert g_worst <= 1.0 < worst
            if mode == 0 and "pack" in kw:
                want = ref.tol["c"][0]
                assert G.rms_ulp(bad, want) > G.RMS_RATIO * G.rms_ulp(good, want)


def test_fp32_mode_with_a_partial_through_bf16_passes_the_old_metric_and_fails_the_new():
    """an fp32-mode result whose second K-range partial went through bf16 on the way (a stream-K, split-K or slab fix-up gone
    wrong): inside 2e-5 sqrt(K) of the largest element at K = 8960, but not the exact profile's bits"""
    c = case_named("plain", "pp256", 300, 520, 8960, 1)
    d = G.make_inputs(c, "exact")
    ref = G.reference(c, d)
    a, w, bias, _ = core(c, d)
    h = c.K // 2
    good = pipeline(a, w, bias, None, 1)
    bad = a[:, :h].float() @ w[:, :h].float().t() + (a[:, h:].float() @ w[:, h:].float().t()).to(BF).float() + bias.float()
    old = rel_err(bad, good)
    wrong = int((G._bits(bad) != G._bits(ref.exact["c"])).sum())
    print(f"MUTANT fp32 partial through bf16: old metric {old:.5f} (limit {2e-5 * math.sqrt(c.K):.5f}), {wrong} of {bad.numel()} wrong bits")
    assert old < 2e-5 * math.sqrt(c.K)
    assert torch.equal(good, ref.exact["c"]) and wrong > 0.2 * bad.numel()
    with pytest.raises(AssertionError, match="differ from the exact result"):
        G.assert_bits(bad, ref.exact["c"], "partial through bf16", c.K)


def test_a_slab_summed_twice_is_no_mutant():
    """slab 0 twice, slab 1 omitted, K ranges of equal statistics: the old metric rejects it as well (recorded, then dropped)"""
    c = case_named("splitk", "policy", 200, 300, 1024, ks=16)
    d = G.make_inputs(c, "exact")
    ref = G.reference(c, d)
    slabs = [ref.exact[f"slab{s}"] for s in range(c.ks)]
    good = sum(slabs).to(BF)
    bad = (sum(slabs) - slabs[1] + slabs[0]).to(BF)
    old = rel_err(bad, good)
    print(f"MUTANT slab summed twice: old metric {old:.3f}")
    assert torch.equal(good, ref.exact["c"]) and old > 1e-2


def test_silu_rounded_once_is_inside_any_honest_bound(fake):
    """act = bf16(silu(g) t) for bf16(bf16(silu(g)) t): recorded, not rejected -- the more accurate form cannot leave E"""
    c = case_named("swiglu", "pipe", 300, 200, 128, coff=0)
    d = G.make_inputs(c, "exact")
    ref = G.reference(c, d)
    good = G.run_double(fake, c, d)
    g, t = good["gu"][:, :c.N].float(), good["gu"][:, c.N:].float()
    bad = (torch.nn.functional.silu(g) * t).to(BF)
    want, E = ref.tol["act"]
    old, chk = rel_err(bad, good["act"]), G.check_gemm(bad, want, E, G.GEMM_LIMIT, "silu once", c.K)
    print(f"MUTANT silu rounded once: old metric {old:.4f}, new worst |err| / E {chk.worst:.3f}, {int((bad != good['act']).sum())} bits differ from the double")
    assert old < 2e-2 and chk.ok and not torch.equal(bad, good["act"])


def test_rotated_v_heads_at_small_magnitude_pass_the_old_metric_and_fail_the_new(fake):
    c = case_named("qkv", "policy", 265, 4 * HD, 128)
    d = G.make_inputs(c, "exact")
    H, G_ = c.H, c.G
    d["w"][(H + G_) * HD:c.N] *= 2.0 ** -7                        # (a power of two: the profile stays exact)
    d["bias"][(H + G_) * HD:c.N] *= 2.0 ** -7
    ref = G.reference(c, d)
    good = G.run_double(fake, c, d)
    qkv = torch.cat([good["qk"], good["v"]], 1)
    bad = qkv.clone()
    v = good["v"].float().view(c.M, G_, HD)
    cs, sn = d["cos"][:c.M, None, :], d["sin"][:c.M, None, :]
    bad[:, (H + G_) * HD:] = torch.cat([v[..., :64] * cs - v[..., 64:] * sn, v[..., 64:] * cs + v[..., :64] * sn], -1).to(BF).view(c.M, -1)
    old = rel_err(bad, qkv)
    print(f"MUTANT rotated v heads: old metric {old:.4f}")
    assert old < 2e-2
    G.check_case(c, d, ref, good, "double")
    with pytest.raises(AssertionError, match="differ from the exact result"):
        G.check_case(c, d, ref, dict(qk=good["qk"], v=bad[:, (H + G_) * HD:]), "rotated v")


@pytest.mark.parametrize("mutant", ["8 columns where 3 remain", "a row beyond M"])
def test_overwrites_are_named_by_the_guard_check(mutant):
    """ldc = N = 203 as in test_gemm_unaligned_output_rows: a last-row store of 8 columns where 3 remain, or a 301st row, lands
    where the old tests have no memory to look at"""
    c = case_named("plain", "policy", 64, 203, 192)
    d = G.make_inputs(c, "exact")
    ref = G.reference(c, d)
    out = G.OutBuf(c.M, c.N, c.N + c.pad, BF, c.coff)
    out.view()[:c.M, :c.N] = ref.exact["c"]
    assert torch.equal(out.check(out.flat, "intact"), ref.exact["c"])
    flat = out.flat.clone()
    if mutant == "a row beyond M":
        out.view(flat)[c.M, :c.N] = ref.exact["c"][0]
    else:
        out.view(flat).view(-1)[c.M * c.N - 3:c.M * c.N + 5] = 1.0
    with pytest.raises(AssertionError, match=f"outside .M = {c.M}, N = {c.N}.*row {c.M}, column 0"):
        out.check(flat, mutant)
    nanned = out.flat.clone()
    out.view(nanned)[3, 5] = G.NAN
    with pytest.raises(AssertionError, match="NaN inside"):
        out.check(nanned, "operand guard read")
