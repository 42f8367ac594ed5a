"""generate(do_sample=True, num_beams > 1) on the CPU: the restatements (tests/beam_sample_ref64.py in float64, tests/beam_sample_ref.py
in HF's torch expressions) against HF's own warpers and against the REAL reference's tokens (tests/golden/mid_generate_beam_sample.npz,
tools/make_golden_generate_beam_sample.py), the product's decode loop and BeamState.update_drawn on the CPU double
(tests/beam_sample_ops.py), the draw's distribution, and the argument rules of the plugin."""
import dataclasses

import numpy as np
import pytest
import torch

import beam_sample_ref64 as R64
import sample_ref64 as S64
from beam_sample_ops import BeamSampleFakeOps
from beam_sample_ref import beam_sample_cases, draw_seed, generate_beam_sampled, prompt_embeddings, same, warp2
from sample_ops import SampleFakeOps
from ps_slm_amd.decode import NEG, BeamState, beam_search_generate, check_sampling
from ps_slm_amd.model import TasuModel


@pytest.fixture(scope="module")
def fixture():
    geo, sd, cases = beam_sample_cases()
    double = TasuModel(geo, BeamSampleFakeOps(), "cpu")
    double.load_reference_state_dict(sd)
    return geo, sd, cases, double


def decode(double, geo, c, **over):
    st = double.prepare_text(c["ids"], c["am"], None, c["post_ids"], None, None)
    double.forward_projector_text(st)
    kw = dict(c["kw"], **over)
    sampling = check_sampling(kw.pop("temperature"), kw.pop("top_k"), kw.pop("top_p"))
    torch.manual_seed(c["manual_seed"])
    return beam_search_generate(double, st, eos_token_id=geo.eos_id, pad_token_id=geo.eos_id, sampling=sampling, **kw).numpy()


def plugin(ops=None):
    from ps_slm_amd.config import ModelConfig, TrainConfig
    from ps_slm_amd.ps_slm import model_factory
    from ps_slm_amd.synthetic import synthetic_text_batch
    tc = TrainConfig(freeze_llm=True, freeze_encoder=True, gt_emb=True, gt_emb_noise=False, ctc_posterior=True, do_psd=True)
    mc = ModelConfig(llm_path="synthetic:mid", encoder_projector="linear-silu", llm_dim=256)
    model, _ = model_factory(tc, mc, device="cpu", ops=BeamSampleFakeOps() if ops is None else ops, init_seed=1234)
    raw = synthetic_text_batch(model.core.geo, 2, seed=3, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=8, noise=False)
    call = dict(input_ids=raw["input_ids"], attention_mask=raw["attention_mask"], input_features=raw["input_features"],
                input_feature_length=raw["input_feature_length"], targets=["ab cd"] * 2)
    model.eval()
    return model, call


# ------------------------------------------------------------------------------------------ the RNG and the draw
def test_key_uniforms_are_exact_odd_multiples_of_two_to_the_minus_24_and_never_0_or_1():
    c = np.concatenate([np.arange(4096), (2 ** 31 - 3 + np.arange(8)), 255 * 151936 + np.arange(151936 - 8, 151936)]).astype(np.int64)
    for seed, t in ((2 ** 63 - 5, 199), (-1, 0), (0, 0), (-2 ** 63, 2047)):
        bits = R64.key_bits(seed, t, c)
        key = (int(seed) & S64.M64) ^ ((t * S64.GOLD) & S64.M64)                       # python integers, modulo 2^64
        want = [S64.mix64((key + int(ci) * S64.ODD) & S64.M64) >> 41 for ci in c]
        assert bits.tolist() == want and bits.min() >= 0 and bits.max() < 2 ** 23
        u = R64.key_uniforms(seed, t, c)
        assert u.dtype == np.float32 and (u > 0).all() and (u < 1).all()
        assert np.array_equal(u.astype(np.float64) * 2 ** 24, 2 * bits + 1)           # (bits + 1/2) * 2^-23, nothing rounded
        assert len(set(bits[:4096].tolist())) > 4000
    assert np.array_equal(R64.key_bits(-1, 3, c), R64.key_bits(2 ** 64 - 1, 3, c))    # an int64 seed is its two's complement
    assert not np.array_equal(R64.key_bits(5, 3, c), R64.key_bits(5, 4, c)) and not np.array_equal(R64.key_bits(5, 3, c), R64.key_bits(6, 3, c))
    # the extreme uniforms give finite keys: G in [-log(24 log 2), 23 log 2 + ...]
    for b in (0, 2 ** 23 - 1):
        u = np.float32((b + 0.5) * 2.0 ** -23)
        assert np.isfinite(-np.log(-np.log(u)))


def test_draw_is_sampling_without_replacement_in_proportion_to_softmax_in_plackett_luce_order():
    """6 candidates of a toy utterance (2 beams x 3 tokens), 20 000 fixed seeds: the first slot's frequencies against softmax(a), the
    (slot 0, slot 1) pair frequencies against p_i p_j / (1 - p_i), each within 4 standard errors of its binomial.  (Checked on the
    restatement alone: it involves no code under test.)"""
    a = np.array([[0.0, -0.7, -1.9, -0.3, -2.5, -1.1]], dtype=np.float32)
    p = np.exp(a[0].astype(np.float64))
    p /= p.sum()
    N = 20000
    first, pair = np.zeros(6), np.zeros((6, 6))
    for seed in range(N):
        i, j = R64.draw_flat(a, 1000003 * seed + 17, seed % 7, 2)[0]
        first[i] += 1
        pair[i, j] += 1
    assert np.trace(pair) == 0                                                         # without replacement
    se = np.sqrt(p * (1 - p) / N)
    assert (np.abs(first / N - p) <= 4 * se).all(), (first / N, p, se)
    pl = p[:, None] * p[None, :] / (1 - p[:, None])
    np.fill_diagonal(pl, 0.0)
    se2 = np.sqrt(pl * (1 - pl) / N)
    assert (np.abs(pair / N - pl) <= 4 * se2).all(), (pair / N, pl)


def test_a_filtered_token_is_never_drawn_and_equal_keys_go_by_beam_then_token():
    a = np.full((2, 12), -np.inf, dtype=np.float32)
    a[0, [1, 5, 7, 10]] = [-0.5, -1.0, -1.0e9, -1.0e9]
    a[1, [0, 2, 6, 8, 9]] = [-1.0e9, -1.0e9, -3.0, -1.0e9, -0.1]
    for seed in range(50):
        ix = R64.draw_flat(a, seed, 3, 4)
        assert set(ix[0].tolist()) == {1, 5, 7, 10} and ix[0, 2:].tolist() == [7, 10]      # -1e9 + G rounds to -1e9: equal keys
        assert set(ix[1, :2].tolist()) == {6, 9} and ix[1, 2:].tolist() == [0, 2]


# ------------------------------------------------------------------------------------------ the restatements against HF
@pytest.mark.parametrize("T,top_k,top_p", [(1.0, 50, 1.0), (0.7, 50, 0.9), (1.5, 8, 0.5), (1.0, 1, 0.9), (0.7, 2, 1.0), (1.5, 50, 0.5), (1.0, 1, 1e-6)])
def test_filters_keep_what_hf_warpers_keep_with_two_tokens_to_keep(T, top_k, top_p):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    g = torch.Generator().manual_seed(12)
    x = torch.log_softmax(torch.randn(6, 1000, generator=g) * 3, -1)
    ids = torch.zeros(6, 0, dtype=torch.long)
    want = x.clone()
    if T != 1.0:
        want = TemperatureLogitsWarper(T)(ids, want)
    want = TopKLogitsWarper(top_k=top_k, min_tokens_to_keep=2)(ids, want)
    if top_p < 1.0:
        want = TopPLogitsWarper(top_p=top_p, min_tokens_to_keep=2)(ids, want)
    assert torch.equal(warp2(x.clone(), T, top_k, top_p), want)
    assert ((want > float("-inf")).sum(-1) >= 2).all()
    for r in range(6):
        row = R64.Row(x[r].numpy(), None, [], 1.0, T, top_k, top_p, 0.0, 1, 0, r, 4, False)
        # (the row reference starts from logits: log_softmax of log-probs is the identity up to rounding)
        if not row.ambiguous:
            assert np.sort(row.ids[:row.cut]).tolist() == torch.nonzero(want[r] > float("-inf")).flatten().tolist(), r


def test_row_reference_top_k_one_is_top_k_two_and_fillers_follow_the_survivors():
    g = np.random.default_rng(5)
    x = np.round(g.normal(size=400) * 24) / 8
    a, b = (R64.Row(x, None, [], 1.0, 1.0, k, 1.0, -2.5, 77, 3, 1, 6, False) for k in (1, 2))
    assert a.want.tolist() == b.want.tolist() and 2 <= len(a.want) <= 6
    n = len(a.want)
    q = [a.pos[int(v)] for v in a.want]
    key, val, idx = np.full(6, -np.inf, np.float32), np.full(6, -np.inf, np.float32), np.full(6, R64.NONE, np.int64)
    key[:n], val[:n], idx[:n] = a.key[q], a.a[q], a.want
    assert a.check(key, val, idx) is None
    assert a.check(key[::-1].copy(), val[::-1].copy(), idx[::-1].copy()) is not None
    key2 = key.copy()
    key2[0] += 1e-3
    assert "key" in a.check(key2, val, idx)


# ------------------------------------------------------------------------------------------ the fixture
def test_fixture_covers_what_it_claims(fixture):
    _, _, cases, _ = fixture
    kws = [c["kw"] for c in cases]
    assert len(cases) >= 24
    assert {k["num_beams"] for k in kws} == {2, 4, 5, 6, 16} and {k["top_k"] for k in kws} == {1, 2, 8, 50}
    assert {k["top_p"] for k in kws} == {1.0, 0.9, 0.5} and {k["temperature"] for k in kws} == {0.7, 1.0, 1.5}
    assert {k["repetition_penalty"] for k in kws} == {1.0, 1.3} and any(k["length_penalty"] != 1.0 for k in kws)
    assert sum(k["min_length"] > c["ids"].shape[1] + 3 for k, c in zip(kws, cases)) >= 2      # an active EOS ban
    assert {c["ids"].shape[0] for c in cases} == {1, 2, 3} and all(4 <= k["max_new_tokens"] <= 12 for k in kws)
    assert sum(c["fp32_stable"] for c in cases) >= 20
    stable = [c["kw"] for c in cases if c["bf16_stable"]]
    assert len(stable) >= 6 and any(k["num_beams"] >= 6 for k in stable) and any(k["repetition_penalty"] != 1.0 for k in stable)
    assert all(draw_seed(c["manual_seed"]) == c["seed"] for c in cases)


def test_restatement_in_fp32_reproduces_the_reference_on_every_case(fixture):
    geo, sd, cases, _ = fixture
    gd = dataclasses.asdict(geo)
    bad = []
    for n, c in enumerate(cases):
        emb, mask = prompt_embeddings(sd, geo, c["ids"], c["am"], c["post_ids"], "fp32")
        t = generate_beam_sampled(sd, emb, mask, gd, c["seed"], mode="fp32", **c["kw"])
        if not same(t, c["tokens"]):
            bad.append((n, t.tolist(), c["tokens"].tolist()))
    assert not bad, bad


class _Posteriors:
    """An encoder tokenizer's stand-in that hands generate() the fixture's posterior ids, one utterance per call."""

    def __init__(self, post_ids):
        self.rest = list(post_ids)

    def encode(self, text):
        return self.rest.pop(0)


def test_plugin_generate_on_the_double_reproduces_the_fp32_stable_cases(fixture):
    """generate() of the plugin on the fixture's weights, the CPU double underneath.  The double restates the bf16 kernels (there is
    no CPU double of the fp32 decode path: tests/fake_ops.py has no f32_* operators), so among the fp32-stable cases it can be held to
    the ones whose tokens also survive bf16 rounding, the ``bf16_stable`` flag of the restatement: 8 of the 24.  (Measured: the
    double reproduces 17 of the 24; none of the 7 it misses is flagged bf16-stable.)  All 24 fp32-stable cases are held on the fp32 path itself, tests/test_gpu_generate_beam_sample.py."""
    geo, sd, cases, _ = fixture
    model, _ = plugin()
    assert dataclasses.asdict(model.core.geo) == dataclasses.asdict(geo)
    model.core.load_reference_state_dict(sd)
    bad, n_run = [], 0
    for n, c in enumerate(cases):
        if not (c["fp32_stable"] and c["bf16_stable"]):
            continue
        n_run += 1
        model.encoder_tokenizer = _Posteriors(c["post_ids"])
        B = c["ids"].shape[0]
        torch.manual_seed(c["manual_seed"])
        t = model.generate(input_ids=c["ids"], attention_mask=c["am"], input_features=torch.zeros(B, 8, geo.feat_dim),
                           input_feature_length=torch.full((B,), 8), targets=["x"] * B, do_sample=True, **c["kw"])
        assert int(model.core._last_beam.seed[0]) == c["seed"]
        if not same(t.numpy(), c["tokens"]):
            bad.append((n, c["kw"], t.tolist(), c["tokens"].tolist()))
    assert n_run >= 6 and not bad, bad


def test_product_decode_loop_on_the_double_reproduces_the_stable_cases(fixture):
    geo, _, cases, double = fixture
    bad = []
    for n, c in enumerate(cases):
        if c["bf16_stable"]:
            t = decode(double, geo, c)
            if not same(t, c["tokens"]):
                bad.append((n, c["kw"], t.tolist(), c["tokens"].tolist()))
    assert not bad, bad


# ------------------------------------------------------------------------------------------ BeamState.update_drawn
def row_candidates(acc, seed, t, nb, V, K):
    """What tasu_beam_sample_rows hands over for HF's accumulated scores acc [B, nb * V]: per row the K largest float32 keys."""
    B = acc.shape[0]
    key = np.full((B, nb, K), -np.inf, np.float32)
    val, tok = key.copy(), np.full((B, nb, K), R64.NONE, np.int64)
    for b in range(B):
        for j in range(nb):
            row = acc[b, j * V:(j + 1) * V]
            ids = np.flatnonzero(row > -np.inf)
            k = (row[ids] + R64.gumbel32(seed, t, (b * nb + j) * V + ids)).astype(np.float32)
            o = np.lexsort((ids, -k.astype(np.float64)))[:K]
            key[b, j, :len(o)], val[b, j, :len(o)], tok[b, j, :len(o)] = k[o], row[ids][o], ids[o]
    return key, val, tok


def test_update_drawn_equals_the_restatement_after_every_step(fixture):
    geo, sd, cases, _ = fixture
    gd = dataclasses.asdict(geo)
    seen = set()
    for c in cases:
        kw = c["kw"]
        if kw["num_beams"] in seen and kw["length_penalty"] == 1.0:
            continue
        seen.add(kw["num_beams"])
        emb, mask = prompt_embeddings(sd, geo, c["ids"], c["am"], c["post_ids"], "fp32")
        steps = []
        toks = generate_beam_sampled(sd, emb, mask, gd, c["seed"], mode="fp32", steps=steps, **kw)
        B, nb, V = c["ids"].shape[0], kw["num_beams"], geo.llm_vocab
        state = BeamState(B, nb, kw["max_new_tokens"], geo.eos_id, geo.eos_id, kw["length_penalty"], max(kw["min_length"] - emb.shape[1], 0))
        for t, s in enumerate(steps):
            assert not state.done
            key, val, tok = row_candidates(s["acc"].numpy(), c["seed"], t, nb, V, 2 * nb)
            nt, npar = state.update_drawn(key, val, tok)
            assert np.array_equal(nt, s["next_tok"].numpy()) and np.array_equal(npar, s["next_parent"].numpy()), t
            assert np.array_equal(state.run_seq, s["run_seq"].numpy()) and np.array_equal(state.run_scores, s["run_scores"].numpy()), t
            assert np.array_equal(state.fin_seq, s["fin_seq"].numpy()) and np.array_equal(state.fin_scores, s["fin_scores"].numpy()), t
            assert np.array_equal(state.fin_len, s["fin_len"].numpy()) and np.array_equal(state.is_fin, s["is_fin"].numpy()), t
            assert np.array_equal(state.unsat, s["unsat"].numpy()) and state.done == s["done"], t
        assert state.done and same(state.result(), toks)
    assert seen == {2, 4, 5, 6, 16}


def test_update_drawn_treats_a_filler_as_token_zero_at_minus_infinity():
    state = BeamState(1, 2, 4, 9, 9)
    key = np.array([[[1.0, -np.inf, -np.inf, -np.inf], [3.0, 2.0, 0.5, -np.inf]]], np.float32)
    val = np.array([[[-1.0, -np.inf, -np.inf, -np.inf], [-4.0, -3.0, -2.0, -np.inf]]], np.float32)
    tok = np.array([[[5, R64.NONE, R64.NONE, R64.NONE], [6, 7, 8, R64.NONE]]])
    nt, npar = state.update_drawn(key, val, tok)
    # draw order: (1, 6), (1, 7), (0, 5), (1, 8); running = the best two BY SCORE: (0, 5) at -1, (1, 8) at -2
    assert nt.tolist() == [[5, 8]] and npar.tolist() == [[0, 1]] and state.run_scores.tolist() == [[-1.0, -2.0]]


# ------------------------------------------------------------------------------------------ the decode loop
def test_top_k_one_decodes_as_top_k_two(fixture):
    geo, sd, cases, double = fixture
    gd = dataclasses.asdict(geo)
    for c in [c for c in cases if c["kw"]["top_k"] == 1][:3]:
        assert same(decode(double, geo, c, top_k=1), decode(double, geo, c, top_k=2))
        emb, mask = prompt_embeddings(sd, geo, c["ids"], c["am"], c["post_ids"], "fp32")
        assert same(generate_beam_sampled(sd, emb, mask, gd, c["seed"], mode="fp32", **dict(c["kw"], top_k=2)), c["tokens"])


def test_other_calls_issue_the_operator_calls_of_the_one_beam_double(fixture):
    """A beam search without do_sample and a one-beam sampled call, on the double WITH the beam-sample operators and on tests/
    sample_ops.py's double without them: the same operator calls in the same order, none of them a beam-sample one."""
    geo, sd, cases, double = fixture
    bare = TasuModel(geo, SampleFakeOps(), "cpu")
    bare.load_reference_state_dict(sd)
    c = cases[0]
    new = {"beam_sample_rows", "f32_beam_sample_rows", "beam_update_drawn"}

    def calls(model, nb, sampling, penalty=1.0):
        st = model.prepare_text(c["ids"], c["am"], None, c["post_ids"], None, None)
        model.forward_projector_text(st)
        model.ops.calls = []
        try:
            torch.manual_seed(5)
            beam_search_generate(model, st, num_beams=nb, max_new_tokens=5, eos_token_id=geo.eos_id, pad_token_id=geo.eos_id,
                                 sampling=sampling, repetition_penalty=penalty)
            return model.ops.calls
        finally:
            model.ops.calls = None

    calls(double, 4, None), calls(bare, 4, None)               # (a model's first decode also registers its decode weights)
    for nb, sampling, penalty in ((4, None, 1.0), (6, None, 1.3), (1, None, 1.0), (1, check_sampling(0.7, 8, 0.9), 1.0),
                                  (1, check_sampling(1.0, 50, 1.0), 1.3)):
        got, want = calls(double, nb, sampling, penalty), calls(bare, nb, sampling, penalty)
        assert got == want and not new & set(got), (nb, sampling)
        assert ("sample_rows" in got) == (sampling is not None) and ("logprob_topk" in got or "logprob_topk_hist" in got) == (sampling is None)
    got = calls(double, 4, check_sampling(0.7, 8, 0.9), 1.3)
    assert {"beam_sample_rows", "beam_update_drawn", "beam_hist_update"} <= set(got)
    assert not {"sample_uniform", "sample_rows", "logprob_topk", "logprob_topk_hist", "beam_update"} & set(got)
    assert "beam_hist_update" not in calls(double, 4, check_sampling(0.7, 8, 0.9))


def test_first_position_fills_its_slots_from_the_absent_beams_and_the_decode_ends(fixture):
    """Tiny top_p and T leave every row its two largest tokens: at the first position beam 0 supplies two finite candidates and beams
    >= 1, at about -1e9, the other 2 nb - 2."""
    geo, _, cases, double = fixture
    c = next(c for c in cases if c["kw"]["num_beams"] == 4 and c["ids"].shape[0] >= 2)
    ops, seen = double.ops, []
    ops.beam_update_drawn = lambda keys, vals, idx, bs: (seen.append((keys.clone(), vals.clone(), idx.clone(), bs.run_scores.clone())),
                                                         BeamSampleFakeOps.beam_update_drawn(ops, keys, vals, idx, bs))[1]
    try:
        t = decode(double, geo, c, top_p=1e-6, temperature=0.05, top_k=50, min_length=1, repetition_penalty=1.0, max_new_tokens=6)
    finally:
        del ops.beam_update_drawn
    B, nb = c["ids"].shape[0], 4
    assert t.shape[0] == B and 1 <= t.shape[1] <= 6 and 2 <= len(seen) <= 6
    keys, vals, idx, _ = seen[0]
    vals, idx = vals.view(B, nb, 2 * nb), idx.view(B, nb, 2 * nb)
    assert (idx[:, :, :2] != R64.NONE).all() and (idx[:, :, 2:] == R64.NONE).all()         # two survivors per row
    assert (vals[:, 0, :2] > -1e3).all() and ((vals[:, 1:, :2] - NEG).abs() <= 1e3).all()
    run = seen[1][3].view(B, nb)                                                           # running scores after the first position
    assert (run[:, :2] > -1e3).all() and ((run[:, 2:] - NEG).abs() <= 1e3).all()


def test_same_manual_seed_same_tokens_and_another_seed_differs(fixture):
    geo, _, cases, double = fixture
    c = next(c for c in cases if c["kw"]["top_k"] == 50 and c["kw"]["num_beams"] == 4)
    a = decode(double, geo, c)
    assert same(a, decode(double, geo, c))
    assert any(not same(a, decode(double, geo, dict(c, manual_seed=c["manual_seed"] + 1 + i))) for i in range(4))


# ------------------------------------------------------------------------------------------ the plugin
def test_plugin_serves_do_sample_at_the_default_four_beams():
    model, call = plugin()
    torch.manual_seed(3)
    out = model.generate(**call, max_new_tokens=6, do_sample=True)                          # the reference's own keyword set
    assert out.shape[0] == 2 and 1 <= out.shape[1] <= 6
    assert model.core._last_beam.nb == 4 and model.core._last_beam.sampling is not None
    torch.manual_seed(3)
    assert same(model.generate(**call, max_new_tokens=6, do_sample=True, num_beams=4, temperature=1.0, top_k=50, top_p=1.0), out)
    for nb in (2, 5, 6, 16):
        o = model.generate(**call, max_new_tokens=5, num_beams=nb, do_sample=True, top_p=0.9, temperature=0.7, repetition_penalty=1.3)
        assert o.shape[0] == 2 and 1 <= o.shape[1] <= 5
    with pytest.raises(ValueError, match="num_beams"):
        model.generate(**call, max_new_tokens=6, num_beams=17, do_sample=True)
    with pytest.raises(ValueError, match="temperature"):
        model.generate(**call, max_new_tokens=6, do_sample=True, temperature=0.0)


def test_plugin_still_refuses_knobs_without_do_sample_and_unbuilt_top_k_before_any_prefill():
    model, call = plugin()
    prefills = []
    model.core.forward_llm = lambda *a, **k: prefills.append(1)
    for kw in (dict(top_p=0.9), dict(temperature=0.7), dict(top_k=8)):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            model.generate(**call, max_new_tokens=6, **kw)
    with pytest.raises(NotImplementedError, match="top_k=0"):
        model.generate(**call, max_new_tokens=6, do_sample=True, top_k=0)
    with pytest.raises(NotImplementedError, match="top_k=1025"):
        model.generate(**call, max_new_tokens=6, do_sample=True, top_k=1025)
    bare, call = plugin(ops=SampleFakeOps())
    bare.core.forward_llm = lambda *a, **k: prefills.append(1)
    with pytest.raises(NotImplementedError, match="do_sample.*beam_sample_rows.*beam_update_drawn"):
        bare.generate(**call, max_new_tokens=6, do_sample=True)
    assert not prefills


# ------------------------------------------------------------------------------------------ the row kernels' cases
@pytest.mark.parametrize("n", range(len(R64.KERNEL_CASES)))
def test_kernel_cases_stay_under_the_ambiguity_cap_on_the_reference_alone(n):
    """The cases tests/test_gpu_generate_beam_sample.py holds the row kernels to: at most 10 % of a case's rows have a class that may
    come out either way, and every row hands over min(K, survivors) >= 2 candidates."""
    c = R64.KERNEL_CASES[n]
    for fast in (False, True):
        rows = R64.kernel_rows(c, fast)
        assert len(rows) == c.M and sum(r.ambiguous for r in rows) <= R64.AMBIGUOUS_CAP * c.M, (c, fast, sum(r.ambiguous for r in rows))
        assert all(2 <= len(r.want) <= c.K for r in rows)
    ks = R64.KERNEL_CASES
    assert {c.V for c in ks} == {1000, 151936} and {c.M for c in ks} == {2, 10, 64} and {c.K for c in ks} == {4, 10, 32}
    assert {(c.M, c.K) for c in ks if c.V == 1000} == {(M, K) for M in (2, 10, 64) for K in (4, 10, 32)}
    assert {c.first for c in ks} == {True, False} and {c.hist for c in ks} == {True, False}
