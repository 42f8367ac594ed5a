"""generate(do_sample=True, num_beams=1) on the CPU: the restatements (tests/sample_ref64.py in float64, tests/sample_ref.py in HF's
torch expressions) against HF's own warpers and against the REAL reference's tokens (tests/golden/mid_generate_sample.npz,
tools/make_golden_generate_sample.py), the product's decode loop on the CPU double (tests/sample_ops.py), and the argument rules of
the plugin."""
import dataclasses
import json

import numpy as np
import pytest
import torch

import sample_ref64 as R64
from sample_ops import SampleFakeOps
from sample_ref import draw_seed, generate_sampled, prompt_embeddings, same, sample_cases, warp
from ps_slm_amd.decode import SAMPLE_POOL, Sampling, beam_search_generate, check_sampling
from ps_slm_amd.model import TasuModel


@pytest.fixture(scope="module")
def fixture():
    geo, sd, cases = sample_cases()
    double = TasuModel(geo, SampleFakeOps(), "cpu")
    double.load_reference_state_dict(sd)
    return geo, sd, cases, double


def decode(double, geo, c, sampled=True, **over):
    st = double.prepare_text(c["ids"], c["am"], None, c["post_ids"], None, None)
    double.forward_projector_text(st)
    kw = dict(c["kw"], **over)
    sampling = check_sampling(kw.pop("temperature"), kw.pop("top_k"), kw.pop("top_p")) if sampled else None
    if not sampled:
        for k in ("temperature", "top_k", "top_p"):
            kw.pop(k)
    torch.manual_seed(c["manual_seed"])
    return beam_search_generate(double, st, num_beams=1, eos_token_id=geo.eos_id, pad_token_id=geo.eos_id, sampling=sampling, **kw).numpy()


# ------------------------------------------------------------------------------------------ the restatements against HF
def hf_warp(scores, T, top_k, top_p):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    ids = torch.zeros(scores.shape[0], 0, dtype=torch.long)
    if T != 1.0:
        scores = TemperatureLogitsWarper(T)(ids, scores)
    scores = TopKLogitsWarper(top_k=top_k)(ids, scores)
    if top_p < 1.0:
        scores = TopPLogitsWarper(top_p=top_p)(ids, scores)
    return scores


@pytest.mark.parametrize("T,top_k,top_p", [(1.0, 50, 1.0), (0.7, 50, 0.9), (1.5, 8, 0.5), (1.0, 1, 0.9), (0.7, 4, 1.0), (1.5, 50, 0.5),
                                           (1.0, 1000, 0.9)])
def test_filters_keep_what_hf_warpers_keep(T, top_k, top_p):
    """Random rows at V = 1000 and a crafted tie row: the float64 restatement's survivors and sample_ref.warp's are HF's."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(6, 1000, generator=g) * 3
    x[5, :6] = torch.tensor([3.0, 2.0, 2.0, 2.0, 1.0, 0.0]) + 20                   # ties at the threshold of top_k = 2 .. 4
    x[5, 6:] -= 10
    want = hf_warp(x.clone(), T, top_k, top_p)
    assert torch.equal(warp(x.clone(), T, top_k, top_p), want)
    s = R64.scores32(x.numpy(), None, [], 1.0, T)
    for r in range(x.shape[0]):
        row = R64.Row(s[r], top_k, top_p)
        assert not row.ambiguous
        kept = torch.nonzero(want[r] > float("-inf")).flatten().tolist()
        if r == 5 and top_p < 1.0:
            # a top-p cut inside a group of equal scores: HF's unstable sort decides which of them stay, the restatement keeps the
            # smaller ids -- the same scores survive, and everything outside the group is the same
            assert sorted(s[r, row.survivors()].tolist()) == sorted(s[r, kept].tolist())
            assert set(row.survivors().tolist()) - {1, 2, 3} == set(kept) - {1, 2, 3}
        else:
            assert row.survivors().tolist() == kept, r


def test_ties_at_the_top_k_threshold_are_kept():
    x = torch.tensor([[3.0, 2.0, 2.0, 2.0, 1.0, 0.0]])
    assert torch.nonzero(hf_warp(x.clone(), 1.0, 2, 1.0)[0] > float("-inf")).flatten().tolist() == [0, 1, 2, 3]
    assert R64.Row(R64.scores32(x.numpy(), None, [], 1.0, 1.0)[0], 2, 1.0).survivors().tolist() == [0, 1, 2, 3]
    # more ties than the pool holds: the entries above the threshold and the first ties by id (the documented departure from HF)
    s = np.zeros(40, dtype=np.float32)
    s[[7, 30]] = 1.0
    assert R64.Row(s, 5, 1.0, pool=6).survivors().tolist() == [0, 1, 2, 3, 7, 30]


def test_uniforms_are_24_bit_fractions_and_depend_on_seed_position_and_row():
    u = R64.uniforms(2 ** 63 - 5, 199, 256)
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all() and ((u.astype(np.float64) * 2 ** 24) % 1 == 0).all()
    assert len(set(u.tolist())) > 250
    assert not np.array_equal(u, R64.uniforms(2 ** 63 - 5, 198, 256)) and not np.array_equal(u, R64.uniforms(2 ** 63 - 6, 199, 256))
    assert np.array_equal(R64.uniforms(-1, 3, 4), R64.uniforms(2 ** 64 - 1, 3, 4))            # an int64 seed is its two's complement
    # the draw: the smallest survivor whose prefix sum passes u Z, for u = 0 the first, for the largest u the last survivor
    row = R64.Row(np.array([0.0, 1.0, -np.inf, 1.0], dtype=np.float32), 3, 1.0)
    assert [row.draw(v) for v in (0.0, 0.15, 0.16, 0.57, 0.58, 1 - 2 ** -24)] == [0, 0, 1, 1, 3, 3]
    assert R64.inverse_cdf(np.array([0.25, 0.0, 0.75]), 0.25) == 2 and R64.inverse_cdf(np.array([0.25, 0.0, 0.75]), 0.2) == 0


# ------------------------------------------------------------------------------------------ the fixture
def test_fixture_covers_what_it_claims(fixture):
    _, _, cases, _ = fixture
    kws = [c["kw"] for c in cases]
    assert len(cases) >= 24
    assert {k["top_k"] for k in kws} == {1, 4, 8, 50} and {k["top_p"] for k in kws} == {1.0, 0.9, 0.5}
    assert {k["temperature"] for k in kws} == {0.7, 1.0, 1.5} and {k["repetition_penalty"] for k in kws} == {1.0, 1.3}
    assert sum(k["min_length"] > c["ids"].shape[1] + 3 for k, c in zip(kws, cases)) >= 2      # an active EOS ban
    assert {c["ids"].shape[0] for c in cases} == {1, 2, 3} and all(6 <= k["max_new_tokens"] <= 16 for k in kws)
    assert sum(c["fp32_stable"] for c in cases) >= 20
    stable = [c["kw"] for c in cases if c["bf16_stable"]]
    assert len(stable) >= 6 and any(k["top_p"] < 1 and k["top_k"] > 1 for k in stable) and any(k["repetition_penalty"] != 1.0 for k in stable)
    assert all(draw_seed(c["manual_seed"]) == c["seed"] for c in cases)


def test_restatement_in_fp32_reproduces_the_reference_on_every_case(fixture):
    geo, sd, cases, _ = fixture
    gd = dataclasses.asdict(geo)
    bad = []
    for n, c in enumerate(cases):
        emb, mask = prompt_embeddings(sd, geo, c["ids"], c["am"], c["post_ids"], "fp32")
        t = generate_sampled(sd, emb, mask, gd, c["seed"], mode="fp32", **c["kw"])
        if not same(t, c["tokens"]):
            bad.append((n, t.tolist(), c["tokens"].tolist()))
    assert not bad, bad


def test_product_decode_loop_on_the_double_reproduces_the_stable_cases(fixture):
    geo, _, cases, double = fixture
    bad = []
    for n, c in enumerate(cases):
        if c["bf16_stable"]:
            t = decode(double, geo, c)
            assert int(double._last_beam.seed[0]) == c["seed"]
            if not same(t, c["tokens"]):
                bad.append((n, c["kw"], t.tolist(), c["tokens"].tolist()))
    assert not bad, bad


def test_top_k_one_and_a_tiny_top_p_decode_the_greedy_tokens(fixture):
    """top_p = 1e-6 keeps the largest only (among equal scores the smallest id: the greedy choice).  top_k = 1 keeps every token TIED
    at the maximum (HF's rule) and draws among them, so it is the greedy decode unless a row's two best bf16 logits are equal at some
    position: such decodes are told by the logits the sampler received and left out (no penalty, no ban: the scores are the logits)."""
    geo, _, cases, double = fixture
    ops, compared = double.ops, 0
    for c in cases[:8]:
        plain = dict(repetition_penalty=1.0, min_length=1)
        greedy = decode(double, geo, c, sampled=False, **plain)
        assert same(decode(double, geo, c, top_p=1e-6, **plain), greedy)
        tied = []
        ops.sample_rows = lambda lg, M, V, *a: (tied.append(bool(((lg[:M, :V].float() == lg[:M, :V].float().max(-1, keepdim=True)[0]).sum(-1) > 1).any())),
                                                SampleFakeOps.sample_rows(ops, lg, M, V, *a))[1]
        try:
            t = decode(double, geo, c, top_k=1, **plain)
        finally:
            del ops.sample_rows
        if not any(tied):
            compared += 1
            assert same(t, greedy)
    assert compared >= 4


def test_same_manual_seed_same_tokens_and_greedy_leaves_the_generator_alone(fixture):
    geo, _, cases, double = fixture
    ops = double.ops
    c = next(c for c in cases if c["kw"]["top_k"] == 50 and c["kw"]["top_p"] == 1.0)
    a, b = decode(double, geo, c), decode(double, geo, c)
    assert same(a, b)
    others = [decode(double, geo, dict(c, manual_seed=c["manual_seed"] + 1 + i)) for i in range(4)]
    assert any(not same(a, o) for o in others)                                     # the seed is used
    ops.calls = []
    try:
        st = double.prepare_text(c["ids"], c["am"], None, c["post_ids"], None, None)
        double.forward_projector_text(st)
        beam_search_generate(double, st, num_beams=1, max_new_tokens=6, eos_token_id=geo.eos_id, pad_token_id=geo.eos_id)
        greedy_calls = ops.calls
        ops.calls = []
        decode(double, geo, c)
        sampled_calls = ops.calls
    finally:
        ops.calls = None
    assert not {"sample_uniform", "sample_rows", "f32_sample_rows"} & set(greedy_calls) and "logprob_topk" in greedy_calls
    assert {"sample_uniform", "sample_rows", "beam_update"} <= set(sampled_calls) and "logprob_topk" not in sampled_calls


def test_do_sample_false_does_not_touch_the_default_generator(fixture):
    geo, _, cases, double = fixture
    c = cases[0]
    torch.manual_seed(77)
    before = torch.get_rng_state().clone()
    st = double.prepare_text(c["ids"], c["am"], None, c["post_ids"], None, None)
    double.forward_projector_text(st)
    beam_search_generate(double, st, num_beams=1, max_new_tokens=6, eos_token_id=geo.eos_id, pad_token_id=geo.eos_id)
    assert torch.equal(torch.get_rng_state(), before)
    decode(double, geo, c)                                                         # (decode() reseeds; a sampled call then draws)
    torch.manual_seed(77)
    st = double.prepare_text(c["ids"], c["am"], None, c["post_ids"], None, None)
    double.forward_projector_text(st)
    beam_search_generate(double, st, num_beams=1, max_new_tokens=6, eos_token_id=geo.eos_id, pad_token_id=geo.eos_id,
                         sampling=Sampling(1.0, 50, 1.0))
    assert not torch.equal(torch.get_rng_state(), before)


# ------------------------------------------------------------------------------------------ the plugin's argument rules
def plugin(ops=None, llm_path="synthetic:mid"):
    from ps_slm_amd.config import ModelConfig, TrainConfig
    from ps_slm_amd.ps_slm import model_factory
    from ps_slm_amd.synthetic import synthetic_text_batch
    tc = TrainConfig(freeze_llm=True, freeze_encoder=True, gt_emb=True, gt_emb_noise=False, ctc_posterior=True, do_psd=True)
    mc = ModelConfig(llm_path=llm_path, encoder_projector="linear-silu", llm_dim=256)
    model, _ = model_factory(tc, mc, device="cpu", ops=SampleFakeOps() if ops is None else ops, init_seed=1234)
    raw = synthetic_text_batch(model.core.geo, 2, seed=3, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=8, noise=False)
    call = dict(input_ids=raw["input_ids"], attention_mask=raw["attention_mask"], input_features=raw["input_features"],
                input_feature_length=raw["input_feature_length"], targets=["ab cd"] * 2)
    model.eval()
    return model, call


def test_plugin_serves_sampling_at_one_beam_and_checks_the_knobs_like_hf():
    model, call = plugin()
    torch.manual_seed(3)
    out = model.generate(**call, max_new_tokens=6, num_beams=1, do_sample=True)
    assert out.shape[0] == 2 and 1 <= out.shape[1] <= 6
    torch.manual_seed(3)
    assert same(model.generate(**call, max_new_tokens=6, num_beams=1, do_sample=True, temperature=1.0, top_k=50, top_p=1.0), out)
    torch.manual_seed(3)
    assert same(model.generate(**call, max_new_tokens=6, num_beams=1, do_sample=True, top_p=1.5), out)      # HF: >= 1 is a no-op
    model.generate(**call, max_new_tokens=6, num_beams=1, do_sample=True, temperature=0.7, top_k=8, top_p=0.9, repetition_penalty=1.3,
                   min_length=3)
    greedy = model.generate(**call, max_new_tokens=6, num_beams=1)
    assert same(model.generate(**call, max_new_tokens=6, num_beams=1, do_sample=True, top_k=1), greedy)
    for bad in (0.0, -1.0, 1, None, "0.7"):
        with pytest.raises(ValueError, match="temperature"):
            model.generate(**call, max_new_tokens=6, num_beams=1, do_sample=True, temperature=bad)
    for bad in (-1, 2.5, "50", None, True):
        with pytest.raises(ValueError, match="top_k"):
            model.generate(**call, max_new_tokens=6, num_beams=1, do_sample=True, top_k=bad)
    with pytest.raises(ValueError, match="top_p"):
        model.generate(**call, max_new_tokens=6, num_beams=1, do_sample=True, top_p=-0.1)


def test_plugin_refuses_what_is_not_built_before_any_prefill():
    model, call = plugin()
    prefills = []
    model.core.forward_llm = lambda *a, **k: prefills.append(1)                    # (would fail the decode: it must not be reached)
    with pytest.raises(NotImplementedError, match=f"top_k.*{SAMPLE_POOL}"):
        model.generate(**call, max_new_tokens=6, num_beams=1, do_sample=True, top_k=SAMPLE_POOL + 1)
    with pytest.raises(NotImplementedError, match=f"top_k=0.*{SAMPLE_POOL}"):
        model.generate(**call, max_new_tokens=6, num_beams=1, do_sample=True, top_k=0)
    for nb in (2, 4):
        with pytest.raises(NotImplementedError, match="do_sample"):
            model.generate(**call, max_new_tokens=6, num_beams=nb, do_sample=True)
    with pytest.raises(NotImplementedError, match="do_sample"):
        model.generate(**call, max_new_tokens=6, do_sample=True)                   # the default num_beams = 4: beam-sample
    for kw in (dict(top_p=0.9), dict(temperature=0.7), dict(top_k=8)):             # HF ignores these without do_sample: refused
        for nb in (1, 4):
            with pytest.raises(NotImplementedError, match=next(iter(kw))):
                model.generate(**call, max_new_tokens=6, num_beams=nb, **kw)
    assert not prefills
    from fake_ops import FakeOps
    bare, call = plugin(ops=FakeOps())
    bare.core.forward_llm = lambda *a, **k: prefills.append(1)
    with pytest.raises(NotImplementedError, match="sampling kernels"):
        bare.generate(**call, max_new_tokens=6, num_beams=1, do_sample=True)
    assert not prefills


def test_top_k_defaults_to_the_generation_config_of_the_llm_path(tmp_path):
    from ps_slm_amd.config import ModelConfig
    from ps_slm_amd.ps_slm import default_top_k
    assert default_top_k(ModelConfig(llm_path="synthetic:mid")) == 50 and default_top_k(ModelConfig(llm_path=str(tmp_path))) == 50
    (tmp_path / "generation_config.json").write_text(json.dumps(dict(do_sample=True, temperature=0.7)))
    assert default_top_k(ModelConfig(llm_path=str(tmp_path))) == 50               # a file without the key
    (tmp_path / "generation_config.json").write_text(json.dumps(dict(do_sample=True, top_k=20, top_p=0.8)))
    assert default_top_k(ModelConfig(llm_path=str(tmp_path))) == 20
    seen = []

    class Spy(SampleFakeOps):
        def sample_rows(self, *a, **k):
            seen.append(a[10])                                                     # top_k
            return SampleFakeOps.sample_rows(self, *a, **k)

    model, call = plugin(ops=Spy())
    model.generate(**call, max_new_tokens=3, num_beams=1, do_sample=True)
    model.model_config = ModelConfig(llm_path=str(tmp_path), encoder_projector="linear-silu", llm_dim=256)
    model.generate(**call, max_new_tokens=3, num_beams=1, do_sample=True)
    model.generate(**call, max_new_tokens=3, num_beams=1, do_sample=True, top_k=7)
    assert set(seen[:1]) == {50} and 20 in seen and seen[-1] == 7 and set(seen) == {50, 20, 7}
