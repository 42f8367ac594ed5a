"""generate(repetition_penalty = p) on the CPU: the restatement tests/penalty_ref.py against the REAL reference's tokens
(tests/golden/mid_generate_penalty.npz, tools/make_golden_generate_penalty.py), the product's decode loop on the CPU double
(tests/penalty_ops.py), the argument checks of the plugin, and the history double against a walk of the back-pointers."""
import dataclasses

import numpy as np
import pytest
import torch

from penalty_ops import PenaltyFakeOps
from penalty_ref import generate_penalised, penalty_cases, prompt_embeddings, same
from ps_slm_amd.decode import beam_search_generate
from ps_slm_amd.model import TasuModel


@pytest.fixture(scope="module")
def fixture():
    geo, sd, cases = penalty_cases()
    double = TasuModel(geo, PenaltyFakeOps(), "cpu")
    double.load_reference_state_dict(sd)
    return geo, sd, cases, double


def decode(double, geo, c, **over):
    st = double.prepare_text(c["ids"], c["am"], None, c["post_ids"], None, None)
    double.forward_projector_text(st)
    return beam_search_generate(double, st, eos_token_id=geo.eos_id, pad_token_id=geo.eos_id, **dict(c["kw"], **over)).numpy()


def test_fixture_covers_what_it_claims(fixture):
    _, _, cases, _ = fixture
    kws = [c["kw"] for c in cases]
    assert len(cases) >= 24 and {k["num_beams"] for k in kws} == {1, 2, 3, 4, 5}
    assert {k["repetition_penalty"] for k in kws} == {1.1, 1.3, 2.0, 0.8}
    assert sum(k["min_length"] > c["ids"].shape[1] + 3 for k, c in zip(kws, cases)) >= 2      # an active EOS ban
    assert sum(k["length_penalty"] != 1.0 for k in kws) >= 2
    assert {c["ids"].shape[0] for c in cases} == {1, 2, 3} and all(8 <= k["max_new_tokens"] <= 30 for k in kws)
    assert 2 * sum(c["differs"] for c in cases) >= len(cases)
    stable = [c for c in cases if c["bf16_stable"]]
    assert len(stable) >= 10 and any(c["kw"]["num_beams"] == 1 for c in stable) and any(c["kw"]["repetition_penalty"] < 1 for c in stable)


def test_restatement_in_fp32_reproduces_the_reference_on_every_case(fixture):
    geo, sd, cases, _ = fixture
    gd = dataclasses.asdict(geo)
    bad = []
    for n, c in enumerate(cases):
        emb, mask = prompt_embeddings(sd, geo, c["ids"], c["am"], c["post_ids"], "fp32")
        t = generate_penalised(sd, emb, mask, gd, mode="fp32", **c["kw"])
        if not same(t, c["tokens"]):
            bad.append((n, t.tolist(), c["tokens"].tolist()))
    assert not bad, bad


def test_product_decode_loop_on_the_double_reproduces_the_stable_cases(fixture):
    geo, _, cases, double = fixture
    bad = [(n, c["kw"]) for n, c in enumerate(cases) if c["bf16_stable"] and not same(decode(double, geo, c), c["tokens"])]
    assert not bad, bad


def test_penalty_one_is_the_call_without_the_argument(fixture):
    """repetition_penalty = 1.0 through the new argument path: the same tokens AND the same operator calls as omitting it (no
    history operator, no other top-k)."""
    geo, _, cases, double = fixture
    ops = double.ops
    for c in cases[:4]:
        kw = {k: v for k, v in c["kw"].items() if k != "repetition_penalty"}
        st = double.prepare_text(c["ids"], c["am"], None, c["post_ids"], None, None)
        double.forward_projector_text(st)
        ops.calls = []
        a = beam_search_generate(double, st, eos_token_id=geo.eos_id, pad_token_id=geo.eos_id, **kw).numpy()
        without, ops.calls = ops.calls, []
        st = double.prepare_text(c["ids"], c["am"], None, c["post_ids"], None, None)
        double.forward_projector_text(st)
        ops.calls = []
        b = beam_search_generate(double, st, eos_token_id=geo.eos_id, pad_token_id=geo.eos_id, repetition_penalty=1.0, **kw).numpy()
        with_one, ops.calls = ops.calls, None
        assert same(a, b)
        assert without == with_one and "beam_hist_update" not in without and "logprob_topk_hist" not in without
        assert "logprob_topk" in without and "beam_update" in without
    ops.calls = []
    decode(double, geo, cases[0])
    names, ops.calls = set(ops.calls), None
    assert {"beam_hist_update", "logprob_topk_hist"} <= names and "logprob_topk" not in names


def plugin():
    from fake_ops import FakeOps  # noqa: F401
    from ps_slm_amd.config import ModelConfig, TrainConfig
    from ps_slm_amd.ps_slm import model_factory
    from ps_slm_amd.synthetic import synthetic_text_batch
    tc = TrainConfig(freeze_llm=True, freeze_encoder=True, gt_emb=True, gt_emb_noise=False, ctc_posterior=True, do_psd=True)
    mc = ModelConfig(llm_path="synthetic:mid", encoder_projector="linear-silu", llm_dim=256)
    model, _ = model_factory(tc, mc, device="cpu", ops=PenaltyFakeOps(), init_seed=1234)
    raw = synthetic_text_batch(model.core.geo, 2, seed=3, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=8, noise=False)
    call = dict(input_ids=raw["input_ids"], attention_mask=raw["attention_mask"], input_features=raw["input_features"],
                input_feature_length=raw["input_feature_length"], targets=["ab cd"] * 2)
    return model, call


def test_plugin_accepts_the_penalty_and_checks_it_like_hf():
    model, call = plugin()
    model.eval()
    base = model.generate(**call, max_new_tokens=6, num_beams=2)
    assert same(model.generate(**call, max_new_tokens=6, num_beams=2, repetition_penalty=1.0), base)
    out = model.generate(**call, max_new_tokens=6, num_beams=2, repetition_penalty=2.0)
    assert out.shape[0] == 2 and out.shape[1] <= 6
    for bad in (0.0, -1.3, 0, 2, "1.3", None, True):
        with pytest.raises(ValueError, match="repetition_penalty"):
            model.generate(**call, max_new_tokens=6, repetition_penalty=bad)
    for kw in (dict(do_sample=True), dict(top_p=0.9), dict(temperature=0.7)):          # the sampling knobs stay refused
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            model.generate(**call, repetition_penalty=1.3, **kw)


def test_history_double_equals_the_walk_of_the_back_pointers_after_every_step(fixture):
    """3-beam decode: after every beam_hist_update, row m's history is what walking bp_tok / bp_par back from slot m gives."""
    geo, _, cases, double = fixture
    c = next(c for c in cases if c["kw"]["num_beams"] == 3 and c["ids"].shape[0] > 1)
    ops, seen = double.ops, []
    orig = ops.beam_hist_update

    def hook(bs):
        done_before = int(bs.ctl[1])
        orig(bs)
        n = int(bs.ctl[0])
        if done_before:
            return
        bpt, bpp = bs.bp_tok.numpy(), bs.bp_par.numpy()
        for b in range(bs.B):
            for slot in range(bs.nb):
                walk, s = [], slot
                for u in range(n - 1, -1, -1):
                    walk.append(int(bpt[u, b, s]))
                    s = int(bpp[u, b, s])
                m = b * bs.nb + slot
                assert int(bs.hist_len[m]) == n and bs.hist[m, :n].tolist() == walk[::-1], (n, b, slot)
        seen.append(n)
    ops.beam_hist_update = hook
    try:
        decode(double, geo, c)
    finally:
        del ops.beam_hist_update
    assert len(seen) >= 5 and seen == list(range(1, len(seen) + 1))


def test_history_tokens_are_penalised_once_and_listed_once():
    """The double of the top-k itself against a plain float64 statement: duplicates in the history, a banned history token."""
    ops = PenaltyFakeOps()
    g = torch.Generator().manual_seed(5)
    M, V, k = 3, 50, 6
    lg = (torch.randn(M, V, generator=g) * 3).to(torch.bfloat16)
    hist = torch.tensor([[7, 7, 9, 7, 0], [49, 1, 1, 1, 1], [3, 3, 3, 3, 3]], dtype=torch.int32)
    hl = torch.tensor([4, 2, 0], dtype=torch.int32)
    banned = torch.tensor([9], dtype=torch.int32)
    for mode in (0, 1):
        for p in (1.7, 0.6):
            val, idx = torch.zeros(M, k), torch.zeros(M, k, dtype=torch.int32)
            ops.logprob_topk_hist(lg, M, V, k, banned, 1, hist, hl, p, mode, val, idx)
            x = lg.double()
            for r in range(M):
                h = sorted(set(hist[r, :int(hl[r])].tolist()))
                row = x[r].clone()
                if mode == 1:
                    row[h] = torch.where(row[h] < 0, row[h] * p, row[h] / p)
                lp = row - torch.logsumexp(row, -1)
                if mode == 0:
                    lp[h] = torch.where(lp[h] < 0, lp[h] * p, lp[h] / p)
                lp[9] = float("-inf")
                order = np.lexsort((np.arange(V), -lp.numpy()))[:k]
                assert idx[r].tolist() == order.tolist() and len(set(idx[r].tolist())) == k
                assert float((val[r].double() - lp[order]).abs().max()) < 1e-5
