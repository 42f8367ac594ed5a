"""Qwen3 decoders on the GPU (per-head q/k RMSNorm, csrc/qk_norm.hip; the bf16 path, frozen decoder).

At ``synthetic:mid-qwen3`` (through model_factory): one training step against the CPU double (tests/qwen3_ops.py) and the bf16
restatement (tests/qwen3_ref.py) at the bars of tests/test_gpu_model.py::test_step_vs_double_and_oracle, and against the REAL
reference's fp32 fixture (tests/golden/mid_qwen3_step.npz) at those of ::test_step_vs_reference_golden; the labelled-rows tail
against the all-rows schedule; graph replay == eager and run == run, bit for bit; generate() token-exact on every bf16_stable case
of tests/golden/mid_qwen3_generate.npz and the same tokens with decode graphs on and off on ALL cases (1 - 16 beams, more than 64
beam rows among them); one case with repetition_penalty and one with do_sample at the restatement's tokens.

At ``synthetic:qwen3-1.7b``, once: the property of tests/test_gpu_fullsize.py::test_full_size_decode_scores_equal_full_forward --
each returned hypothesis' beam score equals the log-softmax sum of a plain forward over prompt + tokens, which ties the append
kernel, the prefill kernel and the plain q|k|v GEMM together on the decode GEMM routes of K = 2048 / 6144 -- and a 4-utterance
training step: finite loss, bitwise repeatable, replay == eager.

Measured on MI355X (9 tests, a few seconds for the file; the QWEN3 lines): step loss 7.378750 against the double's 7.378004 and the
restatement's 7.378301, logits 0.47 % of the logit scale, gradients 1.2 % relative L2; reference fixture: loss 10.4072 against
10.4090 (text), 10.3258 against 10.3327 (audio), logits 1.6 % / 2.1 % (both asserted at 3 %); 20 of 24 decode cases token-exact, the 15 stable ones among
them; decode scores against the full forward: 0.060 nats over 6 tokens at 80 beam rows (mid), 0.078 over 7 at Qwen3-1.7B."""
import dataclasses
import math

import pytest
import torch

import qwen3_ref as R
from penalty_ref import same
from ps_slm_amd.config import ModelConfig, TrainConfig
from ps_slm_amd.model import TasuModel
from ps_slm_amd.synthetic import qwen3_state_dict, synthetic_text_batch
from qwen3_ops import Qwen3FakeOps

pytestmark = pytest.mark.gpu


def cosine(a, b):
    return float(torch.nn.functional.cosine_similarity(a.flatten().float().cpu(), b.flatten().float().cpu(), dim=0))


def factory(llm_path, llm_dim, **kw):
    from ps_slm_amd.ps_slm import model_factory
    tc = TrainConfig(freeze_llm=True, freeze_encoder=True, gt_emb=True, gt_emb_noise=False, ctc_posterior=True, do_psd=True, use_fp16=True)
    mc = ModelConfig(llm_path=llm_path, encoder_projector="linear-silu", llm_dim=llm_dim, **({"encoder_dim": 25055} if llm_dim != 256 else {}))
    return model_factory(tc, mc, init_seed=1234, **kw)[0].core


def run_step(core, batch, audio=False):
    if audio:
        st = core.prepare_audio(batch["input_ids"], batch["attention_mask"], batch["labels"], batch["input_features"],
                                batch["input_feature_length"])
    else:
        st = core.prepare_text(batch["input_ids"], batch["attention_mask"], batch["labels"], batch["post_ids"], batch.get("alphas"),
                               batch.get("keeps"))
        core.forward_projector_text(st)
    core.forward_llm(st)
    core.backward(st)
    if core.device.type == "cuda":
        torch.cuda.synchronize()
    return st


@pytest.fixture(scope="module")
def mid():
    gm = factory("synthetic:mid-qwen3", 256, with_encoder=True)
    assert gm.geo.qk_norm and gm.arith == "bf16" and gm.device.type == "cuda"
    return gm.geo, gm


def test_step_vs_double_and_restatement(mid):
    geo, gm = mid
    sd = qwen3_state_dict(geo, 2026)
    gm.load_reference_state_dict(sd)
    cm = TasuModel(geo, Qwen3FakeOps(), "cpu")
    cm.load_reference_state_dict(sd)
    batch = synthetic_text_batch(geo, 3, seed=31, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=12, noise=True,
                                 drop_prob=0.15, ragged=True)
    sg, sc = run_step(gm, batch), run_step(cm, batch)
    lg, lc = sg.dev["loss_out"].cpu(), sc.dev["loss_out"]
    valid = torch.from_numpy(sc.plan.key_mask[:, :sc.S].astype(bool))
    a, b = gm.logits_view(sg).float().cpu()[valid], cm.logits_view(sc).float()[valid]
    gg, gc = gm.projector_grads(), cm.projector_grads()
    out, grads = R.loss_and_projector_grads(sd, batch, dataclasses.asdict(geo), "bf16")
    print(f"QWEN3 step: loss gpu {float(lg[0]):.6f} double {float(lc[0]):.6f} restatement {float(out['loss'].detach()):.6f}; logits "
          f"{float((a - b).abs().max() / b.abs().max()):.4f}; grads rel L2 {max(R.rel_l2(gg[k].cpu(), gc[k]) for k in gc):.4f}")
    assert abs(float(lg[0]) - float(lc[0])) < 2e-3 and abs(float(lg[1]) - float(lc[1])) <= 1.0 / sc.plan.count + 1e-6
    assert float((a - b).abs().max() / b.abs().max()) < 2e-2
    for k in gc:
        assert cosine(gg[k], gc[k]) > 0.9995, k
        assert R.rel_l2(gg[k].cpu(), gc[k]) < 3e-2, k
    assert abs(float(lg[0]) - float(out["loss"].detach())) < 5e-3
    for k, g in grads.items():
        assert cosine(gg[k], g) > 0.999, k


@pytest.mark.parametrize("tag", ["text", "audio"])
def test_step_vs_reference_fixture(mid, tag):
    """the REAL reference in fp32, both batches: |loss - ref| < 2e-2, logits within 3e-2 of the logit scale; projector gradients
    cosine 0.995 (text) / 0.99 (audio: tests/test_gpu_model.py::test_audio_step_without_merging's)"""
    geo, gm = mid
    _, sd, batch, z = R.step_case()
    gm.load_reference_state_dict(sd)
    st = run_step(gm, batch, tag == "audio")
    valid = torch.from_numpy(st.plan.key_mask[:, :st.S].astype(bool))
    lg = gm.logits_view(st).float().cpu()[:, :, torch.from_numpy(z["cols"])]
    ref = torch.from_numpy(z[f"{tag}_logits_cols"])
    err = float((lg - ref)[valid].abs().max() / ref[valid].abs().max())
    print(f"QWEN3 reference {tag}: loss {float(st.dev['loss_out'][0]):.6f} ref {float(z[tag + '_loss']):.6f}; logits {err:.4f}")
    assert abs(float(st.dev["loss_out"][0]) - float(z[f"{tag}_loss"])) < 2e-2
    assert err < 3e-2
    for k, g in gm.projector_grads().items():
        assert cosine(g, torch.from_numpy(z[f"{tag}_grad." + k[len("encoder_projector."):]])) > (0.995 if tag == "text" else 0.99), k


def test_graph_replay_tail_and_repeatability(mid):
    """run == run and graph replay == eager, bit for bit, on the full-materialisation step and on the throughput step with the
    labelled-rows tail; the tail against the all-rows schedule: the same loss and gradients bit for bit"""
    from ps_slm_amd.ops import HipOps
    geo, gm = mid
    sd = qwen3_state_dict(geo, 2026)
    gm.load_reference_state_dict(sd)
    lean, flat = TasuModel(geo, HipOps(), "cuda", keep_logits=False), TasuModel(geo, HipOps(), "cuda", keep_logits=False)
    for m in (lean, flat):
        m.load_reference_state_dict(sd)
    lean.tail_rows, flat.tail_rows = True, False
    batch = synthetic_text_batch(geo, 3, seed=77, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=12, noise=False,
                                 ragged=True)

    def one(model):
        st = model.prepare_text(batch["input_ids"], batch["attention_mask"], batch["labels"], batch["post_ids"], None, None)
        model.run_forward_text(st)
        model.run_backward(st)
        torch.cuda.synchronize()
        return st, st.dev["loss_out"].clone(), model.proj.g.clone()

    res = {}
    for name, model in (("full", gm), ("lean", lean), ("flat", flat)):
        model.use_graphs = False
        st, l0, g0 = one(model)
        assert math.isfinite(float(l0[0])) and torch.equal(one(model)[1], l0) and torch.equal(one(model)[2], g0)
        model.use_graphs = True
        outs = [one(model) for _ in range(4)]                    # eager warm-up, capture + replay, replay, replay
        assert len(model._graphs) == 2
        model.use_graphs = False
        model._graphs.clear()
        for _, l, g in outs:
            assert torch.equal(l, l0) and torch.equal(g, g0), name
        res[name] = (st, l0, g0)
    assert "xout_tail" in res["lean"][0].dev and "xout_tail" not in res["flat"][0].dev
    assert torch.equal(res["lean"][1], res["flat"][1]) and torch.equal(res["lean"][2], res["flat"][2])
    assert abs(float(res["lean"][1][0]) - float(res["full"][1][0])) < 1e-5 * float(res["full"][1][0])
    assert R.rel_l2(res["lean"][2], res["full"][2]) < 5e-3


@pytest.fixture(scope="module")
def decode(mid):
    geo, gm = mid
    _, sd, cases = R.generate_cases()
    return geo, sd, cases, gm


def test_generate_on_the_fixture(decode):
    """token-exact on every bf16_stable case; decode graphs on and off give the same tokens on ALL cases"""
    geo, sd, cases, gm = decode
    gm.load_reference_state_dict(sd)
    assert gm.decode_graphs
    assert max(c["kw"]["num_beams"] * c["ids"].shape[0] for c in cases) <= 64          # (the row chunks: the test below)
    bad, differ, exact = [], [], 0
    for n, c in enumerate(cases):
        t, e = R.decode_case(gm, geo, c, graphs=True), R.decode_case(gm, geo, c, graphs=False)
        exact += int(same(t, c["tokens"]))
        if c["bf16_stable"] and not same(t, c["tokens"]):
            bad.append((n, c["kw"], t.tolist(), c["tokens"].tolist()))
        if not same(t, e):
            differ.append((n, c["kw"]))
    print(f"QWEN3 generate: {exact} of {len(cases)} cases token-exact, {sum(c['bf16_stable'] for c in cases)} stable")
    assert not bad, bad
    assert not differ, differ


def test_generate_penalty_and_sampled_case(decode):
    geo, sd, cases, gm = decode
    gm.load_reference_state_dict(sd)
    pen, smp = R.knob_cases(cases)
    for c in (pen, smp):
        t, e = R.decode_case(gm, geo, c, graphs=True), R.decode_case(gm, geo, c, graphs=False)
        assert same(t, c["tokens"]), (t.tolist(), c["tokens"].tolist())
        assert same(t, e)


def test_generate_more_than_64_beam_rows(decode):
    """5 utterances x 16 beams = 80 rows: the 64-row chunks of the decode GEMMs and of the append kernel's callers; the GPU's tokens
    against the double's beam by beam is not asked (near-ties), the property is the full-size test's: every returned hypothesis'
    beam score equals the log-softmax sum of a plain forward over prompt + tokens"""
    geo, sd, cases, gm = decode
    gm.load_reference_state_dict(sd)
    scores_equal_full_forward(gm, geo, B=5, nb=16, n_new=6, prompt=11, tol=0.02, floor=False)


def scores_equal_full_forward(m, geo, B, nb, n_new, prompt, tol, floor=True):
    from ps_slm_amd.decode import beam_search_generate
    batch = synthetic_text_batch(geo, B, seed=321, prompt_len=prompt, n_audio=21 if geo.llm_dim == 256 else 104, speech_pos=4, noise=False)
    ids = batch["input_ids"][:, :prompt]
    am = torch.ones_like(ids, dtype=torch.bool)
    st = m.prepare_text(ids, am, None, batch["post_ids"], None, None)
    m.forward_projector_text(st)
    out = beam_search_generate(m, st, num_beams=nb, max_new_tokens=n_new, eos_token_id=-1, pad_token_id=0)
    assert tuple(out.shape) == (B, n_new)
    beam_score = m._last_beam.fin_scores[:, 0].float().cpu() * n_new          # length_penalty 1.0: score = sum / length
    S = st.S
    ids2 = torch.cat([ids, out.to(ids.dtype)], dim=1)
    st2 = m.prepare_text(ids2, torch.ones_like(ids2, dtype=torch.bool), None, batch["post_ids"], None, None)
    m.forward_projector_text(st2)
    m.forward_llm(st2, compute_loss=False, need_backward=False)
    torch.cuda.synchronize()
    assert st2.S == S + n_new
    lp = torch.log_softmax(m.logits_view(st2)[:, S - 1:S - 1 + n_new].float(), dim=-1)
    tok_lp = lp.gather(2, out.cuda().long()[:, :, None])[:, :, 0].cpu()
    worst = float((tok_lp.sum(1) - beam_score).abs().max())
    print(f"QWEN3 decode scores vs full forward (B={B}, nb={nb}, D={geo.llm_dim}): worst {worst:.4f} of {tol * n_new:.3f}")
    if floor:
        assert float(tok_lp.min()) > -math.log(geo.llm_vocab) + 1.0         # the beams' tokens stand out of the uniform floor
    assert worst < tol * n_new, (tok_lp.sum(1), beam_score)


# ------------------------------------------------------------------------------------------------ synthetic:qwen3-1.7b
@pytest.fixture(scope="module")
def full():
    torch.cuda.empty_cache()
    m = factory("synthetic:qwen3-1.7b", 2048, keep_logits=True)
    assert (m.geo.llm_dim, m.geo.llm_layers, m.geo.llm_heads, m.geo.llm_kv_heads, m.geo.llm_inter) == (2048, 28, 16, 8, 6144)
    return m.geo, m


def test_full_size_decode_scores_equal_full_forward(full):
    """tolerance 0.02 nats per token, the 1.5B figure of tests/test_gpu_fullsize.py (two bf16 evaluations of a 28-layer decoder; a
    wrong cache row, position or head norm moves a chosen token's log-prob by nats)"""
    geo, m = full
    scores_equal_full_forward(m, geo, B=5, nb=4, n_new=7, prompt=25, tol=0.02)


def test_full_size_training_step(full):
    """a 4-utterance step: finite loss, bitwise repeatable, replay == eager"""
    geo, m = full
    batch = synthetic_text_batch(geo, 4, seed=5, noise=False)

    def one():
        st = m.prepare_text(batch["input_ids"], batch["attention_mask"], batch["labels"], batch["post_ids"], None, None)
        m.run_forward_text(st)
        m.run_backward(st)
        torch.cuda.synchronize()
        return st.dev["loss_out"].clone(), m.proj.g.clone()

    m.use_graphs = False
    l0, g0 = one()
    assert math.isfinite(float(l0[0])) and 5.0 < float(l0[0]) < 20.0 and bool(torch.isfinite(g0).all()) and float(g0.abs().max()) > 0
    l1, g1 = one()
    assert torch.equal(l1, l0) and torch.equal(g1, g0)
    m.use_graphs = True
    outs = [one() for _ in range(3)]                             # eager warm-up, capture + replay, replay
    m.use_graphs = False
    m._graphs.clear()
    for l, g in outs:
        assert torch.equal(l, l0) and torch.equal(g, g0)
