"""train_config.use_emb (use_peft=true: the LLM's input embedding table trains next to the projector and the adapters,
Multitask/model/ps-slm.py:119-123), host logic on the CPU test double: the REAL host code of ps_slm_amd/model.py + ps_slm.py +
engine.py driven through tests/fake_ops.py (which has no embed_bwd: the model's torch fallback runs), against goldens produced by
the real reference model (tools/make_golden_use_emb.py: tied head = lookup term + lm_head term, untied head = lookup term only)."""
import logging

import numpy as np
import pytest
import torch

from conftest import load_npz
from fake_ops import FakeOps
from ps_slm_amd.config import DEFAULT_DS_CONFIG, ModelConfig, TrainConfig, load_ds_config
from ps_slm_amd.engine import TasuEngine
from ps_slm_amd.lora import LoraConfig
from ps_slm_amd.model import Geometry, TasuModel
from ps_slm_amd.ps_slm import EMBED_KEY, model_factory
from ps_slm_amd.synthetic import MID_GEOMETRY, random_lora_state_dict, random_state_dict, synthetic_text_batch
from test_lora_cpu import check_against_golden, cosine, run_text, to_call

GOLDENS = ("mid_text_lora_emb", "mid_text_lora_emb_untied")


def golden_case(name):
    z = load_npz(name)
    geo = Geometry.from_dict(dict(MID_GEOMETRY, tied=bool(int(z["tied"]))))
    cfg = LoraConfig(r=int(z["r"]), lora_alpha=float(z["alpha"]), lora_dropout=float(z["p"]),
                     target_modules=tuple(str(z["targets"]).split(",")))
    sd = random_state_dict(geo, int(z["seed_w"]), with_encoder=False)
    lsd = random_lora_state_dict(geo, cfg, int(z["seed_l"]))
    batch = synthetic_text_batch(geo, 3, seed=int(z["seed_b"]), prompt_len=9, n_audio=21, target_len=17, speech_pos=4,
                                 feat_frames=12, noise=True, drop_prob=0.15, ragged=True)
    batch["post_ids"] = [list(np.asarray(p)[np.asarray(k, dtype=bool)]) for p, k in zip(batch["post_ids"], batch["keeps"])]
    del batch["alphas"], batch["keeps"]
    return z, geo, cfg, sd, lsd, batch


def build_emb(geo, cfg, sd, lsd, ops, device):
    m = TasuModel(geo, ops, device)
    m.load_reference_state_dict(sd)
    m.enable_lora(cfg)
    m.lora.load_state_dict(lsd)
    m.enable_embedding_training()
    return m


def check_table_gradient(g, z, cos_min=0.995, norm_tol=5e-2, show=None):
    """The bf16 bars check_against_golden applies to the adapters, on the table: the stored rows (every row the batch looks up +
    64 others), the L2 norm of EVERY row, and -- untied head -- exactly the golden's zero rows are zero."""
    g = g.float().cpu()
    rows = torch.from_numpy(z["egrad_rows"].astype(np.int64))
    ref = torch.from_numpy(z["egrad"].astype(np.float32)) / float(z["egrad_scale"])
    norms = torch.from_numpy(z["egrad_norms"].astype(np.float32))
    c, rn, cn = cosine(g[rows], ref), float(g[rows].norm() / ref.norm()), cosine(g.norm(dim=1), norms)
    if show:
        print(f"{show}: table gradient rows cosine {c:.6f} norm ratio {rn:.5f} row-norm cosine {cn:.6f}")
    assert c >= cos_min and abs(rn - 1.0) < norm_tol and cn >= cos_min
    if not int(z["tied"]):
        assert torch.equal(g.norm(dim=1) == 0, norms == 0)
        assert int((norms == 0).sum()) == 940


@pytest.mark.parametrize("name", GOLDENS)
def test_use_emb_step_vs_reference_golden(name):
    z, geo, cfg, sd, lsd, batch = golden_case(name)
    m = build_emb(geo, cfg, sd, lsd, FakeOps(), "cpu")
    st = run_text(m, batch)
    check_against_golden(m, st, z)                 # loss within 2e-2, logits, projector and adapter gradients: the table changes none
    check_table_gradient(m.embed_grad(), z, show=name)


@pytest.mark.parametrize("tied", [True, False])
def test_use_emb_bucket_layout_keys_and_roundtrip(tied):
    geo = Geometry.from_dict(dict(MID_GEOMETRY, tied=tied))
    V, D = geo.llm_vocab, geo.llm_dim
    model, eng = make_emb(tied=tied)
    core, pr, lp = model.core, model.core.proj, model.core.lora
    # [projector | adapters | table], the table's start aligned to 64 elements, nothing behind it
    lo, hi = core.embed_range
    assert lo == core.embed_base and lo % 64 == 0 and lo >= lp.base + lp.numel and lo - (lp.base + lp.numel) < 64
    assert hi == pr.numel == lo + V * D and all(t.numel() == pr.numel for t in (pr.p, pr.g, pr.m, pr.v, pr.pb))
    # llm.embed IS the bucket's range; tied: llm.head is the bf16 image's range; untied: its own frozen tensor
    assert core.llm.embed.data_ptr() == pr.p[lo:].data_ptr() and core.llm.embed.shape == (V, D)
    assert (core.llm.head.data_ptr() == pr.pb[lo:].data_ptr()) == tied
    with pytest.raises(RuntimeError):
        core.enable_embedding_training()
    # the ranges tile [0, numel) and the table's comes last
    for chunks in (1, 4):
        rs = core.grad_ranges(chunks)
        assert rs[-1] == (lp.base + lp.numel, hi)
        cover = sorted(rs)
        assert cover[0][0] == 0 and cover[-1][1] == pr.numel and all(a[1] == b[0] for a, b in zip(cover, cover[1:]))
    core.freeze_projector = True
    assert core.grad_ranges()[-1] == (lp.base + lp.numel, hi) and len(core.grad_ranges()) == len(core.lora_spans()) + 1
    core.freeze_projector = False
    # public surface: peft's key, [V, D] fp32, a leaf view of the master bucket
    named = dict(model.named_parameters())
    assert EMBED_KEY == "llm.base_model.model.model.embed_tokens.weight" and list(named)[-1] == EMBED_KEY
    assert len(named) == 6 + 2 * 7 * geo.llm_layers + 1 and sorted(named) == sorted(model.state_dict())
    p = named[EMBED_KEY]
    assert p.shape == (V, D) and p.dtype == torch.float32 and p.requires_grad and p.is_leaf and p.data_ptr() == core.llm.embed.data_ptr()
    # one step; loss.backward() hands the leaf its slice of the bucket
    raw = synthetic_text_batch(geo, 2, seed=5, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=8, noise=False)
    out, _ = model(**to_call(raw))
    out.loss.backward()
    assert torch.equal(p.grad, core.embed_grad()) and float(p.grad.abs().max()) > 0
    eng._last_state = None
    out, _ = eng(**to_call(raw))
    eng.backward(out.loss)
    eng.step()
    sd = model.state_dict()
    assert sd[EMBED_KEY].shape == (V, D) and torch.equal(sd[EMBED_KEY], core.llm.embed)
    # round trip into a fresh model: the eval loss is bit-equal; into a model built WITHOUT use_emb too (the table is a value)
    model.eval()
    want = float(model(**to_call(raw))[0].loss.detach())
    for use_emb in (True, False):
        m2, _ = make_emb(tied=tied, use_emb=use_emb)
        before = float(m2.eval()(**to_call(raw))[0].loss.detach())
        missing, unexpected = m2.load_state_dict(sd)
        assert not missing and not unexpected
        assert (EMBED_KEY in dict(m2.named_parameters())) == use_emb
        assert float(m2.eval()(**to_call(raw))[0].loss.detach()) == want != before
    m3, _ = make_emb(tied=tied)
    part = {k: v for k, v in sd.items() if k != EMBED_KEY}
    assert m3.load_state_dict(part)[0] == [EMBED_KEY]
    with pytest.raises(KeyError):
        m3.load_state_dict(part, strict=True)


def make_emb(tied=True, use_emb=True, lr=1e-3, ga=1, seed=1234, **tc_kw):
    tc = TrainConfig(freeze_llm=True, freeze_encoder=True, gt_emb=True, gt_emb_noise=False, ctc_posterior=True, do_psd=True,
                     use_peft=True, use_fp16=True, **tc_kw)
    tc.use_emb = use_emb
    tc.peft_config.r, tc.peft_config.lora_alpha, tc.peft_config.lora_dropout = 16, 32, 0.0
    mc = ModelConfig(llm_path="synthetic:mid" if tied else "synthetic:mid-untied", encoder_projector="linear-silu", llm_dim=256)
    model, _ = model_factory(tc, mc, device="cpu", ops=FakeOps(), init_seed=seed)
    cfg = load_ds_config(DEFAULT_DS_CONFIG)
    cfg["lr"] = lr
    cfg["gradient_accumulation_steps"] = ga
    eng = TasuEngine(model, cfg)
    eng.sched_iter = 10                      # past the zero-lr warm-up steps
    return model, eng


@pytest.mark.parametrize("tied", [True, False])
def test_use_emb_engine_step_moves_table_and_head(tied):
    model, eng = make_emb(tied=tied)
    core = model.core
    geo = core.geo
    V, D = geo.llm_vocab, geo.llm_dim
    raw = synthetic_text_batch(geo, 2, seed=5, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=8, noise=False)
    e0, h0, v0 = core.llm.embed.clone(), core.llm.head.clone(), core.embed_version
    out, _ = eng(**to_call(raw))
    eng.backward(out.loss)
    g = core.embed_grad()
    lr, wd = eng.get_lr()[0], eng.cfg["weight_decay"]
    assert lr > 1e-4 and wd == 0.0
    eng.step()
    moved = (core.llm.embed != e0).any(dim=1)
    assert core.embed_version > v0
    if tied:
        assert bool(moved.all())                                      # the lm_head term is dense
        assert torch.equal(core.llm.head, core.llm.embed.to(torch.bfloat16))
        assert torch.equal(core.llm.head_t[:, :V], core.llm.head.t()) and float(core.llm.head_t[:, V:].abs().max()) == 0.0
    else:
        assert torch.equal(moved, g.norm(dim=1) > 0) and 0 < int(moved.sum()) < 100      # weight decay is 0: only looked-up rows move
        assert torch.equal(core.llm.head, h0)                          # the untied lm_head stays frozen
    # the first AdamW step moves an element against the sign of its gradient, by at most lr (by lr where |g| >> eps)
    d, gs = (core.llm.embed - e0)[g.abs() > 1e-6], g[g.abs() > 1e-6]
    assert bool((torch.sign(d) == -torch.sign(gs)).all()) and float(d.abs().max()) <= lr * (1 + 1e-3)
    big = gs.abs() > 1e-3
    assert int(big.sum()) > 100 and torch.allclose(d[big], -lr * torch.sign(gs[big]), rtol=1e-2, atol=0)


def test_use_emb_gradient_accumulation_is_the_weighted_sum():
    model, eng = make_emb(ga=2)
    core = model.core
    raws = [synthetic_text_batch(core.geo, 2, seed=s, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=8, noise=False)
            for s in (5, 6)]
    grads, e0 = [], core.llm.embed.clone()
    for raw in raws:
        out, _ = eng(**to_call(raw))
        eng.backward(out.loss)
        grads.append(core.proj.g.clone())
        eng.step()
        if len(grads) == 1:
            assert torch.equal(core.llm.embed, e0)                    # no optimizer step between boundaries
            lo, hi = core.embed_range
            assert torch.equal(eng._g_acc[lo:hi], grads[0][lo:hi] / 4)
    assert eng._g_acc.numel() == core.proj.numel and float(eng._g_acc.abs().max()) == 0.0   # consumed and cleared
    assert not torch.equal(core.llm.embed, e0)
    # the same update from the 1/k^2-weighted sum in one AdamW step on a fresh model
    m2, e2 = make_emb(ga=1)
    m2.core.proj.g.copy_(grads[0] / 4 + grads[1] / 4)
    e2.step()
    assert torch.equal(m2.core.llm.embed, core.llm.embed)


def test_use_emb_factory_rules(caplog):
    mc = ModelConfig(llm_path="synthetic:mid", encoder_projector="linear-silu", llm_dim=256)
    base = dict(freeze_llm=True, freeze_encoder=True, gt_emb=True, ctc_posterior=True)
    # without use_peft the reference never looks at the knob: a warning, nothing extra trains
    tc = TrainConfig(use_peft=False, use_fp16=True, **base)
    tc.use_emb = True
    with caplog.at_level(logging.WARNING):
        model, _ = model_factory(tc, mc, device="cpu", ops=FakeOps())
    assert any("use_emb" in r.getMessage() and "use_peft" in r.getMessage() for r in caplog.records)
    assert model.core.embed_base is None and len(dict(model.named_parameters())) == 6 and EMBED_KEY not in model.state_dict()
    # fp32 everywhere has no backward into the table
    tc = TrainConfig(use_peft=True, use_fp16=False, mixed_precision=False, **base)
    tc.use_emb = True
    with pytest.raises(NotImplementedError, match="use_emb"):
        model_factory(tc, mc, device="cpu", ops=FakeOps())
    # quantization keeps raising
    tc = TrainConfig(use_peft=True, use_fp16=True, **base)
    tc.quantization = True
    with pytest.raises(NotImplementedError, match="quantization"):
        model_factory(tc, mc, device="cpu", ops=FakeOps())


@pytest.mark.parametrize("tied", [True, False])
def test_use_emb_backward_with_exchange_hook_reports_the_table_last(tied):
    """The path the engine takes when gradients are exchanged (run_backward with on_ready): the ranges are reported in the
    order of grad_ranges(), the table's last, and the bucket equals the hook-less backward's."""
    model, _ = make_emb(tied=tied)
    core = model.core
    raw = synthetic_text_batch(core.geo, 2, seed=5, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=8, noise=False)
    grads = []
    for hook in (False, True):
        model(**to_call(raw))
        seen = []
        core.proj.g.fill_(7.0)
        core.run_backward(model.last_state, on_ready=(lambda lo, hi: seen.append((lo, hi))) if hook else None, w1_chunks=4 if hook else 1)
        grads.append(core.proj.g.clone())
        if hook:
            assert seen == core.grad_ranges(4) and seen[-1][1] == core.proj.numel and seen[-1][0] <= core.embed_base
    assert torch.equal(grads[0], grads[1]) and float((grads[0] == 7.0).float().mean()) < 1e-3


def audio_case(tied):
    """The audio-branch fixture (encoder -> CTC posterior -> PSD -> projector -> LLM) with adapters and a trainable table."""
    import dataclasses
    from conftest import mid_audio_psd_case
    geo, sd, batch, z = mid_audio_psd_case()
    geo = dataclasses.replace(geo, tied=tied)
    if not tied:
        sd = dict(sd)
        sd["llm.lm_head.weight"] = torch.randn(geo.llm_vocab, geo.llm_dim, generator=torch.Generator().manual_seed(77)) * 0.05
    cfg = LoraConfig(r=16, lora_alpha=32, lora_dropout=0.0)
    return geo, cfg, sd, random_lora_state_dict(geo, cfg, 3), batch, z


def run_audio(m, batch):
    st = m.prepare_audio(batch["input_ids"], batch["attention_mask"], batch["labels"], batch["input_features"], batch["input_feature_length"])
    m.forward_llm(st)
    m.backward(st)
    return st


@pytest.mark.parametrize("tied", [True, False])
def test_use_emb_on_the_audio_branch(tied):
    """The audio branch shares the merge plan with the text branch: the table's gradient is the sum of the dx rows of the TEXT
    positions per token id (+ dlogits^T h, tied), recomputed here in float64 from the step's own dx; the rows the merge filled with
    audio (the <speech> placeholder) and ids the batch never looks up get nothing from the lookup term -- exact zeros, untied."""
    geo, cfg, sd, lsd, batch, z = audio_case(tied)
    m = build_emb(geo, cfg, sd, lsd, FakeOps(), "cpu")
    st = run_audio(m, batch)
    assert st.path == "audio" and np.array_equal(st.dev["psd_lens"], z["psd_lens"])
    g, d = m.embed_grad().double(), st.dev
    kind, idx = torch.from_numpy(st.plan.src_kind).long(), torch.from_numpy(st.plan.src_idx).long()
    text = torch.nonzero(kind == 1)[:, 0]
    assert int((kind == 2).sum()) > 0 and geo.speech_id not in idx[text].tolist()
    want = torch.zeros(geo.llm_vocab, geo.llm_dim, dtype=torch.float64)
    want.index_add_(0, idx[text], d["dx"][text].double())
    looked = want.norm(dim=1) > 0
    if tied:
        n = st.M
        want += d["dlogits"][:n, : geo.llm_vocab].double().t() @ d["xn_head"][:n].double()
    else:
        assert torch.equal(g.norm(dim=1) > 0, looked) and float(g[geo.speech_id].abs().max()) == 0.0
    assert 0 < int(looked.sum()) < 100
    assert float((g - want).abs().max()) <= 1e-5 * float(want.abs().max())
