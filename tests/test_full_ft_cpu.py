"""Full fine-tuning of the LLM (train_config.freeze_llm=false without use_peft, Multitask/model/ps-slm.py:105-108), host logic on
the CPU test double: the REAL host code of ps_slm_amd/full_ft.py + model.py + ps_slm.py + engine.py driven through
tests/full_ft_ops.py (FakeOps + the weight-gradient operators), against goldens produced by the real reference model with every
LLM parameter trainable (tools/make_golden_full_ft.py)."""
import logging
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import free_port
from full_ft_ops import GOLDENS, FullFtFakeOps, build_ft, golden_case, llm_grads, stored
from ps_slm_amd.config import DEFAULT_DS_CONFIG, ModelConfig, TrainConfig, load_ds_config
from ps_slm_amd.engine import TasuEngine
from ps_slm_amd.full_ft import EMBED_KEY, HEAD_KEY, NORM_KEY
from ps_slm_amd.ps_slm import model_factory
from ps_slm_amd.synthetic import synthetic_text_batch
from test_lora_cpu import cosine, run_text, to_call


def check_step_against_golden(m, st, z, cos_min=0.995, norm_tol=5e-2, show=None):
    """The project's bf16 bars (test_lora_cpu.check_against_golden): |loss - ref| < 2e-2, logits within 3 % of the range, projector
    gradients cosine > 0.995 -- and EVERY tensor of the decoder on the fixture's sub-grid: cosine > 0.995, full-tensor norm within
    5 %.  No tensor is skipped; the smallest ones (the q / k biases, below 2 % of the largest norm) clear the same bar."""
    res = st.dev["loss_out"].cpu()
    assert abs(float(res[0]) - float(z["loss"])) < 2e-2
    valid = torch.from_numpy(st.plan.key_mask[:, : st.S].astype(bool))
    cols = torch.from_numpy(z["cols"])
    lg = m.logits_view(st).float().cpu()
    ref = torch.from_numpy(z["logits_cols"])
    assert float((lg[:, :, cols] - ref)[valid].abs().max() / ref[valid].abs().max()) < 3e-2
    n = 0
    for k, g in m.projector_grads().items():
        short = "grad." + k[len("encoder_projector."):]
        if short in z:
            assert cosine(g, torch.from_numpy(z[short])) > cos_min, k
            n += 1
    assert n == 5
    gs = llm_grads(m)
    want = sorted(k[len("g."):] for k in z if k.startswith("g."))
    assert sorted(gs) == want and len(want) == 12 * m.geo.llm_layers + 2 + (0 if m.geo.tied else 1)
    worst = (2.0, None)
    for k, g in gs.items():
        sub, ref = stored(g, z, k)
        c, rn = cosine(sub, ref), float(g.float().norm()) / float(z["gnorm." + k])
        worst = min(worst, (c, k))
        assert c > cos_min and abs(rn - 1.0) < norm_tol, (k, c, rn)
    if show:
        print(f"{show}: loss {float(res[0]):.6f} (reference {float(z['loss']):.6f}); lowest gradient cosine {worst[0]:.6f} at {worst[1]}")


@pytest.mark.parametrize("name", GOLDENS)
def test_full_ft_step_vs_reference_golden(name):
    z, geo, sd, batch = golden_case(name)
    m = build_ft(geo, sd, FullFtFakeOps(), "cpu")
    st = run_text(m, batch)
    check_step_against_golden(m, st, z, show=name)


@pytest.mark.parametrize("name", GOLDENS)
def test_both_weight_gradient_routes_and_the_compact_loss_head_agree(name):
    """tasu_gemm_tn_bf16 and the composed route (two transposes + the NT GEMM) are the same sums; the throughput form of the loss
    head (labelled rows only, keep_logits=False: the final norm's weight gradient then takes the row-compacted form) gives the
    same gradients.  The compact last-layer tail is switched off in this mode."""
    z, geo, sd, batch = golden_case(name)
    runs = []
    for split, keep in ((1, True), (99, True), (1, False)):
        m = build_ft(geo, sd, FullFtFakeOps(), "cpu")
        m.full_ft.tn_min_split, m.keep_logits = split, keep
        st = run_text(m, batch)
        assert "xout_tail" not in st.dev and bool(st.dev.get("labelled_only", False)) == (not keep)
        runs.append((float(st.dev["loss_out"][0]), m.proj.g.clone()))
    for loss, g in runs[1:]:
        assert loss == pytest.approx(runs[0][0], rel=1e-6)
        assert torch.allclose(g, runs[0][1], rtol=1e-4, atol=1e-6 * float(runs[0][1].abs().max()))


def make_ft(tied=True, lr=1e-3, ga=1, seed=1234, freeze_llm=False, **tc_kw):
    tc_kw.setdefault("use_fp16", True)
    tc = TrainConfig(freeze_llm=freeze_llm, freeze_encoder=True, gt_emb=True, gt_emb_noise=False, ctc_posterior=True, do_psd=True, **tc_kw)
    mc = ModelConfig(llm_path="synthetic:mid" if tied else "synthetic:mid-untied", encoder_projector="linear-silu", llm_dim=256)
    model, _ = model_factory(tc, mc, device="cpu", ops=FullFtFakeOps(), init_seed=seed)
    cfg = load_ds_config(DEFAULT_DS_CONFIG)
    cfg["lr"] = lr
    cfg["gradient_accumulation_steps"] = ga
    eng = TasuEngine(model, cfg)
    eng.sched_iter = 10                      # past the zero-lr warm-up steps
    return model, eng


def hf_names_and_shapes(geo):
    """named_parameters() of transformers' Qwen2ForCausalLM at this geometry (built on the meta device: names and shapes only)."""
    from transformers import Qwen2Config, Qwen2ForCausalLM
    cfg = Qwen2Config(vocab_size=geo.llm_vocab, hidden_size=geo.llm_dim, intermediate_size=geo.llm_inter, num_hidden_layers=geo.llm_layers,
                      num_attention_heads=geo.llm_heads, num_key_value_heads=geo.llm_kv_heads, tie_word_embeddings=geo.tied)
    with torch.device("meta"):
        hf = Qwen2ForCausalLM(cfg)
    return {"llm." + n: tuple(p.shape) for n, p in hf.named_parameters()}


@pytest.mark.parametrize("tied", [True, False])
def test_full_ft_names_layout_and_ranges(tied):
    model, eng = make_ft(tied=tied)
    core, pr, ft = model.core, model.core.proj, model.core.full_ft
    geo = core.geo
    named = dict(model.named_parameters())
    llm_named = {k: v for k, v in named.items() if k.startswith("llm.")}
    want = hf_names_and_shapes(geo)
    assert {k: tuple(v.shape) for k, v in llm_named.items()} == want
    assert len(named) == 6 + len(want) and sorted(named) == sorted(model.state_dict())
    assert (HEAD_KEY in named) == (not tied) and EMBED_KEY in named and NORM_KEY in named
    # every leaf is a view of the fp32 master bucket; the kernels' tensors are views of the bucket too (bf16 image / masters)
    lo_b, hi_b = pr.p.data_ptr(), pr.p.data_ptr() + 4 * pr.numel
    for k, p in named.items():
        assert p.is_leaf and p.requires_grad and p.dtype == torch.float32 and lo_b <= p.data_ptr() < hi_b, k
        assert not k.startswith("llm.") or (p.is_contiguous() and p.data_ptr() + 4 * p.numel() <= hi_b), k
    w = core.llm.layers[1]
    assert w["wqkv"].data_ptr() == ft.view(pr.pb, "wqkv", 1).data_ptr() and w["ln1"].data_ptr() == ft.view(pr.p, "ln1", 1).data_ptr()
    assert core.llm.embed.data_ptr() == core.embed_view(pr.p).data_ptr() and core.llm.norm.data_ptr() == ft.view(pr.p, "norm").data_ptr()
    assert core.llm.head.data_ptr() == (core.embed_view(pr.pb) if tied else ft.view(pr.pb, "head")).data_ptr()
    assert sum(p.numel() for p in llm_named.values()) == sum(int(np.prod(s)) for s in want.values())
    # the ranges tile the bucket exactly, the decoder's in completion order (last layer first), the table's last
    for chunks in (1, 4):
        rs = core.grad_ranges(chunks)
        cover = sorted(rs)
        assert cover[0][0] == 0 and cover[-1][1] == pr.numel and all(a[1] == b[0] for a, b in zip(cover, cover[1:]))
        assert rs[0][0] == ft.lo and rs[1] == ft.layer_range[geo.llm_layers - 1] and rs[-1][1] == pr.numel and rs[-1][0] == ft.end
    # the exchange hook sees exactly these ranges and the bucket equals the hook-less backward's
    raw = synthetic_text_batch(geo, 2, seed=5, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=8, noise=False)
    grads = []
    for hook in (False, True):
        model(**to_call(raw))
        seen = []
        pr.g.fill_(7.0)
        core.run_backward(model.last_state, on_ready=(lambda lo, hi: seen.append((lo, hi))) if hook else None, w1_chunks=4 if hook else 1)
        grads.append(pr.g.clone())
        assert not hook or seen == core.grad_ranges(4)
    assert torch.equal(grads[0], grads[1])
    # every element of the bucket that belongs to a tensor was written; the alignment gaps were not
    touched = torch.zeros(pr.numel, dtype=torch.bool)
    for _, v, _t in model._views(torch.arange(pr.numel)):
        touched[v.flatten()] = True
    assert bool((grads[0][touched] != 7.0).float().mean() > 0.999)


@pytest.mark.parametrize("tied", [True, False])
def test_full_ft_engine_step_equals_torch_adamw_and_autograd_route(tied):
    """One TasuEngine step = torch.optim.AdamW over model.parameters() on the same gradients (loss.backward() through _HipStep), to
    the existing engine test's tolerance; afterwards the kernels' copies follow the masters.  The key biases are the exception in
    the second step: their gradient is pure cancellation (a softmax does not see a constant added to every key's score; median
    5e-6 here), so masters that differ in the last place after the first step -- two AdamW formulations -- give the two sides
    different noise there (single elements moved by 1 %), and Adam normalises noise to full-size steps.  All that can be said of
    such an element is that each side moved it by at most one step: with two gradients in the moments |m^| / sqrt(v^) <=
    sqrt(w1^2 / a1 + w2^2 / a2) = 1.0014 (Cauchy-Schwarz; w = (b1 c1, c1) / bc1, a = (b2 c2, c2) / bc2), so the two differ by at
    most 2.003 lr.  Every other parameter keeps the two-step comparison at the old tolerance."""
    model, _ = make_ft(tied=tied, seed=77)
    twin, eng = make_ft(tied=tied, seed=77)
    geo = model.core.geo
    params = list(filter(lambda p: p.requires_grad, model.parameters()))
    c = eng.cfg
    opt = torch.optim.AdamW(params, lr=c["lr"], betas=tuple(c["betas"]), eps=c["eps"], weight_decay=c["weight_decay"])
    for step in range(2):
        raw = synthetic_text_batch(geo, 2, seed=30 + step, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=8, noise=False)
        out_e, _ = eng(**to_call(raw))
        lr = eng.get_lr()[0]
        eng.backward(out_e.loss)
        eng.step()
        for g in opt.param_groups:
            g["lr"] = lr
        out, _ = model(**to_call(raw))
        assert float(out.loss.detach()) == pytest.approx(float(out_e.loss.detach()), rel=1e-5)
        opt.zero_grad()
        out.loss.backward()
        for (n, p), (_, gv) in zip(model.named_parameters(), model._trainable_views(model.core.proj.g)):
            assert torch.allclose(p.grad, gv, rtol=1e-6, atol=0), n
        opt.step()
        sd, sd_e = model.state_dict(), twin.state_dict()
        for k in sd:
            noise = step > 0 and k.endswith("self_attn.k_proj.bias")
            assert torch.allclose(sd[k], sd_e[k], rtol=2e-5, atol=2.003 * lr if noise else 2e-7), (step, k)
    core, llm = twin.core, twin.core.llm
    w = llm.layers[0]
    V = geo.llm_vocab
    for n in ("wqkv", "wo", "wgu", "wd"):
        assert torch.equal(w[n], core.full_ft.view(core.proj.p, n, 0).to(torch.bfloat16)) and torch.equal(w[n + "_t"], w[n].t())
    assert torch.equal(llm.head_t[:, :V], llm.head.t()) and torch.equal(llm.head, (llm.embed if tied else core.full_ft.view(core.proj.p, "head")).to(torch.bfloat16))


@pytest.mark.parametrize("tied", [True, False])
def test_full_ft_checkpoint_roundtrip_into_trainable_and_frozen_models(tied):
    model, eng = make_ft(tied=tied, lr=2e-2)
    geo = model.core.geo
    raw = synthetic_text_batch(geo, 2, seed=5, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=8, noise=False)
    out, _ = eng(**to_call(raw))
    eng.backward(out.loss)
    eng.step()
    sd = model.state_dict()
    assert all(v.dtype == torch.float32 for v in sd.values())
    want = float(model.eval()(**to_call(raw))[0].loss.detach())
    for frozen in (False, True):
        m2, _ = make_ft(tied=tied, freeze_llm=frozen)
        before = float(m2.eval()(**to_call(raw))[0].loss.detach())
        missing, unexpected = m2.load_state_dict(dict(sd, **({HEAD_KEY: sd[EMBED_KEY]} if tied else {})))   # tied: a lm_head key is ignored
        assert not missing and not unexpected
        assert (m2.core.full_ft is None) == frozen and len(dict(m2.named_parameters())) == (6 if frozen else len(sd))
        assert float(m2.eval()(**to_call(raw))[0].loss.detach()) == want != before
    m3, _ = make_ft(tied=tied)
    part = {k: v for k, v in sd.items() if k != NORM_KEY}
    assert m3.load_state_dict(part)[0] == [NORM_KEY]
    with pytest.raises(KeyError):
        make_ft(tied=tied, freeze_llm=True)[0].load_state_dict(part)             # a frozen model needs the whole decoder


def test_full_ft_with_a_frozen_projector_trains_the_llm_alone():
    model, eng = make_ft(freeze_projector=True)
    core, pr = model.core, model.core.proj
    assert core.freeze_projector and core.trainable_lo == core.full_ft.lo
    assert not any(k.startswith("encoder_projector.") for k in model.state_dict())
    assert all(k.startswith("llm.") for k, p in model.named_parameters() if p.requires_grad)
    lo = core.full_ft.lo
    pr.g[:lo].fill_(3.0)                                                          # would move the projector if anything read it
    p0, pb0 = pr.p.clone(), pr.pb.clone()
    raw = synthetic_text_batch(core.geo, 2, seed=5, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=8, noise=False)
    out, _ = eng(**to_call(raw))
    eng.backward(out.loss)
    assert bool((pr.g[:lo] == 3.0).all())
    eng.step()
    assert torch.equal(pr.p[:lo], p0[:lo]) and torch.equal(pr.pb[:lo], pb0[:lo]) and torch.equal(pr.m[:lo], torch.zeros(lo))   # bitwise
    assert float((pr.p[lo:] != p0[lo:]).float().mean()) > 0.9
    cover = sorted(core.grad_ranges())
    assert cover[0][0] == lo and cover[-1][1] == pr.numel and all(a[1] == b[0] for a, b in zip(cover, cover[1:]))


def test_full_ft_gradient_accumulation_is_the_weighted_sum():
    model, eng = make_ft(ga=2)
    core = model.core
    raws = [synthetic_text_batch(core.geo, 2, seed=s, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=8, noise=False)
            for s in (5, 6)]
    grads, p0 = [], core.proj.p.clone()
    for raw in raws:
        out, _ = eng(**to_call(raw))
        eng.backward(out.loss)
        grads.append(core.proj.g.clone())
        eng.step()
        if len(grads) == 1:
            assert torch.equal(core.proj.p, p0)
    m2, e2 = make_ft(ga=1)
    m2.core.proj.g.copy_(grads[0] / 4 + grads[1] / 4)
    e2.step()
    assert torch.equal(m2.core.proj.p, core.proj.p) and not torch.equal(core.proj.p, p0)


def test_full_ft_factory_rules(caplog):
    mc = ModelConfig(llm_path="synthetic:mid", encoder_projector="linear-silu", llm_dim=256)
    base = dict(freeze_encoder=True, gt_emb=True, ctc_posterior=True)
    ops = FullFtFakeOps()
    # the fp32 training step has no decoder weight gradients: use_fp16=false, hence the dataclass defaults, are refused by name
    for kw in (dict(use_fp16=False), dict(use_fp16=False, mixed_precision=False), {}):
        with pytest.raises(NotImplementedError, match="freeze_llm") as e:
            model_factory(TrainConfig(freeze_llm=False, **base, **kw), mc, device="cpu", ops=ops)
        assert "use_fp16=true" in str(e.value)
    # use_peft=true: peft freezes the base weights -- a warning, and exactly what freeze_llm=true builds (use_emb as now)
    for use_emb in (False, True):
        models = []
        for freeze in (False, True):
            tc = TrainConfig(freeze_llm=freeze, use_peft=True, use_fp16=True, **base)
            tc.use_emb = use_emb
            tc.peft_config.r, tc.peft_config.lora_dropout = 16, 0.0
            caplog.clear()
            with caplog.at_level(logging.WARNING):
                models.append(model_factory(tc, mc, device="cpu", ops=ops)[0])
            assert any("freeze_llm" in r.getMessage() and "peft" in r.getMessage() for r in caplog.records) == (not freeze)
        a, b = models
        assert a.core.full_ft is None and a.core.lora is not None and (a.core.embed_base is not None) == use_emb
        assert list(dict(a.named_parameters())) == list(dict(b.named_parameters())) and torch.equal(a.core.proj.p, b.core.proj.p)
    # use_emb without use_peft keeps its warning and changes nothing: the table trains anyway, under the decoder's own name
    tc = TrainConfig(freeze_llm=False, use_fp16=True, **base)
    tc.use_emb = True
    with caplog.at_level(logging.WARNING):
        m = model_factory(tc, mc, device="cpu", ops=ops)[0]
    assert any("use_emb" in r.getMessage() and "use_peft" in r.getMessage() for r in caplog.records)
    assert m.core.full_ft is not None and EMBED_KEY in dict(m.named_parameters())
    # freeze_projector=true now leaves the LLM to train; with a frozen LLM it still leaves nothing
    assert model_factory(TrainConfig(freeze_llm=False, use_fp16=True, freeze_projector=True, **base), mc, device="cpu", ops=ops)[0].core.freeze_projector
    with pytest.raises(ValueError, match="nothing to train"):
        model_factory(TrainConfig(freeze_llm=True, use_fp16=True, freeze_projector=True, **base), mc, device="cpu", ops=ops)
    # the operator set must have the kernels: no quiet fall-back
    from fake_ops import FakeOps
    m = model_factory(TrainConfig(freeze_llm=False, use_fp16=True, **base), mc, device="cpu", ops=FakeOps())[0]
    raw = synthetic_text_batch(m.core.geo, 2, seed=5, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=8, noise=False)
    out, _ = m(**to_call(raw))
    with pytest.raises(AttributeError):
        out.loss.backward()


def _dp_worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    model, eng = make_ft()
    core = model.core
    full = synthetic_text_batch(core.geo, 4, seed=100, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=8, noise=False)
    call = to_call(full)
    mine = {k: v[2 * rank: 2 * rank + 2] for k, v in call.items()}                  # this rank's half of the batch
    out, _ = eng(**mine)
    eng.exchange = False
    eng.backward(out.loss)
    g_local = core.proj.g.clone()
    eng.exchange, eng.micro_steps = True, 0
    out, _ = eng(**mine)
    eng.backward(out.loss)
    assert [(lo, hi) for lo, hi, _ in eng._pending] == core.grad_ranges(eng.w1_chunks)
    assert sum(hi - lo for lo, hi, _ in eng._pending) == core.proj.numel           # the ranges tile the bucket
    eng.step()
    ret[rank] = dict(loss=float(out.loss.detach()), grad=g_local, param=core.proj.p.clone())
    dist.destroy_process_group()


def test_full_ft_data_parallel_two_ranks_gloo():
    """Two ranks, each on its half of a batch: replicas stay equal, the update is ONE AdamW step on the ranks' averaged gradient,
    and that average is the single-rank gradient of the concatenated batch (equal label counts: the mean CE of the whole batch is
    the mean of the halves') up to fp32 summation order."""
    world, port = 2, free_port()
    ret = mp.Manager().dict()
    mp.spawn(_dp_worker, args=(world, port, ret), nprocs=world, join=True)
    r0, r1 = ret[0], ret[1]
    assert torch.equal(r0["param"], r1["param"]), "replicas diverged"
    model, eng = make_ft()
    model.core.proj.g.copy_(r0["grad"] + r1["grad"])
    eng.world = 2
    eng.step()
    torch.testing.assert_close(model.core.proj.p, r0["param"], rtol=1e-6, atol=1e-7)
    single, e1 = make_ft()
    full = synthetic_text_batch(single.core.geo, 4, seed=100, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=8, noise=False)
    out, _ = e1(**to_call(full))
    e1.backward(out.loss)
    assert float(out.loss.detach()) == pytest.approx((r0["loss"] + r1["loss"]) / 2, rel=1e-5)
    g, avg = single.core.proj.g, (r0["grad"] + r1["grad"]) / 2
    assert torch.allclose(g, avg, rtol=1e-3, atol=1e-5 * float(avg.abs().max()))
