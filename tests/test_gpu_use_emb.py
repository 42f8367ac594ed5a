"""train_config.use_emb on the GPU: tasu_embed_bwd (the lookup term of the embedding table's gradient) against a float64
index_add_, the step on the HIP kernels against the reference goldens (tools/make_golden_use_emb.py) and the CPU double, eager
against hipGraph replay, and -- after an engine step -- everything that caches the table (bf16 and fp32 decode, the fp32 eval
forward, the cross-attention projector's tables) against a fresh model loaded from the stepped model's state_dict()."""
import numpy as np
import pytest
import torch

from fake_ops import FakeOps
from test_lora_cpu import check_against_golden, cosine, run_text, to_call
from test_use_emb_cpu import GOLDENS, build_emb, check_table_gradient, golden_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from ps_slm_amd.ops import HipOps
    return HipOps()


# ------------------------------------------------------------------------------------------ 5. the kernel
def _segments(ids_per_row):
    """The host plan of TasuModel._embed_plan for a list of per-row ids (id < 0: a row nothing looks up)."""
    ids = np.asarray(ids_per_row, dtype=np.int64)
    text = np.nonzero(ids >= 0)[0]
    order = np.argsort(ids[text], kind="stable")
    uniq, first = np.unique(ids[text][order], return_index=True)
    return text[order].astype(np.int32), uniq.astype(np.int32), first.astype(np.int32)


def _patterns(n, V, g):
    r = lambda hi, k: torch.randint(0, hi, (k,), generator=g).numpy()
    out = {"distinct": torch.randperm(V, generator=g)[:n].numpy(), "same": np.full(n, int(r(V, 1)[0]))}
    rep = torch.randperm(V, generator=g)[:n].numpy()
    rep[r(n, 12)] = rep[0]                                               # one id (up to) 12 times
    out["repeat12"] = rep
    ends = torch.randperm(V, generator=g)[:n].numpy()
    ends[0], ends[-1] = V - 1, 0                                         # the table's first and last row
    out["ends"] = ends
    holes = rep.copy()
    holes[::3] = -1                                                      # skipped rows interleaved
    if n > 1:
        out["holes"] = holes
    return out


@pytest.mark.parametrize("D", [256, 1536])
@pytest.mark.parametrize("n", [1, 77, 300])
def test_embed_bwd_against_float64_index_add(ops, D, n):
    V = 1000
    g = torch.Generator().manual_seed(100 * n + D)
    for name, ids in _patterns(n, V, g).items():
        dx = torch.randn(n, D, generator=g)
        dst0 = torch.randn(V, D, generator=g)                            # pre-filled: the kernel adds
        rows, seg_id, first = _segments(ids)
        n_text, n_real = len(rows), len(seg_id)
        # the three layouts the model uploads: rows padded with -1, segment ids with -1, starts with the number of text rows
        pad = 5
        rows_p = np.concatenate([rows, np.full(n + pad - n_text, -1, np.int32)])
        seg_id_p = np.concatenate([seg_id, np.full(n + pad - n_real, -1, np.int32)])
        start_p = np.concatenate([first, np.full(n + pad + 1 - n_real, n_text, np.int32)])
        if name == "holes":                                              # a skipped SEGMENT in the middle, and a skipped row inside a segment
            seg_id_p[1 % n_real] = -1 if n_real > 1 else seg_id_p[0]
            rows_p[0] = -1
        d = lambda a: torch.from_numpy(a).cuda()
        outs = []
        for _ in range(2):
            dst = dst0.cuda()
            ops.embed_bwd(dx.cuda(), d(rows_p), d(start_p), d(seg_id_p), dst, len(rows_p), len(seg_id_p))
            torch.cuda.synchronize()
            outs.append(dst.cpu())
        assert torch.equal(outs[0], outs[1]), name                       # no atomics: the same bits on every run
        # float64 reference + the fp32 summation bound per element: (segment length + 1) * 2^-24 * sum |terms|
        ref, mag = dst0.double().clone(), dst0.double().abs().clone()
        cnt = torch.ones(V, dtype=torch.float64)
        touched = torch.zeros(V, dtype=torch.bool)
        for s in range(len(seg_id_p)):
            if seg_id_p[s] < 0:
                continue
            touched[seg_id_p[s]] = True
            for j in range(start_p[s], start_p[s + 1]):
                if rows_p[j] >= 0:
                    ref[seg_id_p[s]] += dx[rows_p[j]].double()
                    mag[seg_id_p[s]] += dx[rows_p[j]].double().abs()
                    cnt[seg_id_p[s]] += 1
        err = (outs[0].double() - ref).abs()
        bound = cnt[:, None] * 2.0 ** -24 * mag
        assert bool((err <= bound).all()), (name, float((err / bound).max()))
        assert torch.equal(outs[0][~touched], dst0[~touched]), name      # rows no id names: untouched, bitwise
        assert int(touched.sum()) >= 1 and not torch.equal(outs[0][touched], dst0[touched])


def test_embed_bwd_rejects_bad_arguments(ops):
    lib = ops.lib
    assert lib.tasu_embed_bwd(None, None, None, None, None, 4, 4, 4, 10, 256, None) == 1
    t = torch.zeros(8, 256, device="cuda")
    i = torch.zeros(9, dtype=torch.int32, device="cuda")
    p = lambda x: x.data_ptr()
    assert lib.tasu_embed_bwd(p(t), p(i), p(i), p(i), p(t), 8, 8, 8, 8, 254, None) == 1        # D % 4
    assert lib.tasu_embed_bwd(p(t), p(i), p(i), p(i), p(t), 8, 0, 8, 8, 256, None) == 1
    assert lib.tasu_embed_bwd(p(t), p(i), p(i), p(i), p(t) + 4, 8, 8, 8, 8, 256, None) == 1    # 16-byte alignment


# ------------------------------------------------------------------------------------------ 6. the step
@pytest.fixture(scope="module")
def double_runs():
    """The CPU double's step on both golden cases, computed once."""
    out = {}
    for name in GOLDENS:
        z, geo, cfg, sd, lsd, batch = golden_case(name)
        cm = build_emb(geo, cfg, sd, lsd, FakeOps(), "cpu")
        sc = run_text(cm, batch)
        out[name] = (float(sc.dev["loss_out"][0]), cm.embed_grad(), cm.lora_grads(), cm.projector_grads())
    return out


@pytest.mark.parametrize("name", GOLDENS)
def test_use_emb_step_hip_vs_reference_golden_and_double(ops, double_runs, name):
    z, geo, cfg, sd, lsd, batch = golden_case(name)
    gm = build_emb(geo, cfg, sd, lsd, ops, "cuda")
    sg = run_text(gm, batch)
    torch.cuda.synchronize()
    check_against_golden(gm, sg, z)
    check_table_gradient(gm.embed_grad(), z, show=name + " (HIP)")
    loss_c, eg_c, lg_c, pg_c = double_runs[name]
    eg = gm.embed_grad().cpu()
    c, rel = cosine(eg, eg_c), float((eg - eg_c).norm() / eg_c.norm())
    print(f"{name}: HIP vs double: loss diff {abs(float(sg.dev['loss_out'][0]) - loss_c):.2e} table cosine {c:.6f} relative error {rel:.2e}")
    assert abs(float(sg.dev["loss_out"][0]) - loss_c) < 2e-3
    assert c > 0.9995 and rel < 3e-2
    assert torch.equal(eg.norm(dim=1) == 0, eg_c.norm(dim=1) == 0)
    for k, g2 in lg_c.items():
        g1 = gm.lora_grads()[k].cpu()
        assert cosine(g1, g2) > 0.9995 and float((g1 - g2).norm() / g2.norm()) < 3e-2, k
    for k, g2 in pg_c.items():
        assert cosine(gm.projector_grads()[k], g2) > 0.9995, k


@pytest.mark.parametrize("with_lora", [True, False])
@pytest.mark.parametrize("name", GOLDENS)
def test_use_emb_graph_replay_equals_eager_on_another_batch(ops, name, with_lora):
    """Eager launches against hipGraph replay (first call of a shape eager, second captured, third replayed); the replay runs
    on a DIFFERENT batch of the same shape, so the uploaded plan arrays -- not anything baked in at capture -- must decide which
    rows of the table receive what.  With adapters the forward is the graph and the adapted backward is launched eagerly (the
    product's choice: TasuModel.run_backward); a model whose table trains without adapters replays the whole backward -- the head
    weight gradient and tasu_embed_bwd included -- as one graph."""
    from ps_slm_amd.model import TasuModel
    from ps_slm_amd.synthetic import synthetic_text_batch
    z, geo, cfg, sd, lsd, _ = golden_case(name)
    if with_lora:
        gm = build_emb(geo, cfg, sd, lsd, ops, "cuda")
    else:
        gm = TasuModel(geo, ops, "cuda")
        gm.load_reference_state_dict(sd)
        gm.enable_embedding_training()
    gm.keep_logits = False                                              # the throughput mode: the labelled rows only
    mk = lambda seed: synthetic_text_batch(geo, 3, seed=seed, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=12, noise=False)
    b1, b2 = mk(41), mk(42)
    assert not torch.equal(b1["input_ids"], b2["input_ids"]) and b1["input_ids"].shape == b2["input_ids"].shape

    def step(batch, graphs):
        gm.use_graphs = graphs
        st = gm.prepare_text(batch["input_ids"], batch["attention_mask"], batch["labels"], batch["post_ids"])
        gm.run_forward_text(st)
        gm.run_backward(st)
        torch.cuda.synchronize()
        gm.use_graphs = False
        return st, st.dev["loss_out"].clone(), gm.proj.g.clone()

    st1, loss_e, g_e = step(b2, False)
    step(b1, True), step(b1, True)                                     # eager first pass of the key, then the capture
    st2, loss_g, g_g = step(b2, True)                                  # replay, other batch
    assert gm._shape_key(st1, "bwd") == gm._shape_key(st2, "bwd")
    assert gm._shape_key(st2, ("fwd_text", True, True)) in gm._graphs
    assert (gm._shape_key(st2, "bwd") in gm._graphs) == (not with_lora)
    assert torch.equal(loss_e, loss_g) and torch.equal(g_e, g_g)
    lo, hi = gm.embed_range
    assert float(g_g[lo:hi].abs().max()) > 0 and not torch.equal(g_g[lo:hi], step(b1, True)[2][lo:hi])


@pytest.mark.parametrize("tied", [True, False])
def test_use_emb_audio_branch_hip_vs_double(ops, tied):
    """One audio-branch step (encoder, PSD, projector, adapted decoder) on the HIP kernels against the CPU double: the bars
    tests/test_gpu_lora.py uses for adapters, on the table's gradient; untied, the same rows are exactly zero."""
    from test_use_emb_cpu import audio_case, run_audio
    geo, cfg, sd, lsd, batch, z = audio_case(tied)
    gm, cm = build_emb(geo, cfg, sd, lsd, ops, "cuda"), build_emb(geo, cfg, sd, lsd, FakeOps(), "cpu")
    sg, sc = run_audio(gm, batch), run_audio(cm, batch)
    torch.cuda.synchronize()
    assert sg.path == "audio" and np.array_equal(np.asarray(sg.dev["psd_lens"].cpu() if torch.is_tensor(sg.dev["psd_lens"]) else sg.dev["psd_lens"]), z["psd_lens"])
    assert abs(float(sg.dev["loss_out"][0]) - float(sc.dev["loss_out"][0])) < 2e-3
    g1, g2 = gm.embed_grad().cpu(), cm.embed_grad()
    c, rel = cosine(g1, g2), float((g1 - g2).norm() / g2.norm())
    print(f"audio branch tied={tied}: table cosine {c:.6f} relative error {rel:.2e}")
    assert c > 0.9995 and rel < 3e-2
    assert torch.equal(g1.norm(dim=1) == 0, g2.norm(dim=1) == 0)
    if not tied:
        assert float(g1[geo.speech_id].abs().max()) == 0.0 and 0 < int((g1.norm(dim=1) > 0).sum()) < 100


# ------------------------------------------------------------------------------------------ 7. after an engine step
def _factory(tied, fp16, use_emb=True, projector="linear-silu"):
    from ps_slm_amd.config import DEFAULT_DS_CONFIG, ModelConfig, TrainConfig, load_ds_config
    from ps_slm_amd.engine import TasuEngine
    from ps_slm_amd.ps_slm import model_factory
    tc = TrainConfig(freeze_llm=True, freeze_encoder=True, gt_emb=True, gt_emb_noise=False, ctc_posterior=True, do_psd=True,
                     use_fp16=fp16, use_peft=True, peft_config=dict(r=8, lora_alpha=16, lora_dropout=0.0))
    tc.use_emb = use_emb
    mc = ModelConfig(llm_path="synthetic:mid" if tied else "synthetic:mid-untied", encoder_projector=projector, llm_dim=256)
    model, tok = model_factory(tc, mc, device="cuda:0", init_seed=77)
    cfg = load_ds_config(DEFAULT_DS_CONFIG)
    cfg["lr"] = 2e-2                                                    # one step has to move the argmax of some position
    eng = TasuEngine(model, cfg)
    eng.sched_iter = 10
    return model, eng


@pytest.mark.parametrize("fp16", [True, False])
def test_decode_and_eval_follow_the_stepped_table(fp16):
    """Tied head.  generate() before the step fills every cache (fragment-order head, decode graphs, fp32 fragments); after one
    engine step it must equal, token for token, generate() of a fresh model loaded from the stepped model's state_dict() -- on the
    bf16 decode path (use_fp16=true) and on the fp32 one (use_fp16=false), where the fp32 eval loss is bit-equal too."""
    from ps_slm_amd.synthetic import random_lora_state_dict, synthetic_text_batch
    model, eng = _factory(True, fp16)
    core = model.core
    assert core.arith == ("bf16" if fp16 else "fp32") and core.arith_train == "bf16"
    core.lora.load_state_dict(random_lora_state_dict(core.geo, core.lora.cfg, 5, b_scale=0.05))
    core.sync_projector_copies()
    raw = synthetic_text_batch(core.geo, 2, seed=5, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=8, noise=False)
    ids = raw["input_ids"][:, :10]
    am = torch.ones_like(ids, dtype=torch.bool)
    targets = ["ab cde f ghij kl m", "no pq rst uvw"]
    gen = lambda m: m.generate(input_ids=ids, attention_mask=am, targets=targets, num_beams=4, max_new_tokens=12).cpu().numpy()
    ev = lambda m: m.eval()(**to_call(raw))[0].loss.detach().cpu().clone()
    model.eval()
    t0, l0 = gen(model), ev(model)
    model.train()
    out, _ = eng(**to_call(raw))
    eng.backward(out.loss)
    eng.step()
    model.eval()
    t1, l1 = gen(model), ev(model)
    fresh, _ = _factory(True, fp16)
    missing, unexpected = fresh.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    assert not missing and not unexpected
    t2, l2 = gen(fresh), ev(fresh)
    torch.cuda.synchronize()
    assert np.array_equal(t1, t2), (t1, t2)
    assert torch.equal(l1, l2) and not torch.equal(l1, l0)
    assert not np.array_equal(t0, t1)                                   # (the step did change what is decoded: the caches were live)


def test_cross_attention_tables_follow_the_stepped_untied_table(ops):
    """Untied head + the cross-attention projector (keys and values are the embedding table, read detached): the projector's bf16
    tables follow the trained values -- the eval loss changes after the step and equals a reloaded model's."""
    from conftest import ca_projector_case
    from ps_slm_amd.config import DEFAULT_DS_CONFIG, ModelConfig, TrainConfig, load_ds_config
    from ps_slm_amd.engine import TasuEngine
    from ps_slm_amd.lora import LoraConfig
    from ps_slm_amd.model import Geometry, TasuModel
    from ps_slm_amd.ps_slm import EMBED_KEY, SyntheticLLMTokenizer, setup_encoder_tokenizer, slam_model_asr
    from ps_slm_amd.synthetic import random_lora_state_dict, random_state_dict
    import dataclasses
    geo0, _, raw, z = ca_projector_case()
    geo = Geometry.from_dict(dict(dataclasses.asdict(geo0), tied=False))
    sd = random_state_dict(geo, int(z["seed_w"]), with_encoder=False)
    cfg = LoraConfig(r=8, lora_alpha=16, lora_dropout=0.0)

    def make():
        core = TasuModel(geo, ops, "cuda")
        core.load_reference_state_dict(sd)
        core.enable_lora(cfg)
        core.lora.load_state_dict(random_lora_state_dict(geo, cfg, 5, b_scale=0.05))
        core.enable_embedding_training()
        tc = TrainConfig(freeze_llm=True, freeze_encoder=True, gt_emb=True, gt_emb_noise=False, ctc_posterior=True, do_psd=True,
                         use_fp16=True, use_peft=True)
        mc = ModelConfig(llm_path="synthetic:mid-untied", encoder_projector="cross-attention")
        return slam_model_asr(core, SyntheticLLMTokenizer(geo), setup_encoder_tokenizer(mc, geo), tc, mc)

    model = make()
    core = model.core
    dscfg = load_ds_config(DEFAULT_DS_CONFIG)
    dscfg["lr"] = 2e-2
    eng = TasuEngine(model, dscfg)
    eng.sched_iter = 10
    call = dict(input_ids=raw["input_ids"], attention_mask=raw["attention_mask"], labels=raw["labels"], input_features=None,
                input_feature_length=None, GT=[" ".join(map(str, p)) for p in raw["post_ids"]])
    ev = lambda m: m.eval()(**call)[0].loss.detach().cpu().clone()
    l0 = ev(model)
    assert core.llm._ca_e.data_ptr() == core.embed_view(core.proj.pb).data_ptr()       # the bf16 image AdamW writes
    h0, w0 = core.llm.head.clone(), core.proj.p[: core.proj_end].clone()
    model.train()
    out, _ = eng(**call)
    eng.backward(out.loss)
    g = core.embed_grad()
    # the projector reads the table detached: only looked-up rows carry a gradient
    assert 0 < int((g.norm(dim=1) > 0).sum()) < 100
    # the table alone moves: put the projector's own weights back, so that the eval loss below can only follow the TABLE
    eng.step()
    core.proj.p[: core.proj_end].copy_(w0)
    core.sync_projector_copies()
    l1 = ev(model)
    assert torch.equal(core.llm.head, h0)
    assert torch.equal(core.llm._ca_et[:, : geo.llm_vocab], core.llm._ca_e.t())
    fresh = make()
    tab_only = {EMBED_KEY: model.state_dict()[EMBED_KEY].cpu()}
    lsd = {k: v.cpu() for k, v in model.state_dict().items() if ".lora_" in k}
    fresh.load_state_dict({**tab_only, **lsd})
    l2 = ev(fresh)
    assert torch.equal(l1, l2) and not torch.equal(l1, l0)
