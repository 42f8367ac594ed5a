"""Shared by tests/test_resume_cpu.py (FakeOps double) and tests/test_gpu_resume.py (HipOps): the recipes and the one pattern
every resume test follows (TasuEngine.save_state / load_state, DESIGN.md "Training state").

    1. A : N optimizer steps, uninterrupted            A' : the same again -- the control
    2. B : k steps, then save_state
    3. C : another model, everything the state must bring back made different first (see ``spoil``)
    4. C : load_state, then the remaining N - k steps on the same batches
    5. C against A: p, m, v and the bf16 image of the WHOLE bucket, the losses after the split, get_lr(), the three counters

"Equal" is ``torch.equal``.  Where the control is bit-equal (the expected case) the resumed run must be; where it is not, the
measured A-A' difference is reported and the resumed run is held to twice it (``compare``).

What "another model" means: where the decoder itself trains (freeze_llm=false) C is built from another ``init_seed`` outright.
Where the decoder is frozen its weights are not part of a training state -- a run is resumed on the same base model -- so C gets
the same frozen weights, and ``spoil`` then rewrites every element of p, m and v, runs a step on a foreign batch (counters,
schedule position, dropout counter, accumulation buffer and CPU generator all move) and, if asked, a generate() that fills every
decode-time cache with the spoiled weights."""
import torch

from ps_slm_amd.config import DEFAULT_DS_CONFIG, ModelConfig, TrainConfig, load_ds_config
from ps_slm_amd.engine import TasuEngine
from ps_slm_amd.ps_slm import model_factory
from ps_slm_amd.synthetic import synthetic_text_batch

RECIPES = {   # name -> (TrainConfig fields, llm_path, C takes another init_seed)
    "shipped": (dict(freeze_llm=True, gt_emb_noise=True, use_fp16=True), "synthetic:mid", False),
    # (the graph cases keep the CPS noise off: with drops every batch has its own row count and no step would ever be replayed)
    "shipped_static": (dict(freeze_llm=True, gt_emb_noise=False, use_fp16=True), "synthetic:mid", False),
    "shipped_fp32": (dict(freeze_llm=True, gt_emb_noise=True, use_fp16=False), "synthetic:mid", False),
    "lora_emb": (dict(freeze_llm=True, gt_emb_noise=True, use_fp16=True, use_peft=True, use_emb=True,
                      peft_config=dict(r=8, lora_alpha=16, lora_dropout=0.05)), "synthetic:mid", False),
    "full_ft": (dict(freeze_llm=False, gt_emb_noise=True, use_fp16=True), "synthetic:mid", True),
    "full_ft_untied": (dict(freeze_llm=False, gt_emb_noise=True, use_fp16=True), "synthetic:mid-untied", True),
}


def build(recipe, device, ops=None, other=False, lr=1e-3, ga=1, graphs=False, projector="linear-silu"):
    kw, llm_path, reseed = RECIPES[recipe]
    kw = dict(kw)
    peft = kw.pop("peft_config", None)
    use_emb = kw.pop("use_emb", False)
    tc = TrainConfig(freeze_encoder=True, gt_emb=True, ctc_posterior=True, do_psd=True, **kw)
    if peft:
        tc.peft_config.r, tc.peft_config.lora_alpha, tc.peft_config.lora_dropout = peft["r"], peft["lora_alpha"], peft["lora_dropout"]
    tc.use_emb = use_emb
    mc = ModelConfig(llm_path=llm_path, encoder_projector=projector, llm_dim=256)
    extra = {} if ops is None else {"ops": ops}
    model, _ = model_factory(tc, mc, device=device, init_seed=4321 if (other and reseed) else 1234, keep_logits=False, **extra)
    model.core.use_graphs = graphs
    cfg = load_ds_config(DEFAULT_DS_CONFIG)
    cfg.update(lr=lr, gradient_accumulation_steps=ga)
    eng = TasuEngine(model, cfg)
    eng.sched_iter = 10                      # past the zero-lr warm-up steps
    return model, eng


def batches(geo, n, seed=300):
    """n batches of 2 utterances, 47 merged positions (9 prompt + 21 pseudo-posterior rows + 17 target)."""
    return [synthetic_text_batch(geo, 2, seed=seed + i, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=8,
                                 noise=False) for i in range(n)]


def to_call(raw):
    return dict(input_ids=raw["input_ids"], attention_mask=raw["attention_mask"], labels=raw["labels"],
                input_features=raw["input_features"], input_feature_length=raw["input_feature_length"],
                GT=[" ".join(map(str, p)) for p in raw["post_ids"]])


def run(eng, raws):
    """One engine(**batch) / backward / step per batch -> the losses (bit patterns, as CPU tensors)."""
    losses = []
    for raw in raws:
        out, _ = eng(**to_call(raw))
        eng.backward(out.loss)
        eng.step()
        losses.append(out.loss.detach().float().cpu().clone())
    return losses


def snapshot(eng):
    pr = eng.core.proj
    s = {n: getattr(pr, n).detach().cpu().clone() for n in ("p", "m", "v", "pb")}
    if eng.ga > 1:
        s["g_acc"] = eng._g_acc.detach().cpu().clone()
    s["lr"], s["counters"] = eng.get_lr(), (eng.global_steps, eng.sched_iter, eng.micro_steps)
    if eng.core.lora is not None:
        s["lora_rng"] = eng.core.lora.rng.cpu().clone()
    return s


def spoil(model, eng, generate=None):
    """Everything a state must restore, made different in C (module docstring)."""
    pr = eng.core.proj
    g = torch.Generator().manual_seed(777)
    noise = lambda scale: (torch.randn(pr.p.numel(), generator=g) * scale).to(pr.p.device)
    pr.p.add_(noise(0.01))
    pr.m.copy_(noise(0.01))
    pr.v.copy_(noise(0.01).abs())
    eng.core.sync_projector_copies()
    torch.manual_seed(99)
    run(eng, batches(eng.core.geo, eng.ga, seed=900))
    if generate is not None:
        generate(model)                      # decode-time caches now hold the spoiled weights
        model.train()
    assert eng.global_steps == 1


def max_diff(a, b):
    """Largest absolute difference over the tensors of two snapshots / two loss lists (0.0 = bit-equal where torch.equal holds)."""
    worst = 0.0
    for x, y in zip(a, b):
        if not torch.equal(x, y):
            worst = max(worst, float((x.double() - y.double()).abs().max()), 5e-324)
    return worst


def compare(sa, sc, la, lc, control, what):
    """C against A.  ``control``: the A-A' difference (0.0 = bit-equal: then C must be bit-equal to A)."""
    assert sa["counters"] == sc["counters"] and sa["lr"] == sc["lr"], (what, sa["counters"], sc["counters"], sa["lr"], sc["lr"])
    keys = [k for k in sa if torch.is_tensor(sa[k])]
    d = max(max_diff([sa[k] for k in keys], [sc[k] for k in keys]), max_diff(la, lc))
    print(f"{what}: control A-A' max difference {control:.3e}, resumed C-A max difference {d:.3e}")
    if control == 0.0:
        for k in keys:
            assert torch.equal(sa[k], sc[k]), (what, k)
        assert len(la) == len(lc) and all(torch.equal(x, y) for x, y in zip(la, lc)), (what, la, lc)
    else:
        assert d <= 2 * control, (what, d, control)


def resume_pattern(make, save_dir, N=4, k=2, what="", generate=None, before_load=None):
    """``make(other)`` -> (model, engine).  Returns (A's model, C's model, A-A' difference) for further checks; N and k count
    micro-batches (= optimizer steps unless the engine accumulates)."""
    geo = None
    runs = []
    for _ in range(2):                                   # A and the control A'
        model, eng = make(False)
        geo = eng.core.geo
        raws = batches(geo, N)
        torch.manual_seed(5)
        runs.append((model, eng, run(eng, raws)))
    (model_a, eng_a, la), (_, eng_a2, la2) = runs
    sa = snapshot(eng_a)
    s2 = snapshot(eng_a2)
    keys = [x for x in sa if torch.is_tensor(sa[x])]
    control = max(max_diff([sa[x] for x in keys], [s2[x] for x in keys]), max_diff(la, la2))
    del runs, eng_a2
    model_b, eng_b = make(False)
    torch.manual_seed(5)
    lb = run(eng_b, raws[:k])
    path = eng_b.save_state(str(save_dir), client_state={"k": k})
    assert control != 0.0 or all(torch.equal(x, y) for x, y in zip(la[:k], lb))
    sb = snapshot(eng_b)
    model_c, eng_c = make(True)
    spoil(model_c, eng_c, generate)
    sx = snapshot(eng_c)                                 # (the pattern can fail: nothing of C is what the state holds)
    assert all(not torch.equal(sb[x], sx[x]) for x in ("p", "m", "v", "pb")) and sb["counters"] != sx["counters"]
    assert not all(torch.equal(x, la[0]) for x in la[1:])
    if before_load is not None:
        before_load(model_c, eng_c)
    got, client = eng_c.load_state(str(save_dir))
    assert got == path and client == {"k": k}
    lc = run(eng_c, raws[k:])
    compare(sa, snapshot(eng_c), la[k:], lc, control, what)
    return model_a, model_c, control
