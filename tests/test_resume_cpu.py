"""Resuming a training run (TasuEngine.save_state / load_state, ``train(resume=...)``, the ``deepspeed_ckpt_path`` /
``deepspeed_ckpt_id`` / ``state_interval`` keys), host logic on the CPU double.  The pattern and the recipes: tests/resume_cases.py.
On the double two uninterrupted runs are bit-equal, so every resumed run here is held to the uninterrupted run's bits."""
import json
import logging
import os
import random

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import dataset_fixtures as fx
import ps_slm_amd.engine as engine_mod
import resume_cases as rc
from conftest import free_port
from fake_ops import FakeOps
from full_ft_ops import FullFtFakeOps
from ps_slm_amd.config import LogConfig, RunConfig, TrainConfig, apply_overrides


def cpu(recipe, ops=FakeOps, **kw):
    return lambda other: rc.build(recipe, "cpu", ops=ops(), other=other, **kw)


# ------------------------------------------------------------------------------------------ 1-3. the engine, recipe by recipe
def test_shipped_recipe_resumes_bit_equal(tmp_path):
    """linear-silu projector, text branch, gt_emb_noise on (the CPS draws come from the torch CPU generator the state carries);
    N = 6, k = 3, lr raised so that steps move the weights visibly."""
    a, c, control = rc.resume_pattern(cpu("shipped", lr=2e-3), tmp_path, N=6, k=3, what="shipped (CPU double)")
    assert control == 0.0
    meta = json.load(open(tmp_path / "global_step3" / "meta.json"))
    assert (tmp_path / "latest").read_text() == "global_step3"
    assert meta["global_steps"] == 3 and meta["sched_iter"] == 13 and meta["micro_steps"] == 3 and meta["world"] == 1
    assert meta["numel"] == a.core.proj.p.numel() and meta["fingerprint"]["projector"] == "linear-silu"
    assert [e[0] for e in meta["fingerprint"]["entries"]] == ["encoder_projector." + n for n in a.core.proj.names]
    assert sorted(os.listdir(tmp_path / "global_step3")) == ["m.f32", "meta.json", "p.f32", "rank_0.pt", "v.f32"]
    assert os.path.getsize(tmp_path / "global_step3" / "p.f32") == 4 * meta["numel"]


def test_noise_draws_matter_for_the_pattern(tmp_path):
    """The pattern can see a generator that was not restored: the same resume with the CPU generator disturbed after load_state
    does not reproduce the uninterrupted losses."""
    model, eng = rc.build("shipped", "cpu", ops=FakeOps())
    raws = rc.batches(eng.core.geo, 2)
    torch.manual_seed(5)
    rc.run(eng, raws[:1])
    eng.save_state(str(tmp_path))
    want = rc.run(eng, raws[1:])
    m2, e2 = rc.build("shipped", "cpu", ops=FakeOps())
    e2.load_state(str(tmp_path))
    torch.manual_seed(6)
    assert not torch.equal(rc.run(e2, raws[1:])[0], want[0])
    e2.load_state(str(tmp_path))
    assert torch.equal(rc.run(e2, raws[1:])[0], want[0])


def test_accumulation_window_survives_an_odd_micro_step(tmp_path):
    """gradient_accumulation_steps = 2, saved after micro-step 3: _g_acc and micro_steps travel, the next boundary step equals
    the uninterrupted one."""
    def dirty(model, eng):
        eng._g_acc.fill_(7.0)
    a, c, control = rc.resume_pattern(cpu("shipped", lr=2e-3, ga=2), tmp_path, N=6, k=3, what="ga=2", before_load=dirty)
    assert control == 0.0
    assert "g_acc.f32" in os.listdir(tmp_path / "global_step1")
    meta = json.load(open(tmp_path / "global_step1" / "meta.json"))
    assert meta["micro_steps"] == 3 and meta["global_steps"] == 1 and meta["gradient_accumulation_steps"] == 2
    # a state from the middle of a window does not load into a run that accumulates differently
    _, e1 = rc.build("shipped", "cpu", ops=FakeOps(), ga=1)
    with pytest.raises(ValueError, match="accumulation window"):
        e1.load_state(str(tmp_path))


@pytest.mark.parametrize("recipe,ops", [("lora_emb", FakeOps), ("full_ft", FullFtFakeOps), ("full_ft_untied", FullFtFakeOps)])
def test_lora_dropout_use_emb_and_full_ft_resume_bit_equal(tmp_path, recipe, ops):
    a, c, control = rc.resume_pattern(cpu(recipe, ops=ops), tmp_path, N=4, k=2, what=recipe)
    assert control == 0.0
    core = c.core
    keys = [e[0] for e in json.load(open(tmp_path / "global_step2" / "meta.json"))["fingerprint"]["entries"]]
    assert keys == [k for k, _, _ in c._views(core.proj.p)]          # the bucket's tensors, in bucket order of named_parameters()
    if recipe == "lora_emb":
        assert int(core.lora.rng[1]) == 4                             # the dropout counter went on from the saved position
    # what derives from the masters followed: the eval loss of the resumed model is the uninterrupted model's
    raw = rc.batches(core.geo, 1, seed=77)[0]
    ev = lambda m: m.eval()(**rc.to_call(raw))[0].loss.detach().clone()
    torch.manual_seed(1)
    la = ev(a)
    torch.manual_seed(1)
    assert torch.equal(la, ev(c))


# ------------------------------------------------------------------------------------------ 4. two ranks
def _dp_worker(rank, world, port, root, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    make = lambda other: rc.build("shipped", "cpu", ops=FakeOps(), other=other, lr=2e-3)
    real = rc.batches
    rc.batches = lambda geo, n, seed=300: real(geo, n, seed=seed + 50 * rank)      # every rank its own data
    try:
        a, c, control = rc.resume_pattern(make, root, N=4, k=2, what=f"rank {rank} of {world}")
    finally:
        rc.batches = real
    ret[rank] = dict(control=control, p=c.core.proj.p.clone(), files=sorted(os.listdir(os.path.join(root, "global_step2"))))
    dist.destroy_process_group()


def test_two_ranks_resume_and_world_size_is_checked(tmp_path):
    world, port = 2, free_port()
    ret = mp.Manager().dict()
    mp.spawn(_dp_worker, args=(world, port, str(tmp_path), ret), nprocs=world, join=True)
    assert ret[0]["control"] == 0.0 and ret[1]["control"] == 0.0
    assert torch.equal(ret[0]["p"], ret[1]["p"])
    assert ret[0]["files"] == ["m.f32", "meta.json", "p.f32", "rank_0.pt", "rank_1.pt", "v.f32"]
    _, eng = rc.build("shipped", "cpu", ops=FakeOps())
    before = rc.snapshot(eng)
    with pytest.raises(ValueError, match="world size 2"):
        eng.load_state(str(tmp_path))
    after = rc.snapshot(eng)
    assert all(torch.equal(before[k], after[k]) for k in ("p", "m", "v", "pb")) and before["counters"] == after["counters"]


# ------------------------------------------------------------------------------------------ 5. the training loop
class _Cap(Exception):
    pass


def _cap_steps(eng, n):
    """The test's step cap: the n + 1-th optimizer step does not happen (nothing is killed)."""
    real, calls = eng.step, [0]

    def step():
        if calls[0] >= n:
            raise _Cap()
        calls[0] += 1
        real()
    eng.step = step


class _Tok(fx.CharTokenizer):
    eos_token_id, pad_token_id = 980, 981

    def encode(self, text):
        return [990 if t == fx.SPEECH_ID else t for t in super().encode(text)]


def _dataset(kind, geo, root):
    from ps_slm_amd.finetune_deepspeed import SyntheticDataset, get_dataset
    if kind == "synthetic":
        return SyntheticDataset(geo, 2, 5, 0)
    dirs = fx.write_corpus(str(root), split_sizes=(("train", 9),))    # 9 utterances under a 260-frame budget: 5 batches
    cfg = fx.dataset_config(str(root), dirs, False, 260)
    cfg.text_only, cfg.file = True, "ps_slm_amd/dataset.py:get_speech_dataset"
    ds = get_dataset(cfg, _Tok(), "train", geo, 0)
    ds.dp.rng = random.Random(4242)                       # the split's own generator, as main() installs it
    assert sum(1 for _ in ds) == 5
    ds.dp.rng = random.Random(4242)
    return ds


@pytest.mark.parametrize("kind", ["synthetic", "jsonl"])
@pytest.mark.parametrize("workers", [0, 1])
def test_train_loop_resumes_in_the_second_epoch(tmp_path, kind, workers):
    """Two epochs of 5 batches, state_interval = 3; the first process stops after step 7 (epoch 2), the second resumes from
    ``latest`` (step 6): final state_dict() and the metrics records after the split equal the uninterrupted run's; the two newest
    tags remain."""
    import ps_slm_amd.synthetic as syn
    from ps_slm_amd.finetune_deepspeed import train
    real = syn.synthetic_text_batch
    syn.synthetic_text_batch = lambda geo, B, seed, noise=False: real(geo, B, seed=seed, prompt_len=9, n_audio=21, target_len=17,
                                                                       speech_pos=4, feat_frames=8, noise=noise)
    tcfg = TrainConfig(num_epochs=2, run_validation=False, save_model=False, batching_strategy="dynamic", num_workers_dataloader=workers)

    def go(name, cap=None, resume_from=None, other=False):
        model, eng = rc.build("shipped", "cpu", ops=FakeOps(), other=other, lr=2e-3)
        ds = _dataset(kind, eng.core.geo, tmp_path / "corpus")
        lcfg = LogConfig(log_interval=1, use_wandb=True, wandb_dir=str(tmp_path / name))
        state_dir = str(tmp_path / (resume_from or name) / "state")
        resume = None
        if resume_from:
            rc.spoil(model, eng)
            _, resume = eng.load_state(state_dir)
        else:
            torch.manual_seed(5)
        if cap:
            _cap_steps(eng, cap)
        try:
            res = train(eng, ds, tcfg, lcfg, 0, 1, resume=resume, state_dir=state_dir, state_interval=3)
        except _Cap:
            res = None
        recs = [json.loads(l) for l in open(tmp_path / name / "metrics.jsonl")]
        return model, eng, res, recs

    try:
        m_a, e_a, res_a, recs_a = go("straight")
        _, e_b, res_b, recs_b = go("first", cap=7)
        assert res_b is None and e_b.global_steps == 7
        assert sorted(os.listdir(tmp_path / "first" / "state")) == ["global_step3", "global_step6", "latest"]
        assert (tmp_path / "first" / "state" / "latest").read_text() == "global_step6"
        m_c, e_c, res_c, recs_c = go("second", resume_from="first", other=True)
    finally:
        syn.synthetic_text_batch = real
    assert res_a["steps"] == res_c["steps"] == 10 and e_c.global_steps == 10
    sd_a, sd_c = m_a.state_dict(), m_c.state_dict()
    assert sorted(sd_a) == sorted(sd_c) and all(torch.equal(sd_a[k], sd_c[k]) for k in sd_a)
    assert len(recs_a) == 12 and len(recs_c) == 5 and recs_a[-5:] == recs_c          # steps 7..10 and the second epoch's record
    assert recs_b[:6] == recs_a[:6]
    assert res_a["avg_train_loss"] == res_c["avg_train_loss"] and res_a["avg_train_acc"] == res_c["avg_train_acc"]
    assert sorted(os.listdir(tmp_path / "first" / "state")) == ["global_step6", "global_step9", "latest"]
    assert sorted(os.listdir(tmp_path / "straight" / "state")) == ["global_step6", "global_step9", "latest"]


def test_state_goes_with_the_weights_a_validation_improvement_saves(tmp_path):
    """state_interval = 0 with a state directory: a state is written at the end of every iteration whose validation pass wrote
    pytorch_model.bin (the first pass always improves on +inf); resuming from it reproduces the rest of the run, the validation
    records and the best-so-far figures included."""
    import ps_slm_amd.synthetic as syn
    from ps_slm_amd.finetune_deepspeed import SyntheticDataset, train
    real = syn.synthetic_text_batch
    syn.synthetic_text_batch = lambda geo, B, seed, noise=False: real(geo, B, seed=seed, prompt_len=9, n_audio=21, target_len=17,
                                                                       speech_pos=4, feat_frames=8, noise=noise)

    def go(name, cap=None, resume_from=None):
        model, eng = rc.build("shipped", "cpu", ops=FakeOps(), lr=2e-3)
        tcfg = TrainConfig(num_epochs=1, run_validation=True, validation_interval=2, save_model=True, batching_strategy="dynamic",
                           output_dir=str(tmp_path / name / "out"), num_workers_dataloader=0)
        lcfg = LogConfig(log_interval=1, use_wandb=True, wandb_dir=str(tmp_path / name))
        state_dir, resume = str(tmp_path / (resume_from or name) / "state"), None
        if resume_from:
            rc.spoil(model, eng)
            _, resume = eng.load_state(state_dir, tag="global_step2")
        else:
            torch.manual_seed(5)
        if cap:
            _cap_steps(eng, cap)
        try:
            res = train(eng, SyntheticDataset(eng.core.geo, 2, 5, 0), tcfg, lcfg, 0, 1, eval_dataset=SyntheticDataset(eng.core.geo, 2, 2, 0),
                        resume=resume, state_dir=state_dir, state_interval=0)
        except _Cap:
            res = None
        return model, res, [json.loads(l) for l in open(tmp_path / name / "metrics.jsonl")]

    try:
        m_a, res_a, recs_a = go("straight")
        go("first", cap=3)
        assert "global_step2" in os.listdir(tmp_path / "first" / "state")
        assert os.path.isfile(tmp_path / "first" / "out" / "asr_model_epoch_1_step_2" / "pytorch_model.bin")
        m_c, res_c, recs_c = go("second", resume_from="first")
    finally:
        syn.synthetic_text_batch = real
    sd_a, sd_c = m_a.state_dict(), m_c.state_dict()
    assert all(torch.equal(sd_a[k], sd_c[k]) for k in sd_a)
    assert len(recs_c) >= 5 and recs_a[-len(recs_c):] == recs_c and any("valid/best_val_loss" in r for r in recs_c)
    assert {k: v for k, v in res_a.items() if "per_s" not in k} == {k: v for k, v in res_c.items() if "per_s" not in k}


def test_new_config_keys():
    cfg = RunConfig()
    assert cfg.deepspeed_ckpt_path is None and cfg.deepspeed_ckpt_id is None and cfg.state_interval == 0
    assert {"deepspeed_ckpt_path", "deepspeed_ckpt_id", "state_interval"} <= set(cfg.keys())
    cfg = apply_overrides(cfg, ["++deepspeed_ckpt_path=/x/state", "++deepspeed_ckpt_id=global_step12", "++state_interval=500"])
    assert cfg.deepspeed_ckpt_path == "/x/state" and cfg.deepspeed_ckpt_id == "global_step12" and cfg.state_interval == 500


# ------------------------------------------------------------------------------------------ 6. refusals
def _untouched(eng, fn, exc, match):
    before = rc.snapshot(eng)
    with pytest.raises(exc, match=match):
        fn()
    after = rc.snapshot(eng)
    assert all(torch.equal(before[k], after[k]) for k in ("p", "m", "v", "pb")) and before["counters"] == after["counters"]


def test_refusals_come_before_anything_is_overwritten(tmp_path):
    _, lora = rc.build("lora_emb", "cpu", ops=FakeOps())
    rc.run(lora, rc.batches(lora.core.geo, 1))
    lora.save_state(str(tmp_path / "lora"))
    _, plain = rc.build("shipped", "cpu", ops=FakeOps())
    rc.run(plain, rc.batches(plain.core.geo, 1))
    plain.save_state(str(tmp_path / "plain"))
    # LoRA state into a model without adapters: the first entry only the state holds is named
    first_lora = next(iter(lora.core.lora.names()))[0]
    _untouched(plain, lambda: plain.load_state(str(tmp_path / "lora")), ValueError, "lora_A")
    with pytest.raises(ValueError) as e:
        plain.load_state(str(tmp_path / "lora"))
    assert first_lora in str(e.value)
    # another projector kind: the first differing key is the projector's first tensor
    _, lin = rc.build("shipped", "cpu", ops=FakeOps(), projector="linear")
    _untouched(lin, lambda: lin.load_state(str(tmp_path / "plain")), ValueError, "encoder_projector.norm.weight")
    # truncated tensor file
    v = tmp_path / "plain" / "global_step1" / "v.f32"
    blob = v.read_bytes()
    v.write_bytes(blob[:-4])
    _untouched(plain, lambda: plain.load_state(str(tmp_path / "plain")), ValueError, "v.f32")
    v.write_bytes(blob)
    plain.load_state(str(tmp_path / "plain"))
    # latest names a tag that is not there; a directory without latest
    (tmp_path / "plain" / "latest").write_text("global_step99")
    _untouched(plain, lambda: plain.load_state(str(tmp_path / "plain")), FileNotFoundError, "global_step99")
    _untouched(plain, lambda: plain.load_state(str(tmp_path / "nowhere")), FileNotFoundError, "latest")
    assert plain.load_checkpoint(str(tmp_path / "plain"), tag="global_step1")[0].endswith("global_step1")   # DeepSpeed's name


def test_entrypoint_starts_fresh_when_the_state_directory_is_missing(tmp_path, caplog, monkeypatch):
    """deepspeed_ckpt_path set, nothing there: main() says so and trains from step 0 (the same command line serves the first
    launch and every relaunch).  The double stands in for the GPU: main()'s device calls are patched out."""
    import ps_slm_amd.finetune_deepspeed as ft
    import ps_slm_amd.synthetic as syn
    real_factory = ft.get_custom_model_factory
    monkeypatch.setattr(ft, "ensure_hw_queues", lambda: None)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(ft, "get_custom_model_factory", lambda mc: lambda tc, mcfg, **kw: real_factory(mc)(
        tc, mcfg, **dict(kw, device="cpu", ops=FakeOps())))
    real = syn.synthetic_text_batch
    monkeypatch.setattr(syn, "synthetic_text_batch", lambda geo, B, seed, noise=False: real(
        geo, B, seed=seed, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=8, noise=noise))
    state = tmp_path / "state"
    argv = ["++model_config.llm_path=synthetic:mid", "++model_config.llm_dim=256", "++model_config.encoder_projector=linear-silu",
            "++train_config.freeze_llm=true", "++train_config.freeze_encoder=true", "++train_config.gt_emb=true",
            "++train_config.ctc_posterior=true", "++train_config.num_epochs=1", "++train_config.run_validation=false",
            "++train_config.save_model=false", "++train_config.num_workers_dataloader=0", "++dataset_config.file=synthetic",
            "++synthetic_steps=3", "++synthetic_batch=2", f"++deepspeed_ckpt_path={state}", "++state_interval=2"]
    with caplog.at_level(logging.INFO, logger="ps_slm_amd.finetune_deepspeed"):
        res = ft.main(argv)
    assert res["steps"] == 3 and any("starting fresh" in r.getMessage() for r in caplog.records)
    assert sorted(os.listdir(state)) == ["global_step2", "latest"]
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="ps_slm_amd.finetune_deepspeed"):
        res = ft.main(argv)                                # relaunch: resumes behind step 2, one step is left
    assert any("resuming from" in r.getMessage() for r in caplog.records) and res["steps"] == 3
    assert sorted(os.listdir(state)) == ["global_step2", "latest"]


# ------------------------------------------------------------------------------------------ 7-8. the files
def test_chunked_io_round_trips_a_bucket_that_is_no_multiple_of_the_chunk(tmp_path, monkeypatch):
    monkeypatch.setattr(engine_mod, "STATE_CHUNK_ELEMS", 1000)
    _, eng = rc.build("shipped", "cpu", ops=FakeOps())
    rc.run(eng, rc.batches(eng.core.geo, 2))
    numel = eng.core.proj.p.numel()
    assert numel % 1000 != 0 and numel > 3000
    want = rc.snapshot(eng)
    eng.save_state(str(tmp_path), tag="mine")
    assert eng._stage.numel() == 1000
    _, other = rc.build("shipped", "cpu", ops=FakeOps())
    rc.spoil(None, other)
    path, client = other.load_state(str(tmp_path))
    got = rc.snapshot(other)
    assert path.endswith("mine") and client is None and other._stage.numel() == 1000
    assert all(torch.equal(want[k], got[k]) for k in ("p", "m", "v", "pb")) and want["counters"] == got["counters"]
    import numpy as np
    assert np.array_equal(np.fromfile(tmp_path / "mine" / "m.f32", dtype="<f4"), want["m"].numpy())


def test_interrupted_save_is_ignored(tmp_path):
    """A temporary directory left by a save that died (made by hand) is never ``latest``, does not load, survives pruning
    untouched, and the next save of the same tag replaces it."""
    from ps_slm_amd.finetune_deepspeed import _prune_states
    _, eng = rc.build("shipped", "cpu", ops=FakeOps())
    rc.run(eng, rc.batches(eng.core.geo, 1))
    eng.save_state(str(tmp_path))
    os.makedirs(tmp_path / "global_step2.tmp")
    (tmp_path / "global_step2.tmp" / "p.f32").write_bytes(b"\0" * 64)
    assert (tmp_path / "latest").read_text() == "global_step1"
    _prune_states(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["global_step1", "global_step2.tmp", "latest"]
    _, other = rc.build("shipped", "cpu", ops=FakeOps())
    assert other.load_state(str(tmp_path))[0].endswith("global_step1") and other.global_steps == 1
    with pytest.raises(FileNotFoundError):
        other.load_state(str(tmp_path), tag="global_step2.tmp")
    rc.run(eng, rc.batches(eng.core.geo, 1))
    eng.save_state(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["global_step1", "global_step2", "latest"]
    assert (tmp_path / "latest").read_text() == "global_step2" and "meta.json" in os.listdir(tmp_path / "global_step2")
