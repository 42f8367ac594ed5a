"""Resuming a training run on the MI355X (TasuEngine.save_state / load_state, ``train(resume=...)``, the entrypoint's
``deepspeed_ckpt_path`` / ``state_interval`` keys) through the HIP kernels.  The pattern and the recipes: tests/resume_cases.py --
every test first runs the control (two uninterrupted runs A, A'); where it is bit-equal the resumed run must equal A bit for
bit.  All models at the ``synthetic:mid`` geometry, 2 utterances of 47 merged positions, N = 4 optimizer steps, split at k = 2."""
import json
import os

import numpy as np
import pytest
import torch

import resume_cases as rc
from ps_slm_amd.config import LogConfig, TrainConfig

pytestmark = pytest.mark.gpu


def gpu(recipe, **kw):
    return lambda other: rc.build(recipe, "cuda:0", other=other, **kw)


def _generate(model):
    raw = rc.batches(model.core.geo, 1, seed=41)[0]
    ids = raw["input_ids"][:, :10]
    am = torch.ones_like(ids, dtype=torch.bool)
    model.eval()
    out = model.generate(input_ids=ids, attention_mask=am, targets=["ab cde f ghij kl m", "no pq rst uvw"], num_beams=4,
                         max_new_tokens=8).cpu().numpy()
    model.train()
    return out


# ------------------------------------------------------------------------------------------ 1 + 3. recipe by recipe
@pytest.mark.parametrize("recipe,graphs,decode", [
    ("shipped", False, False), ("shipped_static", True, False), ("lora_emb", False, True), ("full_ft", False, True),
    ("full_ft_untied", False, True), ("shipped_fp32", False, True)])
def test_resumed_run_equals_the_uninterrupted_run(tmp_path, recipe, graphs, decode):
    """p, m, v, the bf16 image, losses, lr and counters of the resumed run against the uninterrupted one; for the recipes that
    move decoder weights (and for the fp32 decode path) generate() -- beam 4, 8 new tokens -- of the resumed model gives the
    uninterrupted model's tokens, although C had decoded with other weights before the load (every decode-time copy was live:
    transposes, fragment-order decode weights, merged adapters, fp32 copies)."""
    a, c, control = rc.resume_pattern(gpu(recipe, graphs=graphs), tmp_path, N=4, k=2, what=f"{recipe}{' + graphs' if graphs else ''}",
                                      generate=_generate if decode else None)
    if recipe == "shipped_fp32":
        assert a.core.arith == "fp32" and a.core.arith_train == "fp32"
    if graphs:
        assert len(c.core._graphs) > 0                    # steps 3 and 4 of C were captured / replayed
    if decode:
        ta, tc = _generate(a), _generate(c)
        torch.cuda.synchronize()
        assert ta.shape[1] >= 1 and np.array_equal(ta, tc), (ta, tc)


# ------------------------------------------------------------------------------------------ 2. into live graphs
def test_load_into_an_engine_whose_step_graphs_are_live(tmp_path):
    """C has replayed its step graphs before load_state: the load writes the buffers the graphs read IN PLACE, so the very next
    replay continues A's run; no graph is dropped or re-captured."""
    seen = {}

    def warm(model, eng):
        rc.run(eng, rc.batches(eng.core.geo, 3, seed=900))           # eager, capture + replay, replay
        seen["graphs"] = {k: id(model.core._graphs._graphs[k][0]) for k in model.core._graphs}
        seen["ptr"] = model.core.proj.p.data_ptr()
        assert seen["graphs"]
    a, c, control = rc.resume_pattern(gpu("shipped_static", graphs=True), tmp_path, N=4, k=2, what="load into live graphs", before_load=warm)
    assert {k: id(c.core._graphs._graphs[k][0]) for k in c.core._graphs} == seen["graphs"] and c.core.proj.p.data_ptr() == seen["ptr"]


# ------------------------------------------------------------------------------------------ 4. the entrypoint
def test_entrypoint_relaunch_ends_where_a_straight_run_ends(tmp_path, monkeypatch):
    """finetune_deepspeed.main on a generated jsonl corpus (text-only alignment recipe with CPS noise, reader thread on), three
    epochs of two batches, state_interval = 3: a run that stops after step 4 and is launched again with the SAME argument list
    writes the pytorch_model.bin of a straight run."""
    import dataset_fixtures as fx
    from ps_slm_amd.engine import TasuEngine
    from ps_slm_amd.finetune_deepspeed import main
    dirs = fx.write_corpus(str(tmp_path), split_sizes=(("train", 4),))
    with open(tmp_path / "multiprompt.jsonl", "w") as f:
        for task, prompt in (("ASR", "11 12 13"), ("ASR", "14 15"), ("ST", "21 22"), ("hotword", "31 32 33 34")):
            f.write(json.dumps({"task": task, "prompt": prompt}) + "\n")

    def argv(name):
        return ["++model_config.file=ps_slm_amd/ps_slm.py:model_factory", "++model_config.llm_path=synthetic:mid", "++model_config.llm_dim=256",
                "++model_config.encoder_projector=linear-silu", "++train_config.freeze_llm=true", "++train_config.freeze_encoder=true",
                "++train_config.gt_emb=true", "++train_config.gt_emb_noise=true", "++train_config.ctc_posterior=true",
                "++train_config.use_fp16=true", "++train_config.do_psd=true", "++train_config.num_epochs=3",
                "++train_config.run_validation=false", "++train_config.save_model=true", f"++train_config.output_dir={tmp_path}/{name}/out",
                "++dataset_config.file=ps_slm_amd/dataset.py:get_speech_dataset", f"++dataset_config.train_scp_file_path={dirs['train']}",
                f"++dataset_config.multitask_prompt_path={tmp_path}/multiprompt.jsonl", "++dataset_config.prompt_style={} 990",
                "++dataset_config.text_only=true", "++dataset_config.train_max_frame_length=25", "++dataset_config.ds_rate=8",
                "++metric=acc", "++log_config.log_interval=1", f"++deepspeed_ckpt_path={tmp_path}/{name}/state", "++state_interval=3"]

    straight = main(argv("straight"))
    assert straight["steps"] == 6                          # 2 batches x 3 epochs

    class Cap(Exception):
        pass
    real, calls = TasuEngine.step, [0]

    def capped(self):
        if calls[0] >= 4:
            raise Cap()
        calls[0] += 1
        real(self)
    monkeypatch.setattr(TasuEngine, "step", capped)
    with pytest.raises(Cap):
        main(argv("twice"))
    monkeypatch.setattr(TasuEngine, "step", real)
    assert (tmp_path / "twice" / "state" / "latest").read_text() == "global_step3"
    assert not os.path.exists(tmp_path / "twice" / "out" / "pytorch_model.bin")
    again = main(argv("twice"))
    assert again["steps"] == 6
    assert sorted(os.listdir(tmp_path / "twice" / "state")) == ["global_step3", "global_step6", "latest"]
    sa = torch.load(tmp_path / "straight" / "out" / "pytorch_model.bin")
    sb = torch.load(tmp_path / "twice" / "out" / "pytorch_model.bin")
    assert sorted(sa) == sorted(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert again["avg_train_loss"] == straight["avg_train_loss"]


# ------------------------------------------------------------------------------------------ 5. a step that does not save
def test_steps_that_do_not_save_issue_the_same_launches(tmp_path):
    """tasu_gemm_launch_count over every step of train() with and without state_interval: the same GEMM launches step for step
    (saving is copies and file writes: the interval that holds the save adds none either), and the same losses."""
    import ps_slm_amd.synthetic as syn
    from ps_slm_amd.finetune_deepspeed import SyntheticDataset, train
    real = syn.synthetic_text_batch
    syn.synthetic_text_batch = lambda geo, B, seed, noise=False: real(geo, B, seed=seed, prompt_len=9, n_audio=21, target_len=17,
                                                                       speech_pos=4, feat_frames=8, noise=noise)

    def go(interval):
        model, eng = rc.build("shipped", "cuda:0")
        lib = eng.core.ops.lib
        counts, step = [], eng.step

        def counted():
            step()
            counts.append(int(lib.tasu_gemm_launch_count()))
        eng.step = counted
        tcfg = TrainConfig(num_epochs=1, run_validation=False, save_model=False, batching_strategy="dynamic", num_workers_dataloader=0)
        torch.manual_seed(5)
        res = train(eng, SyntheticDataset(eng.core.geo, 2, 5, 0), tcfg, LogConfig(log_interval=1), 0, 1,
                    state_dir=str(tmp_path / f"state{interval}") if interval else None, state_interval=interval)
        return [b - a for a, b in zip(counts, counts[1:])], res, rc.snapshot(eng)

    try:
        plain, res0, s0 = go(0)
        saving, res3, s3 = go(3)
    finally:
        syn.synthetic_text_batch = real
    assert os.listdir(tmp_path / "state3") and not os.path.exists(tmp_path / "state0")
    assert len(plain) == 4 and min(plain) > 0 and plain == saving, (plain, saving)
    assert res0["avg_train_loss"] == res3["avg_train_loss"] and all(torch.equal(s0[k], s3[k]) for k in ("p", "m", "v", "pb"))
