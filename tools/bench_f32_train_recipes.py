"""The fp32 training step (train_config.use_fp16 = false, mixed_precision = false: ps_slm_amd/train_fp32.py) of the alternate
projectors and of an adapted decoder at Qwen2.5-1.5B, 16 utterances, through TasuEngine like bench.py's fp32 leg (271 ms for
linear-silu without adapters).

    python tools/bench_f32_train_recipes.py [lora cross-attention cov1d-linear linear linear-silu]

``lora``: linear-silu with the reference's PeftConfig (r = 64, dropout 0.05, all seven Linears).  One JSON line per recipe: ms per
step and the peak HBM allocation (clean for the FIRST recipe of a run only: run one recipe per process for that figure)."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def time_step(kind, B=16, steps=3):
    use_peft, projector = kind == "lora", "linear-silu" if kind == "lora" else kind
    from ps_slm_amd.config import DEFAULT_DS_CONFIG, ModelConfig, TrainConfig, load_ds_config
    from ps_slm_amd.engine import TasuEngine
    from ps_slm_amd.ps_slm import model_factory
    from ps_slm_amd.synthetic import synthetic_text_batch
    tc = TrainConfig(freeze_llm=True, freeze_encoder=True, gt_emb=True, gt_emb_noise=False, ctc_posterior=True, do_psd=True, use_fp16=False,
                     mixed_precision=False, use_peft=use_peft, batching_strategy="dynamic")
    extra = dict(encoder_projector_ds_rate=2) if projector in ("linear", "cov1d-linear") else {}
    mc = ModelConfig(llm_path="synthetic:qwen2.5-1.5b", encoder_projector=projector, encoder_dim=25055, llm_dim=1536, **extra)
    torch.cuda.reset_peak_memory_stats()
    model, _ = model_factory(tc, mc, device="cuda:0", init_seed=1234, keep_logits=False, with_encoder=False)
    assert model.core.arith_train == "fp32"
    if use_peft:                                            # non-zero B: every product of the adapters' backward does work
        from ps_slm_amd.synthetic import random_lora_state_dict
        model.core.lora.load_state_dict(random_lora_state_dict(model.core.geo, model.core.lora.cfg, 7, b_scale=0.01))
        model.core.sync_projector_copies()
    eng = TasuEngine(model, load_ds_config(DEFAULT_DS_CONFIG))
    eng.train()
    raw = synthetic_text_batch(model.core.geo, B, seed=1234, noise=False)
    batch = dict(input_ids=raw["input_ids"], attention_mask=raw["attention_mask"], labels=raw["labels"], input_features=None,
                 input_feature_length=None, GT=[" ".join(map(str, p)) for p in raw["post_ids"]])

    def step():
        out, _ = eng(**batch)
        eng.backward(out.loss)
        eng.step()
        return out

    step()                                                  # warm-up: allocations, the transposed fp32 weight copies
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    st = eng._last_state
    rec = {"fp32_training_step": kind, "utterances": B, "seq_len": st.S, "projector_rows": st.Rap, "ms_per_step": round(dt * 1e3, 2),
           "peak_hbm_gb": round(torch.cuda.max_memory_allocated() / 1e9, 2), "final_loss": round(float(out.loss.detach()), 4)}
    eng.destroy()
    del eng, model
    import gc
    gc.collect()
    torch.cuda.empty_cache()
    return rec


if __name__ == "__main__":
    for kind in (sys.argv[1:] or ["lora", "cross-attention", "cov1d-linear"]):
        print(json.dumps(time_step(kind)), flush=True)
