"""Step cost of full fine-tuning of the LLM (train_config.freeze_llm=false, use_fp16=true): bench.py's synthetic text step (16
utterances x S = 256, hipGraph replay, fused AdamW) with the decoder frozen (the shipped recipe) and fully trainable, each in a
process of its own, warmed, timed by device events around the timed steps; for the trainable model also the cost of the parts
that exist only there -- AdamW over the whole bucket (about 30 bytes of traffic per element: p, g, m, v read, p, m, v and the bf16
image written), the working-copy refresh after the step -- and the device memory in use.

    python tools/bench_full_ft.py [--steps 20] [--warmup 3] [--models qwen2.5-1.5b] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_full_ft.py --child qwen2.5-1.5b 1 --steps 5     # the per-kernel split

Prints one JSON line per configuration: {"model", "full_ft", "step_ms", "bucket_elements", "device_gb", "split_ms": {...}}.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def child(model_name, full_ft, steps, warmup, batch):
    import torch

    from ps_slm_amd.config import DEFAULT_DS_CONFIG, ModelConfig, TrainConfig, load_ds_config
    from ps_slm_amd.engine import TasuEngine
    from ps_slm_amd.ps_slm import model_factory
    from ps_slm_amd.synthetic import synthetic_text_batch

    tc = TrainConfig(freeze_llm=not full_ft, freeze_encoder=True, gt_emb=True, gt_emb_noise=True, ctc_posterior=True, do_psd=True,
                     use_fp16=True, batching_strategy="dynamic")
    mc = ModelConfig(llm_path=f"synthetic:{model_name}", encoder_projector="linear-silu", encoder_dim=25055,
                     llm_dim={"qwen2.5-1.5b": 1536, "qwen2.5-7b": 3584, "mid": 256}[model_name])
    model, _ = model_factory(tc, mc, device="cuda:0", init_seed=1234, keep_logits=False)
    model.drop_prob = 0.0
    core = model.core
    core.use_graphs = True
    engine = TasuEngine(model, load_ds_config(DEFAULT_DS_CONFIG))
    engine.train()
    raw = synthetic_text_batch(core.geo, batch, seed=1234, noise=False)
    call = dict(input_ids=raw["input_ids"], attention_mask=raw["attention_mask"], labels=raw["labels"], input_features=None,
                input_feature_length=None, GT=[" ".join(map(str, p)) for p in raw["post_ids"]])
    torch.manual_seed(1234)

    def step():
        out, _ = engine(**call)
        engine.backward(out.loss)
        engine.step()

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    pr = core.proj
    rec = dict(model=model_name, full_ft=bool(full_ft), step_ms=round(e0.elapsed_time(e1) / steps, 3), batch=batch,
               S=int(engine._last_state.S), rows=int(engine._last_state.M), labelled_rows=int(engine._last_state.nLp),
               bucket_elements=int(pr.numel), device_gb=round((total - free) / 2 ** 30, 2),
               torch_peak_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))
    if full_ft:
        c = engine.cfg

        def timed(fn, reps=10):
            ms = []
            for _ in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                ms.append(a.elapsed_time(b))
            return round(sorted(ms)[len(ms) // 2], 3)

        split = {}
        split["adamw_bucket"] = timed(lambda: core.ops.adamw(pr.p, pr.g, pr.m, pr.v, pr.pb, 0.0, c["betas"][0], c["betas"][1], c["eps"],
                                                             c["weight_decay"], 1, 1.0))
        split["adamw_GBps_at_30B_per_element"] = round(30.0 * pr.numel / split["adamw_bucket"] / 1e6, 1)
        split["refresh"] = timed(core.refresh_working_copies)
        rec["split_ms"] = split
    print("RESULT " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--models", default="qwen2.5-1.5b")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=2, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1] == "1", args.steps, args.warmup, args.batch)
    lines = []
    for name in args.models.split(","):
        for full_ft in (0, 1):
            cmd = [sys.executable, os.path.abspath(__file__), "--steps", str(args.steps), "--warmup", str(args.warmup), "--batch", str(args.batch),
                   "--child", name, str(full_ft)]
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            got = [l[len("RESULT "):] for l in res.stdout.splitlines() if l.startswith("RESULT ")]
            if res.returncode != 0 or not got:
                sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
                raise SystemExit(f"{name} full_ft={full_ft}: the measuring process failed with code {res.returncode}")   # nothing further starts on the GPU
            print(got[0], flush=True)
            lines.append(got[0])
            if args.out:
                with open(args.out, "w") as f:
                    f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
