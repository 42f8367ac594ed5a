"""First record of full fine-tuning of a Qwen3 decoder (train_config.freeze_llm=false on ``synthetic:qwen3-1.7b``): bench.py's synthetic
text step (16 utterances x S = 256, fused AdamW through TasuEngine) on the bf16-autocast step (use_fp16=true, hipGraph replay) and on
the fp32 step (use_fp16=false, launched eagerly), each figure from ``--processes`` processes of its own, the median reported next
to every process' figure, with the device memory in use.  The step is timed by device events around the timed steps.

    python tools/bench_qwen3_full_ft.py [--processes 3] [--steps 10] [--warmup 3] [--model qwen3-1.7b] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_qwen3_full_ft.py --child bf16 --steps 5
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_qwen3_full_ft.py --child fp32 --steps 3
(the per-kernel split: qk_norm_wgrad_part_kernel / f32_qk_norm_wgrad_part_kernel and qk_norm_wgrad_sum_kernel run once per layer and
step)

Prints one JSON line: {"model", "bf16": {"step_ms": {"median", "runs"}, "device_gb", ...}, "fp32": {...}}.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
DIMS = {"qwen3-1.7b": 2048, "mid-qwen3": 256}


def child(model_name, arith, steps, warmup, batch):
    import torch

    from ps_slm_amd.config import DEFAULT_DS_CONFIG, ModelConfig, TrainConfig, load_ds_config
    from ps_slm_amd.engine import TasuEngine
    from ps_slm_amd.ps_slm import model_factory
    from ps_slm_amd.synthetic import synthetic_text_batch

    tc = TrainConfig(freeze_llm=False, freeze_encoder=True, gt_emb=True, gt_emb_noise=True, ctc_posterior=True, do_psd=True,
                     use_fp16=arith == "bf16", batching_strategy="dynamic")
    mc = ModelConfig(llm_path=f"synthetic:{model_name}", encoder_projector="linear-silu", encoder_dim=25055, llm_dim=DIMS[model_name])
    model, _ = model_factory(tc, mc, device="cuda:0", init_seed=1234, keep_logits=False, with_encoder=False)
    model.drop_prob = 0.0
    core = model.core
    assert core.full_ft is not None and core.geo.qk_norm and core.arith_train == arith
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
        return out

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        out = step()
    e1.record()
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    rec = dict(arith=arith, step_ms=round(e0.elapsed_time(e1) / steps, 3), batch=batch, S=int(engine._last_state.S),
               rows=int(engine._last_state.M), labelled_rows=int(engine._last_state.nLp), loss=round(float(out.loss), 4),
               bucket_elements=int(core.proj.numel), device_gb=round((total - free) / 2 ** 30, 2),
               torch_peak_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))
    print("RESULT " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--model", default="qwen3-1.7b", choices=sorted(DIMS))
    ap.add_argument("--arith", default="bf16,fp32")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=["bf16", "fp32"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.model, args.child, args.steps, args.warmup, args.batch)
    legs = args.arith.split(",")
    runs = {leg: [] for leg in legs}
    for _ in range(args.processes):
        for leg in legs:                                   # alternating: a drift of the box reaches both legs alike
            cmd = [sys.executable, os.path.abspath(__file__), "--model", args.model, "--steps", str(args.steps), "--warmup", str(args.warmup),
                   "--batch", str(args.batch), "--child", leg]
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            got = [l[len("RESULT "):] for l in res.stdout.splitlines() if l.startswith("RESULT ")]
            if res.returncode != 0 or not got:
                sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
                raise SystemExit(f"{leg}: the measuring process failed with code {res.returncode}")      # nothing further starts on the GPU
            runs[leg].append(json.loads(got[0]))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    rec = dict(model=args.model, processes=args.processes)
    for leg in legs:
        ms = [r["step_ms"] for r in runs[leg]]
        rec[leg] = dict(runs[leg][0], step_ms=dict(median=med(ms), runs=ms))
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
