"""First record of a Qwen3 decoder on the bf16 path (train_config.use_fp16=true, frozen decoder): bench.py's synthetic text step (16
utterances x S = 256, hipGraph replay, fused AdamW through TasuEngine) and bench.py's decode leg (16 utterances x 4 beams, prefill
128, 200 generated positions) at ``synthetic:qwen3-1.7b``, each timed in a process of its own -- ``--processes`` of them, the
median reported next to every process' figure.  The step is timed by device events around the timed steps, the decode leg by
bench.decode_leg (host clock around work that ends in a device synchronise, second run).

    python tools/bench_qwen3.py [--processes 3] [--steps 20] [--warmup 3] [--model qwen3-1.7b] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_qwen3.py --child train --steps 5      # the per-kernel split
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_qwen3.py --child decode --new-tokens 50

Prints one JSON line: {"model", "train_step_ms": {"median", "runs"}, "decode_ms_per_position": {"median", "runs"}, ...}.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
DIMS = {"qwen3-1.7b": 2048, "qwen2.5-1.5b": 1536, "mid-qwen3": 256}


def build(model_name):
    from ps_slm_amd.config import ModelConfig, TrainConfig
    from ps_slm_amd.ps_slm import model_factory
    tc = TrainConfig(freeze_llm=True, freeze_encoder=True, gt_emb=True, gt_emb_noise=True, ctc_posterior=True, do_psd=True, use_fp16=True,
                     batching_strategy="dynamic")
    mc = ModelConfig(llm_path=f"synthetic:{model_name}", encoder_projector="linear-silu", encoder_dim=25055, llm_dim=DIMS[model_name])
    return model_factory(tc, mc, device="cuda:0", init_seed=1234, keep_logits=False, with_encoder=False)[0]


def child_train(model_name, steps, warmup, batch):
    import torch

    from ps_slm_amd.config import DEFAULT_DS_CONFIG, load_ds_config
    from ps_slm_amd.engine import TasuEngine
    from ps_slm_amd.synthetic import synthetic_text_batch
    model = build(model_name)
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
    rec = dict(step_ms=round(e0.elapsed_time(e1) / steps, 3), batch=batch, S=int(engine._last_state.S), rows=int(engine._last_state.M),
               labelled_rows=int(engine._last_state.nLp), loss=round(float(out.loss), 4))
    print("RESULT " + json.dumps(rec), flush=True)


def child_decode(model_name, batch, new_tokens):
    import bench
    from ps_slm_amd.synthetic import synthetic_text_batch
    model = build(model_name)
    raw = synthetic_text_batch(model.core.geo, batch, seed=1234, noise=False)
    print("RESULT " + json.dumps(bench.decode_leg(model.core, raw, batch, new_tokens=new_tokens)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--new-tokens", type=int, default=200)
    ap.add_argument("--model", default="qwen3-1.7b", choices=sorted(DIMS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=["train", "decode"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child == "train":
        return child_train(args.model, args.steps, args.warmup, args.batch)
    if args.child == "decode":
        return child_decode(args.model, args.batch, args.new_tokens)
    runs = {"train": [], "decode": []}
    for _ in range(args.processes):
        for leg in ("train", "decode"):                    # alternating: a drift of the box reaches both legs alike
            cmd = [sys.executable, os.path.abspath(__file__), "--model", args.model, "--steps", str(args.steps), "--warmup", str(args.warmup),
                   "--batch", str(args.batch), "--new-tokens", str(args.new_tokens), "--child", leg]
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            got = [l[len("RESULT "):] for l in res.stdout.splitlines() if l.startswith("RESULT ")]
            if res.returncode != 0 or not got:
                sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
                raise SystemExit(f"{leg}: the measuring process failed with code {res.returncode}")      # nothing further starts on the GPU
            runs[leg].append(json.loads(got[0]))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    tr, de = [r["step_ms"] for r in runs["train"]], [r["ms_per_step"] for r in runs["decode"]]
    rec = dict(model=args.model, processes=args.processes, train_step_ms=dict(median=med(tr), runs=tr),
               decode_ms_per_position=dict(median=med(de), runs=de), train=runs["train"][0], decode=runs["decode"][0])
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
