"""Step cost of train_config.use_emb: the LoRA step of bench.py's LoRA leg (text-only recipe, 16 utterances x S = 256, use_peft=true
with the reference's defaults r = 64 / alpha = 16 / dropout 0.05 on all seven Linears, hipGraph replay of the forward, fused AdamW)
timed with and without use_emb, at Qwen2.5-1.5B (tied head) and Qwen2.5-7B (untied head), plus the per-kernel split of the work
use_emb adds.  Every configuration runs in a process of its own (a fresh allocator and HIP runtime each time).

    python tools/bench_use_emb.py [--steps 20] [--warmup 3] [--models qwen2.5-1.5b,qwen2.5-7b] [--out FILE]

Prints one JSON line per configuration: {"model", "use_emb", "step_ms", "table_elements", "split_ms": {...}}.  split_ms (use_emb
only; eager launches between event pairs, median of 10): head_wgrad = the two operand transposes + dW = dlogits^T h (tied only),
lookup = the zero fill (untied only) + tasu_embed_bwd, adamw_table = the fused AdamW over the table's range, refresh = what
TasuModel._embed_changed() does after the step (tied: the [D, Vpad] transpose of the head).
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def child(model_name, use_emb, steps, warmup, batch):
    import torch

    from ps_slm_amd.config import DEFAULT_DS_CONFIG, ModelConfig, TrainConfig, load_ds_config
    from ps_slm_amd.engine import TasuEngine
    from ps_slm_amd.ps_slm import model_factory
    from ps_slm_amd.synthetic import synthetic_text_batch

    tc = TrainConfig(freeze_llm=True, freeze_encoder=True, gt_emb=True, gt_emb_noise=True, ctc_posterior=True, do_psd=True,
                     use_fp16=True, batching_strategy="dynamic")
    tc.use_peft, tc.use_emb = True, bool(use_emb)
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
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    rec = dict(model=model_name, use_emb=bool(use_emb), step_ms=round((time.perf_counter() - t0) / steps * 1e3, 3),
               batch=batch, S=int(engine._last_state.S), labelled_rows=int(engine._last_state.nLp),
               table_elements=core.geo.llm_vocab * core.geo.llm_dim if use_emb else 0)
    if use_emb:
        st, pr, c = engine._last_state, core.proj, engine.cfg
        lo, hi = core.embed_range

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

        core.use_graphs = False
        out, _ = engine(**call)                            # an eager forward: the operands of the backward pieces are in place
        engine.backward(out.loss)
        st = engine._last_state
        split = {}
        if core.geo.tied:
            split["head_wgrad"] = timed(lambda: core._head_wgrad(st))
        split["lookup"] = timed(lambda: core.backward_embed(st))
        split["adamw_table"] = timed(lambda: core.ops.adamw(pr.p[lo:hi], pr.g[lo:hi], pr.m[lo:hi], pr.v[lo:hi], pr.pb[lo:hi], 0.0, c["betas"][0],
                                                            c["betas"][1], c["eps"], c["weight_decay"], 1, 1.0))
        split["refresh"] = timed(core._embed_changed)
        rec["split_ms"] = split
    print("RESULT " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--models", default="qwen2.5-1.5b,qwen2.5-7b")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=2, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1] == "1", args.steps, args.warmup, args.batch)
    lines = []
    for name in args.models.split(","):
        for use_emb in (0, 1):
            cmd = [sys.executable, os.path.abspath(__file__), "--steps", str(args.steps), "--warmup", str(args.warmup), "--batch", str(args.batch),
                   "--child", name, str(use_emb)]
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            got = [l[len("RESULT "):] for l in res.stdout.splitlines() if l.startswith("RESULT ")]
            if res.returncode != 0 or not got:
                sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
                raise SystemExit(f"{name} use_emb={use_emb}: the measuring process failed with code {res.returncode}")   # nothing further starts on the GPU
            print(got[0], flush=True)
            lines.append(got[0])
            if args.out:
                with open(args.out, "w") as f:
                    f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
