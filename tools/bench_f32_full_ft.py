"""Full fine-tuning of the LLM on the fp32 training step (train_config.freeze_llm=false, use_fp16=false), measured on the GPU:

  1. per decoder shape at Qwen2.5-1.5B (16 x 256 token rows): tasu_f32_gemm_tn (csrc/wgrad_f32.hip: dW = dY^T X from the row-major
     fp32 operands) against the composed route -- two tasu_f32_transpose + tasu_f32_gemm_nt, what the projector's weight gradients
     run -- the routes alternated inside one process on COLD ROTATING operands (each call reads another copy of dY / X; the copies
     together exceed the 256 MB of last-level cache), timed by device events; plus tasu_f32_rmsnorm_wgrad and the two column sums;
  2. the whole step (forward, backward, AdamW, refresh) at 16 x 256 with the decoder frozen and fully trainable, each in a process
     of its own, with the per-step refresh of the working copies (the fp32 transposed copies of the dgrads among them), AdamW over the
     bucket and the device memory in use.

    python tools/bench_f32_full_ft.py [--steps 5] [--warmup 2] [--reps 4] [--rounds 3] [--only shapes|step]

One JSON line per shape and per configuration.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# (what, R, N, K): dW [N, K] = dY [R, N]^T X [R, K]; the fp32 step forms the head term over all 4096 rows
SHAPES = [("q|k|v", 4096, 2048, 1536), ("o", 4096, 1536, 1536), ("gate|up", 4096, 17920, 1536), ("down", 4096, 1536, 8960),
          ("lm_head", 4096, 151936, 1536)]
F32_PEAK_TFLOPS = 157.3                                  # MI355X dense fp32 MFMA peak
COLD_BYTES = 512 << 20                                   # operand copies per shape: at least twice the last-level cache


def shapes(reps, rounds):
    import torch

    from ps_slm_amd.ops import RMS_WGRAD_SPLIT, HipOps
    ops = HipOps()

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n              # us

    for what, R, N, K in SHAPES:
        sets = max(2, min(8, -(-COLD_BYTES // (4 * R * (N + K)))))
        As = [torch.randn(R, N, device="cuda") for _ in range(sets)]
        Bs = [torch.randn(R, K, device="cuda") for _ in range(sets)]
        Rp = (R + 31) // 32 * 32
        a_t, b_t = torch.empty(N, Rp, device="cuda"), torch.empty(K, Rp, device="cuda")
        c_new, c_old = torch.empty(N, K, device="cuda"), torch.empty(N, K, device="cuda")
        nsplit = ops.f32_gemm_tn_split(R, N, K)
        ws = torch.empty(nsplit * N * K, device="cuda") if nsplit > 1 else None
        gws = torch.empty(max(16 * 128 * 4096, 2 * 64 * 151936), device="cuda")      # decode_fp32._gemm_ws

        def tn(i):
            ops.f32_gemm_tn(As[i % sets], Bs[i % sets], c_new, R, N, K, nsplit=nsplit, ws=ws)

        def composed(i):
            ops.f32_transpose(As[i % sets], a_t, R, N, Rp)
            ops.f32_transpose(Bs[i % sets], b_t, R, K, Rp)
            ops.f32_gemm(a_t, b_t, c_old, N, K, Rp, ws=gws)

        routes = {"tn": tn, "composed": composed}
        for fn in routes.values():                       # warm every route at this shape
            fn(0), fn(1)
        torch.cuda.synchronize()
        us = {k: [] for k in routes}
        for _ in range(rounds):                          # alternate the routes
            for k, fn in routes.items():
                us[k].append(timed(fn, reps))
        tn(0), composed(0)
        torch.cuda.synchronize()
        diff = float((c_new - c_old).abs().max() / c_old.abs().max())
        best = {k: min(v) for k, v in us.items()}
        flop = 2.0 * R * N * K
        print(json.dumps({"shape": what, "R": R, "N": N, "K": K, "nsplit": nsplit, "operand_sets": sets,
                          "us": {k: [round(x, 1) for x in v] for k, v in us.items()},
                          "tn_tflops": round(flop / best["tn"] / 1e6, 1), "tn_share_of_fp32_peak": round(flop / best["tn"] / 1e6 / F32_PEAK_TFLOPS, 3),
                          "composed_tflops": round(flop / best["composed"] / 1e6, 1), "faster": min(best, key=best.get),
                          "max_rel_diff": diff}), flush=True)
        del As, Bs, a_t, b_t, c_new, c_old, ws, gws
        torch.cuda.empty_cache()
    # the row-wise reductions at 4096 rows: the norm weights (reads dy and x once), the q|k|v bias by both column sums
    R, D, C = 4096, 1536, 2048
    sets = 8
    dys, xs = [torch.randn(R, D, device="cuda") for _ in range(sets)], [torch.randn(R, D, device="cuda") for _ in range(sets)]
    qs = [torch.randn(R, C, device="cuda") for _ in range(sets)]
    dw, out = torch.empty(D, device="cuda"), torch.empty(C, device="cuda")
    ws = torch.empty(RMS_WGRAD_SPLIT * C + R, device="cuda")
    fns = {"rmsnorm_wgrad": lambda i: ops.f32_rmsnorm_wgrad(dys[i % sets], xs[i % sets], dw, ws, 1e-6),
           "colsum_split": lambda i: ops.f32_colsum_split(qs[i % sets], out, ws, R, C),
           "colsum_one_pass": lambda i: ops.f32_colsum(qs[i % sets], out, R, C)}
    for name, fn in fns.items():
        fn(0), fn(1)
        torch.cuda.synchronize()
        t = [timed(fn, 4 * reps) for _ in range(rounds)]
        print(json.dumps({"shape": name, "R": R, "columns": D if name == "rmsnorm_wgrad" else C, "us": [round(v, 1) for v in t]}), flush=True)


def step_child(full_ft, steps, warmup, batch):
    import torch

    from ps_slm_amd.config import DEFAULT_DS_CONFIG, ModelConfig, TrainConfig, load_ds_config
    from ps_slm_amd.engine import TasuEngine
    from ps_slm_amd.ps_slm import model_factory
    from ps_slm_amd.synthetic import synthetic_text_batch

    tc = TrainConfig(freeze_llm=not full_ft, freeze_encoder=True, gt_emb=True, gt_emb_noise=True, ctc_posterior=True, do_psd=True,
                     use_fp16=False, batching_strategy="dynamic")
    mc = ModelConfig(llm_path="synthetic:qwen2.5-1.5b", encoder_projector="linear-silu", encoder_dim=25055, llm_dim=1536)
    model, _ = model_factory(tc, mc, device="cuda:0", init_seed=1234, keep_logits=False)
    model.drop_prob = 0.0
    core = model.core
    assert core.arith_train == "fp32" and (core.full_ft is not None) == bool(full_ft)
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
    st = model.last_state
    rec = dict(model="qwen2.5-1.5b", arith="fp32", full_ft=bool(full_ft), step_ms=round(e0.elapsed_time(e1) / steps, 2), batch=batch,
               S=int(st.S), rows=int(st.M), bucket_elements=int(pr.numel), device_gb=round((total - free) / 2 ** 30, 2),
               torch_peak_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))

    def timed(fn, reps=5):
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return round(sorted(ms)[len(ms) // 2], 3)

    c = engine.cfg
    split = {"refresh": timed(core.refresh_working_copies)}
    split["adamw_bucket"] = timed(lambda: core.ops.adamw(pr.p, pr.g, pr.m, pr.v, pr.pb, 0.0, c["betas"][0], c["betas"][1], c["eps"],
                                                         c["weight_decay"], 1, 1.0))
    rec["split_ms"] = split
    print("RESULT " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None, choices=("shapes", "step"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child == "shapes":
        return shapes(args.reps, args.rounds)
    if args.child in ("0", "1"):
        return step_child(args.child == "1", args.steps, args.warmup, args.batch)
    jobs = ([] if args.only == "step" else ["shapes"]) + ([] if args.only == "shapes" else ["0", "1"])
    for job in jobs:                                     # every measurement in a process of its own, one after the other
        cmd = [sys.executable, os.path.abspath(__file__), "--steps", str(args.steps), "--warmup", str(args.warmup), "--batch", str(args.batch),
               "--reps", str(args.reps), "--rounds", str(args.rounds), "--child", job]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        lines = [l for l in res.stdout.splitlines() if l.startswith("{") or l.startswith("RESULT ")]
        for l in lines:
            print(l[len("RESULT "):] if l.startswith("RESULT ") else l, flush=True)
        if res.returncode != 0 or not lines:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit(f"{job}: the measuring process failed with code {res.returncode}")   # nothing further starts on the GPU


if __name__ == "__main__":
    main()
