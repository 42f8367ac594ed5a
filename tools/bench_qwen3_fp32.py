"""First record of a Qwen3 decoder on the fp32 path (train_config.use_fp16=false, frozen decoder) at ``synthetic:qwen3-1.7b``:

  decode   ms per generated position at 16 utterances x 4 beams over 200 positions (bench.py's fp32 decode leg), with the q|k|v
           projection on the fused entry point (tasu_f32_gemm_qkv_norm_rope: head norm, rotation and cache append in the launch that
           sums the K-range slabs) and on the unfused route (tasu_f32_gemm_nt, then tasu_f32_qk_norm_rope), ALTERNATING in one process
           -- fused, unfused, fused, unfused after a warm-up run of each -- so that a drift of the box reaches both alike;
  train    ms per training step of 16 utterances x S = 256 through TasuEngine (eager launches: the fp32 step is not replayed);

each in ``--processes`` processes of its own, every process' figure reported next to the median.  The decode leg is timed by the host
clock around work that ends in a device synchronise, the step by device events around the timed steps.

    python tools/bench_qwen3_fp32.py [--processes 3] [--steps 3] [--new-tokens 200] [--model qwen3-1.7b] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_qwen3_fp32.py --child decode --new-tokens 50   # the per-kernel split
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_qwen3_fp32.py --child train --steps 1

Prints one JSON line: {"model", "decode_ms_per_position": {"fused": {"median", "runs"}, "unfused": {...}}, "train_step_ms": {...}}.
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
DIMS = {"qwen3-1.7b": 2048, "mid-qwen3": 256}


def build(model_name):
    from ps_slm_amd.config import ModelConfig, TrainConfig
    from ps_slm_amd.ps_slm import model_factory
    tc = TrainConfig(freeze_llm=True, freeze_encoder=True, gt_emb=True, gt_emb_noise=False, ctc_posterior=True, do_psd=True, use_fp16=False,
                     batching_strategy="dynamic")
    mc = ModelConfig(llm_path=f"synthetic:{model_name}", encoder_projector="linear-silu", llm_dim=DIMS[model_name],
                     **({"encoder_dim": 25055} if DIMS[model_name] != 256 else {}))
    model = model_factory(tc, mc, device="cuda:0", init_seed=1234, keep_logits=False, with_encoder=False)[0]
    assert model.core.arith == "fp32" and model.core.geo.qk_norm
    return model


def unfused_qkv(self, a, wqkv, bias, qkv, wq, wk, cos, sin, M, H, G, K, eps, ws, kc=None, vc=None, slot=None, ctx=0):
    """HipOps.f32_gemm_qkv_norm_rope as two entry points (the A/B route of this tool; the same bits)"""
    self.f32_gemm(a, wqkv, qkv, M, (H + 2 * G) * 128, K, bias=bias, ws=ws)
    self.f32_qk_norm_rope(qkv, wq, wk, cos, sin, qkv, None, M, H, G, eps, kc=kc, vc=vc, slot=slot, ctx=ctx)


def child_decode(model_name, batch, new_tokens, beams=4):
    import torch

    from ps_slm_amd.decode_fp32 import beam_search_generate_fp32
    from ps_slm_amd.ops import HipOps
    from ps_slm_amd.synthetic import synthetic_text_batch
    core = build(model_name).core
    raw = synthetic_text_batch(core.geo, batch, seed=1234, noise=False)
    ids = raw["input_ids"][:, :25]
    am = torch.ones_like(ids, dtype=torch.bool)
    fused = HipOps.f32_gemm_qkv_norm_rope

    def run(route):
        HipOps.f32_gemm_qkv_norm_rope = fused if route == "fused" else unfused_qkv
        core._dec_graphs.clear()                           # the captured positions hold the other route's launches
        st = core.prepare_text(ids, am, None, raw["post_ids"], None, None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = beam_search_generate_fp32(core, st, num_beams=beams, max_new_tokens=new_tokens, eos_token_id=-1, pad_token_id=0)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / int(out.shape[1]) * 1e3, out, int(st.S)

    ms = {"fused": [], "unfused": []}
    toks, S = {}, 0
    for route in ("fused", "unfused"):                     # warm-up: allocations, fragment-order copies, the first capture
        _, toks[route], S = run(route)
    assert torch.equal(toks["fused"], toks["unfused"])     # (the two routes give the same bits)
    for _ in range(2):
        for route in ("fused", "unfused"):
            ms[route].append(round(run(route)[0], 4))
    HipOps.f32_gemm_qkv_norm_rope = fused
    print("RESULT " + json.dumps(dict(fused_ms=min(ms["fused"]), unfused_ms=min(ms["unfused"]), fused_runs=ms["fused"], unfused_runs=ms["unfused"],
                                      utterances=batch, beams=beams, new_tokens=new_tokens, prefill_len=S)), flush=True)


def child_train(model_name, steps, warmup, batch):
    import torch

    from ps_slm_amd.config import DEFAULT_DS_CONFIG, load_ds_config
    from ps_slm_amd.engine import TasuEngine
    from ps_slm_amd.synthetic import synthetic_text_batch
    model = build(model_name)
    assert model.core.arith_train == "fp32"
    engine = TasuEngine(model, load_ds_config(DEFAULT_DS_CONFIG))
    engine.train()
    raw = synthetic_text_batch(model.core.geo, batch, seed=1234, noise=False)
    call = dict(input_ids=raw["input_ids"], attention_mask=raw["attention_mask"], labels=raw["labels"], input_features=None,
                input_feature_length=None, GT=[" ".join(map(str, p)) for p in raw["post_ids"]])

    def step():
        out, _ = engine(**call)
        engine.backward(out.loss)
        engine.step()
        return out

    for _ in range(warmup):                                # allocations, the transposed fp32 weight copies
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        out = step()
    e1.record()
    torch.cuda.synchronize()
    st = engine._last_state
    print("RESULT " + json.dumps(dict(step_ms=round(e0.elapsed_time(e1) / steps, 2), batch=batch, S=int(st.S), rows=int(st.M),
                                      loss=round(float(out.loss.detach()), 4))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--new-tokens", type=int, default=200)
    ap.add_argument("--model", default="qwen3-1.7b", choices=sorted(DIMS))
    ap.add_argument("--legs", default="decode,train")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=["train", "decode"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child == "train":
        return child_train(args.model, args.steps, args.warmup, args.batch)
    if args.child == "decode":
        return child_decode(args.model, args.batch, args.new_tokens)
    legs = [l for l in args.legs.split(",") if l]
    runs = {l: [] for l in legs}
    for _ in range(args.processes):
        for leg in legs:                                   # alternating: a drift of the box reaches both legs alike
            cmd = [sys.executable, os.path.abspath(__file__), "--model", args.model, "--steps", str(args.steps), "--warmup", str(args.warmup),
                   "--batch", str(args.batch), "--new-tokens", str(args.new_tokens), "--child", leg]
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            got = [l[len("RESULT "):] for l in res.stdout.splitlines() if l.startswith("RESULT ")]
            if res.returncode != 0 or not got:
                sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
                raise SystemExit(f"{leg}: the measuring process failed with code {res.returncode}")      # nothing further starts on the GPU
            runs[leg].append(json.loads(got[0]))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    rec = dict(model=args.model, processes=args.processes)
    if "decode" in runs:
        fu, un = [r["fused_ms"] for r in runs["decode"]], [r["unfused_ms"] for r in runs["decode"]]
        rec["decode_ms_per_position"] = dict(fused=dict(median=med(fu), runs=fu), unfused=dict(median=med(un), runs=un),
                                             spread_ms=round(max(max(fu) - min(fu), max(un) - min(un)), 4), config=runs["decode"][0])
    if "train" in runs:
        tr = [r["step_ms"] for r in runs["train"]]
        rec["train_step_ms"] = dict(median=med(tr), runs=tr, config=runs["train"][0])
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
