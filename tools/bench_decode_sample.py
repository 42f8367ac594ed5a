"""What generate(do_sample=True, num_beams=1) costs per generated position: Qwen2.5-1.5B geometry, 16 utterances, ONE beam, a
25-position prompt, 200 forced positions (an EOS id that never matches), bf16 arithmetic (``--arith fp32`` for the other).

Greedy (do_sample=False) and sampled (top_k = 50, top_p = 0.9, T = 1.0) decodes run in the same process on the same build,
alternating, after one warm-up run of each (the warm-up captures the position's graph: the sampling knobs are part of the graph
key).  ``--processes N`` repeats that in N fresh child processes, one after the other: the spread between processes is what a
difference has to exceed.  Timed region as in bench.py's decode leg: prefill + the whole decode loop, host clock around a device
synchronise.  ``--greedy-only`` times the greedy decode alone and touches nothing of the sampling interface, so the same file
measures an older checkout at the same shape on the same box.

``--launches`` times the launches the two positions differ in, alone, with device events over 200 back-to-back repetitions on random
logits [16, 151936]: tasu_logprob_topk (k = 2) against tasu_sample_uniform + tasu_sample_rows.

    python tools/bench_decode_sample.py [--runs 3] [--processes 3] [--arith bf16] [--greedy-only] [--launches]"""
import argparse
import gc
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOP_K, TOP_P, TEMPERATURE = 50, 0.9, 1.0


def leg(arith, runs, greedy_only, B=16, new_tokens=200):
    from ps_slm_amd.config import ModelConfig, TrainConfig
    from ps_slm_amd.decode import beam_search_generate
    from ps_slm_amd.decode_fp32 import beam_search_generate_fp32
    from ps_slm_amd.ps_slm import model_factory
    from ps_slm_amd.synthetic import synthetic_text_batch

    tc = TrainConfig(freeze_llm=True, freeze_encoder=True, gt_emb=True, gt_emb_noise=False, ctc_posterior=True, do_psd=True,
                     use_fp16=arith == "bf16", batching_strategy="dynamic")
    mc = ModelConfig(llm_path="synthetic:qwen2.5-1.5b", encoder_projector="linear-silu", encoder_dim=25055, llm_dim=1536)
    model, _ = model_factory(tc, mc, device="cuda:0", init_seed=1234, keep_logits=False, with_encoder=False)
    core = model.core
    raw = synthetic_text_batch(core.geo, B, seed=1234, noise=False)
    ids = raw["input_ids"][:, :25]
    am = torch.ones_like(ids, dtype=torch.bool)

    def run(sampled):
        kw = {}
        if sampled:
            from ps_slm_amd.decode import check_sampling
            kw["sampling"] = check_sampling(TEMPERATURE, TOP_K, TOP_P)
            torch.manual_seed(4321)                                    # the same draws every run
        st = core.prepare_text(ids, am, None, raw["post_ids"], None, None)
        if arith == "fp32":
            return beam_search_generate_fp32(core, st, num_beams=1, max_new_tokens=new_tokens, eos_token_id=-1, pad_token_id=0, **kw)
        core.forward_projector_text(st)
        return beam_search_generate(core, st, num_beams=1, max_new_tokens=new_tokens, eos_token_id=-1, pad_token_id=0, **kw)

    def timed(sampled):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = run(sampled)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / int(out.shape[1]), out

    modes = (False,) if greedy_only else (False, True)
    outs = {m: run(m) for m in modes}                                 # warm-up: every shape and both graphs
    ms = {m: [] for m in modes}
    for _ in range(runs):
        for m in modes:
            t, out = timed(m)
            assert torch.equal(out, outs[m])                           # the same tokens every run
            ms[m].append(round(t, 4))
    rec = {"arith": arith, "utterances": B, "beams": 1, "new_tokens": int(outs[False].shape[1]), "ms_per_position_greedy": ms[False]}
    if not greedy_only:
        rec.update({"ms_per_position_sampled": ms[True], "top_k": TOP_K, "top_p": TOP_P,
                    "median_difference_us": round((statistics.median(ms[True]) - statistics.median(ms[False])) * 1e3, 1),
                    "tokens_differ": not torch.equal(outs[False], outs[True])})
    core._dec_graphs.clear()
    del model, core
    gc.collect()
    torch.cuda.empty_cache()
    return rec


def launches(M=16, V=151936, reps=200):
    """us per launch set, device events around ``reps`` back-to-back repetitions (the logits stay in L2 / the Infinity Cache, as they
    do behind the lm_head GEMM that has just written them)."""
    from ps_slm_amd.ops import HipOps
    ops = HipOps()
    g = torch.Generator().manual_seed(1)
    lg = (torch.randn(M, V, generator=g) * 2.5).to(torch.bfloat16).cuda()
    val, idx = torch.zeros(M, 2, device="cuda"), torch.zeros(M, 2, dtype=torch.int32, device="cuda")
    ban = torch.tensor([-1], dtype=torch.int32, device="cuda")
    seed, ctl = torch.tensor([99], dtype=torch.int64, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    u = torch.zeros(M, device="cuda")

    def topk():
        ops.logprob_topk(lg, M, V, 2, ban, 1, val, idx)

    def sample(top_k=TOP_K, top_p=TOP_P):
        ops.sample_uniform(seed, ctl, M, u)
        ops.sample_rows(lg, M, V, u, ban, 1, None, None, 1.0, TEMPERATURE, top_k, top_p, val, idx)

    def us(fn):
        for _ in range(10):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return round(a.elapsed_time(b) * 1e3 / reps, 2)

    return {"rows": M, "vocab": V, "logprob_topk_k2_us": [us(topk) for _ in range(3)], "uniform_plus_sample_rows_us": [us(sample) for _ in range(3)],
            "uniform_plus_sample_rows_top_k_1024_us": [us(lambda: sample(1024, 1.0)) for _ in range(3)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--processes", type=int, default=1)
    ap.add_argument("--arith", default="bf16")
    ap.add_argument("--greedy-only", action="store_true")
    ap.add_argument("--launches", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode_sample.py measures on the GPU: no device found")
    if args.launches:
        print(json.dumps({"decode_sample_launches": launches()}))
        return
    if args.processes > 1:                                             # fresh child processes, one after the other
        recs = []
        for _ in range(args.processes):
            cmd = [sys.executable, os.path.abspath(__file__), "--runs", str(args.runs), "--arith", args.arith] + (["--greedy-only"] if args.greedy_only else [])
            out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout
            recs.append(json.loads(out.strip().splitlines()[-1])["decode_sample"][0])
        print(json.dumps({"decode_sample_processes": recs}))
        return
    print(json.dumps({"decode_sample": [leg(a, args.runs, args.greedy_only) for a in args.arith.split(",")]}))


if __name__ == "__main__":
    main()
