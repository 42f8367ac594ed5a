"""What generate(do_sample=True, num_beams > 1) costs per generated position: Qwen2.5-1.5B geometry, ``--shapes`` utterances x beams
(default 16x4 and 4x16: 64 beam rows each), a 25-position prompt, 200 forced positions (an EOS id that never matches), bf16 arithmetic
(``--arith fp32`` for the other).

Beam search (do_sample=False) and beam-sample (top_k = 50, top_p = 0.9, T = 1.0) decodes run in the same process on the same build,
alternating, after one warm-up run of each (the warm-up captures the position's graph: the sampling knobs are part of the graph
key).  ``--processes N`` repeats that in N fresh child processes, one after the other: the spread between processes is what a
difference has to exceed.  Timed region as in bench.py's decode leg: prefill + the whole decode loop, host clock around a device
synchronise.  ``--search-only`` times the beam search alone and touches nothing of the sampling interface, so the same file measures an
older checkout at the same shapes on the same box.

``--launches`` times the launches the two positions differ in, alone, with device events over 200 back-to-back repetitions on random
logits [64, 151936]: tasu_logprob_topk (k = 2 nb) + tasu_beam_update against tasu_beam_sample_rows + tasu_beam_update_drawn.

    python tools/bench_decode_beam_sample.py [--runs 3] [--processes 3] [--arith bf16] [--shapes 16x4,4x16] [--search-only] [--launches]"""
import argparse
import gc
import json
import os
import statistics
import subprocess
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOP_K, TOP_P, TEMPERATURE = 50, 0.9, 1.0


def leg(arith, runs, search_only, shapes, new_tokens=200):
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
    recs = []
    for B, nb in shapes:
        raw = synthetic_text_batch(core.geo, B, seed=1234, noise=False)
        ids = raw["input_ids"][:, :25]
        am = torch.ones_like(ids, dtype=torch.bool)

        def run(sampled):
            kw = {}
            if sampled:
                from ps_slm_amd.decode import check_sampling
                kw["sampling"] = check_sampling(TEMPERATURE, TOP_K, TOP_P)
                torch.manual_seed(4321)                                # the same draws every run
            st = core.prepare_text(ids, am, None, raw["post_ids"], None, None)
            if arith == "fp32":
                return beam_search_generate_fp32(core, st, num_beams=nb, max_new_tokens=new_tokens, eos_token_id=-1, pad_token_id=0, **kw)
            core.forward_projector_text(st)
            return beam_search_generate(core, st, num_beams=nb, max_new_tokens=new_tokens, eos_token_id=-1, pad_token_id=0, **kw)

        def timed(sampled):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = run(sampled)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / int(out.shape[1]), out

        modes = (False,) if search_only else (False, True)
        outs = {m: run(m) for m in modes}                             # warm-up: every shape and both graphs
        ms = {m: [] for m in modes}
        for _ in range(runs):
            for m in modes:
                t, out = timed(m)
                assert torch.equal(out, outs[m])                       # the same tokens every run
                ms[m].append(round(t, 4))
        rec = {"arith": arith, "utterances": B, "beams": nb, "new_tokens": int(outs[False].shape[1]), "ms_per_position_search": ms[False]}
        if not search_only:
            rec.update({"ms_per_position_beam_sample": ms[True], "top_k": TOP_K, "top_p": TOP_P,
                        "median_difference_us": round((statistics.median(ms[True]) - statistics.median(ms[False])) * 1e3, 1),
                        "tokens_differ": not torch.equal(outs[False], outs[True])})
        recs.append(rec)
        core._dec_graphs.clear()
    del model, core
    gc.collect()
    torch.cuda.empty_cache()
    return recs


def launches(shapes, V=151936, reps=200):
    """us per launch set, device events around ``reps`` back-to-back repetitions (the logits stay in L2 / the Infinity Cache, as they
    do behind the lm_head GEMM that has just written them).  The update launches run on a state whose done flag is clear and whose
    position is put back to 0 before every repetition set."""
    from ps_slm_amd.decode import DeviceBeam, check_sampling
    from ps_slm_amd.model import Geometry, TasuModel
    from ps_slm_amd.ops import HipOps
    from ps_slm_amd.synthetic import MID_GEOMETRY
    ops = HipOps()
    model = TasuModel(Geometry.from_dict(dict(MID_GEOMETRY, llm_layers=0)), ops, "cuda")
    out = []
    for B, nb in shapes:
        M, K = B * nb, 2 * nb
        g = torch.Generator().manual_seed(1)
        lg = (torch.randn(M, V, generator=g) * 2.5).to(torch.bfloat16).cuda()
        key, val = torch.zeros(M, K, device="cuda"), torch.zeros(M, K, device="cuda")
        idx = torch.zeros(M, K, dtype=torch.int32, device="cuda")
        bs = DeviceBeam(model, B, nb, reps + 16, -1, 1.0, 0, 25, [25] * B, 1.0, check_sampling(TEMPERATURE, TOP_K, TOP_P))
        rows = types.SimpleNamespace(nb=nb, seed=bs.seed, ctl=torch.zeros(2, dtype=torch.int32, device="cuda"), run_scores=bs.run_scores,
                                     banned=torch.tensor([-1], dtype=torch.int32, device="cuda"), hist=None, hist_len=None, penalty=1.0)
        ban = rows.banned

        def us(fn):
            bs.ctl.zero_()
            for _ in range(10):
                fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            assert int(bs.ctl[1]) == 0
            return round(a.elapsed_time(b) * 1e3 / reps, 2)

        out.append({"utterances": B, "beams": nb, "rows": M, "vocab": V,
                    "logprob_topk_us": [us(lambda: ops.logprob_topk(lg, M, V, K, ban, 1, val, idx)) for _ in range(3)],
                    "beam_sample_rows_us": [us(lambda: ops.beam_sample_rows(lg, M, V, K, False, rows, 1, TEMPERATURE, TOP_K, TOP_P, key, val, idx))
                                            for _ in range(3)],
                    "beam_update_us": [us(lambda: ops.beam_update(val, idx, bs, False)) for _ in range(3)],
                    "beam_update_drawn_us": [us(lambda: ops.beam_update_drawn(key, val, idx, bs)) for _ in range(3)]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--processes", type=int, default=1)
    ap.add_argument("--arith", default="bf16")
    ap.add_argument("--shapes", default="16x4,4x16")
    ap.add_argument("--search-only", action="store_true")
    ap.add_argument("--launches", action="store_true")
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode_beam_sample.py measures on the GPU: no device found")
    if args.launches:
        print(json.dumps({"decode_beam_sample_launches": launches(shapes)}))
        return
    if args.processes > 1:                                             # fresh child processes, one after the other
        recs = []
        for _ in range(args.processes):
            cmd = [sys.executable, os.path.abspath(__file__), "--runs", str(args.runs), "--arith", args.arith, "--shapes", args.shapes] + \
                  (["--search-only"] if args.search_only else [])
            out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900).stdout
            recs.append(json.loads(out.strip().splitlines()[-1])["decode_beam_sample"])
        print(json.dumps({"decode_beam_sample_processes": recs}))
        return
    print(json.dumps({"decode_beam_sample": [r for a in args.arith.split(",") for r in leg(a, args.runs, args.search_only, shapes)]}))


if __name__ == "__main__":
    main()
