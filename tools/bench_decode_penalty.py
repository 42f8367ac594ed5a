"""What generate(repetition_penalty != 1) costs per generated position, at bench.py's decode shape: 16 utterances x 4 beams, a
128-position prompt, 200 forced positions (an EOS id that never matches), Qwen2.5-1.5B geometry, bf16 and fp32 arithmetic.

repetition_penalty = 1.0 and 1.3 run in the same process on the same build, alternating, after one warm-up run of each (the warm-up
captures the position's graph: the penalty is part of the graph key).  Per arithmetic the line reports ms per position of every
timed run, the range of both settings and the difference of their medians.  Timed region as in bench.py's decode leg: prefill +
the whole decode loop, host clock around a device synchronise.

    python tools/bench_decode_penalty.py [--runs 3] [--arith bf16,fp32]"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def leg(arith, runs, B=16, beams=4, new_tokens=200, penalty=1.3):
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

    def run(p):
        st = core.prepare_text(ids, am, None, raw["post_ids"], None, None)
        if arith == "fp32":
            return beam_search_generate_fp32(core, st, num_beams=beams, max_new_tokens=new_tokens, eos_token_id=-1, pad_token_id=0,
                                             repetition_penalty=p)
        core.forward_projector_text(st)
        return beam_search_generate(core, st, num_beams=beams, max_new_tokens=new_tokens, eos_token_id=-1, pad_token_id=0,
                                    repetition_penalty=p)

    def timed(p):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = run(p)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / int(out.shape[1]), out

    outs = {p: run(p) for p in (1.0, penalty)}                       # warm-up: every shape and both graphs
    ms = {1.0: [], penalty: []}
    for _ in range(runs):
        for p in (1.0, penalty):
            t, out = timed(p)
            assert torch.equal(out, outs[p])                           # the same tokens every run
            ms[p].append(round(t, 4))
    rec = {"arith": arith, "utterances": B, "beams": beams, "new_tokens": int(outs[1.0].shape[1]),
           "ms_per_position_p1.0": ms[1.0], f"ms_per_position_p{penalty}": ms[penalty],
           "median_difference_us": round((statistics.median(ms[penalty]) - statistics.median(ms[1.0])) * 1e3, 1),
           "tokens_differ": not torch.equal(outs[1.0], outs[penalty])}
    core._dec_graphs.clear()
    del model, core
    gc.collect()
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--arith", default="bf16,fp32")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode_penalty.py measures on the GPU: no device found")
    print(json.dumps({"decode_penalty": [leg(a, args.runs) for a in args.arith.split(",")]}))


if __name__ == "__main__":
    main()
