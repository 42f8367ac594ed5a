"""What a generated position costs at 64 beam rows cut three ways -- 16 utterances x 4 beams (bench.py's decode shape), 8 x 8 and
4 x 16 -- at Qwen2.5-1.5B geometry, a 128-position prompt and 200 forced positions (an EOS id that never matches), bf16 and fp32
arithmetic.  The GEMMs and the cache attention see the same 64 rows in all three; the difference is the top-k (k = 8 / 16 / 32), the
beam update and the position's set-up launches.

All shapes run in one process on one build, alternating, after one warm-up run of each (it captures the position's graph).  Per
arithmetic the line reports ms per position of every timed run.  Timed region as in bench.py's decode leg: prefill + the whole decode
loop, host clock around a device synchronise.  A build that does not serve a width reports null for it.

    python tools/bench_decode_wide.py [--runs 3] [--arith bf16,fp32] [--shapes 16x4,8x8,4x16] [--penalty 1.0]"""
import argparse
import gc
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def leg(arith, runs, shapes, penalty, new_tokens):
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
    raw = synthetic_text_batch(core.geo, max(b for b, _ in shapes), seed=1234, noise=False)

    def run(B, beams):
        ids = raw["input_ids"][:B, :25]
        st = core.prepare_text(ids, torch.ones_like(ids, dtype=torch.bool), None, raw["post_ids"][:B], None, None)
        kw = dict(num_beams=beams, max_new_tokens=new_tokens, eos_token_id=-1, pad_token_id=0, repetition_penalty=penalty)
        if arith == "fp32":
            return beam_search_generate_fp32(core, st, **kw)
        core.forward_projector_text(st)
        return beam_search_generate(core, st, **kw)

    outs = {}
    for s in shapes:                                                   # warm-up: every shape's buffers and graph
        try:
            outs[s] = run(*s)
        except ValueError as e:                                        # a build that does not serve this width
            outs[s] = None
            print(f"# {s[0]} x {s[1]}: {e}", file=sys.stderr)
    ms = {s: [] for s in shapes}
    for _ in range(runs):
        for s in shapes:
            if outs[s] is None:
                continue
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = run(*s)
            torch.cuda.synchronize()
            ms[s].append(round((time.perf_counter() - t0) * 1e3 / int(out.shape[1]), 4))
            assert torch.equal(out, outs[s])                           # the same tokens every run
    rec = {"arith": arith, "repetition_penalty": penalty, "new_tokens": new_tokens,
           "ms_per_position": {f"{b}x{n}": (ms[(b, n)] if outs[(b, n)] is not None else None) for b, n in shapes}}
    core._dec_graphs.clear()
    del model, core
    gc.collect()
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--arith", default="bf16,fp32")
    ap.add_argument("--shapes", default="16x4,8x8,4x16")
    ap.add_argument("--penalty", type=float, default=1.0)
    ap.add_argument("--new-tokens", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode_wide.py measures on the GPU: no device found")
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    print(json.dumps({"decode_wide": [leg(a, args.runs, shapes, args.penalty, args.new_tokens) for a in args.arith.split(",")]}))


if __name__ == "__main__":
    main()
