"""fp32 cross-attention projector kernel (tasu_f32_ca_attn) and fp32 generate() of a LoRA model against its base model.

    python tools/bench_f32_ca.py
    python tools/bench_f32_ca.py --bwd       # the kernel legs only, forward and backward (tasu_f32_ca_attn_bwd: 6 R V D FLOP)

Kernel: the Qwen2.5-1.5B (D = 1536, dh = 192) and 7B (D = 3584, dh = 448) geometries, V = 151,936, R in {64, 512}; reported in ms
and as the fraction of the 157 TFLOPS fp32 matrix peak (4 R V D FLOP: two products of R x V x dh per head).  Decode: fp32
generate() in ms per generated position at Qwen2.5-1.5B, 16 utterances x 4 beams, for the base model and the same model with
r = 64 adapters on all seven Linears (the merged fp32 weights make the two the same step).  One JSON line per measurement."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_F32 = 157e12


def time_ca(ops, R, D, V=151936, H=8, reps=10):
    g = torch.Generator(device="cuda").manual_seed(R + D)
    table = torch.randn(V, D, generator=g, device="cuda") * 0.02
    q = torch.randn(R, D, generator=g, device="cuda")
    out = torch.empty(R, D, device="cuda")
    ws = torch.empty(ops.f32_ca_workspace_floats(R, V, D, H), device="cuda")
    for _ in range(2):
        ops.f32_ca_attn(q, table, out, R, H, ws=ws)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        ops.f32_ca_attn(q, table, out, R, H, ws=ws)
    ev[1].record()
    torch.cuda.synchronize()
    ms = ev[0].elapsed_time(ev[1]) / reps
    flop = 4.0 * R * V * D
    return {"kernel": "tasu_f32_ca_attn", "R": R, "V": V, "D": D, "dh": D // H, "ms": round(ms, 3),
            "tflops": round(flop / ms / 1e9, 1), "frac_f32_peak": round(flop / (ms * 1e-3) / PEAK_F32, 3)}


def time_ca_bwd(ops, R, D, V=151936, H=8, reps=10):
    """tasu_f32_ca_attn_bwd: three products of R x V x dh per head (S = Q K^T, dP = dO K^T, dq = dS K)."""
    g = torch.Generator(device="cuda").manual_seed(R + D)
    table = torch.randn(V, D, generator=g, device="cuda") * 0.02
    q, dout = torch.randn(R, D, generator=g, device="cuda"), torch.randn(R, D, generator=g, device="cuda")
    out, lse, dq = torch.empty(R, D, device="cuda"), torch.empty(R, H, device="cuda"), torch.empty(R, D, device="cuda")
    ws = torch.empty(ops.f32_ca_workspace_floats(R, V, D, H), device="cuda")
    ops.f32_ca_attn_lse(q, table, out, lse, R, H, ws=ws)
    for _ in range(2):
        ops.f32_ca_attn_bwd(q, table, out, dout, lse, dq, R, H, ws=ws)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        ops.f32_ca_attn_bwd(q, table, out, dout, lse, dq, R, H, ws=ws)
    ev[1].record()
    torch.cuda.synchronize()
    ms = ev[0].elapsed_time(ev[1]) / reps
    flop = 6.0 * R * V * D
    return {"kernel": "tasu_f32_ca_attn_bwd", "R": R, "V": V, "D": D, "dh": D // H, "ms": round(ms, 3),
            "tflops": round(flop / ms / 1e9, 1), "frac_f32_peak": round(flop / (ms * 1e-3) / PEAK_F32, 3)}


def time_generate(use_peft, B=16, new_tokens=64, beams=4):
    from ps_slm_amd.config import ModelConfig, TrainConfig
    from ps_slm_amd.decode_fp32 import beam_search_generate_fp32
    from ps_slm_amd.ps_slm import model_factory
    from ps_slm_amd.synthetic import random_lora_state_dict, synthetic_text_batch
    tc = TrainConfig(freeze_llm=True, freeze_encoder=True, gt_emb=True, gt_emb_noise=False, ctc_posterior=True, do_psd=True, use_fp16=False,
                     use_peft=use_peft, batching_strategy="dynamic")
    mc = ModelConfig(llm_path="synthetic:qwen2.5-1.5b", encoder_projector="linear-silu", encoder_dim=25055, llm_dim=1536)
    model, _ = model_factory(tc, mc, device="cuda:0", init_seed=1234, keep_logits=False, with_encoder=False)
    core = model.core
    if use_peft:
        core.lora.load_state_dict(random_lora_state_dict(core.geo, core.lora.cfg, 7, b_scale=0.01))
        core.sync_projector_copies()
    raw = synthetic_text_batch(core.geo, B, seed=1234, noise=False)
    ids = raw["input_ids"][:, :25]
    am = torch.ones_like(ids, dtype=torch.bool)

    def run():
        st = core.prepare_text(ids, am, None, raw["post_ids"], None, None)
        return beam_search_generate_fp32(core, st, num_beams=beams, max_new_tokens=new_tokens, eos_token_id=-1, pad_token_id=0)

    run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rec = {"generate_fp32": "lora r=64 (merged fp32 weights)" if use_peft else "base", "utterances": B, "beams": beams,
           "new_tokens": int(out.shape[1]), "ms_per_position": round(dt / int(out.shape[1]) * 1e3, 3)}
    core._dec_graphs.clear()
    del model, core
    import gc
    gc.collect()
    torch.cuda.empty_cache()
    return rec


def main():
    from ps_slm_amd.ops import HipOps
    ops = HipOps()
    bwd = "--bwd" in sys.argv[1:]
    for D in (1536, 3584):
        for R in (64, 512):
            print(json.dumps(time_ca(ops, R, D)), flush=True)
            if bwd:
                print(json.dumps(time_ca_bwd(ops, R, D)), flush=True)
    if bwd:
        return
    torch.cuda.empty_cache()
    for use_peft in (False, True):
        print(json.dumps(time_generate(use_peft)), flush=True)


if __name__ == "__main__":
    main()
