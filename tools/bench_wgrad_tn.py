"""tasu_gemm_tn_bf16 (csrc/wgrad.hip: dW = dY^T X from the row-major operands) against the composed route -- two
tasu_transpose_bf16 + the NT GEMM with fp32 output, what the projector's weight gradients run -- on the decoder's weight-gradient
shapes of the training step (16 x 256 tokens), the two routes alternated inside one process, timed by device events; and
tasu_rmsnorm_wgrad at the same row count.  One JSON line per shape.

    python tools/bench_wgrad_tn.py [--geometry 1.5b|7b] [--reps 20] [--rounds 3]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from ps_slm_amd.ops import GEMM_F32, RMS_WGRAD_SPLIT, HipOps

SHAPES = {   # (what, R, N, K): dW [N, K] = dY [R, N]^T X [R, K]
    "1.5b": [("q|k|v", 4096, 2048, 1536), ("o", 4096, 1536, 1536), ("gate|up", 4096, 17920, 1536), ("down", 4096, 1536, 8960),
             ("lm_head", 2048, 151936, 1536)],
    "7b": [("q|k|v", 4096, 4608, 3584), ("o", 4096, 3584, 3584), ("gate|up", 4096, 37888, 3584), ("down", 4096, 3584, 18944)],
}
BF16_PEAK_TFLOPS = 2500.0                                # MI355X dense bf16 MFMA peak


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps              # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", default="1.5b", choices=sorted(SHAPES))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    ops = HipOps()
    bf = torch.bfloat16
    for what, R, N, K in SHAPES[args.geometry]:
        a = torch.randn(R, N, device="cuda").to(bf)
        b = torch.randn(R, K, device="cuda").to(bf)
        a_t, b_t = torch.empty(N, R, dtype=bf, device="cuda"), torch.empty(K, R, dtype=bf, device="cuda")
        c_new, c_old = torch.empty(N, K, device="cuda"), torch.empty(N, K, device="cuda")
        nsplit = ops.gemm_tn_split(R, N, K)
        ws = torch.empty(nsplit * N * K, device="cuda") if nsplit > 1 else None

        def composed():
            ops.transpose(a, a_t, R, N, R, N)
            ops.transpose(b, b_t, R, K, R, K)
            ops.gemm(a_t, b_t, c_old, N, K, R, mode=GEMM_F32)

        routes = {"tn": lambda: ops.gemm_tn(a, b, c_new, R, N, K, nsplit=nsplit, ws=ws), "composed": composed}
        if nsplit > 1:
            routes["tn_whole"] = lambda: ops.gemm_tn(a, b, c_new, R, N, K)
        for fn in routes.values():                       # warm every route at this shape
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in routes}
        for _ in range(args.rounds):                     # alternate the routes
            for k, fn in routes.items():
                us[k].append(timed(fn, args.reps))
        routes["tn"]()
        composed()
        torch.cuda.synchronize()
        diff = float((c_new - c_old).abs().max() / c_old.abs().max())
        best = {k: min(v) for k, v in us.items()}
        flop = 2.0 * R * N * K
        print(json.dumps({"shape": what, "R": R, "N": N, "K": K, "nsplit": nsplit, "us": {k: [round(x, 1) for x in v] for k, v in us.items()},
                          "tn_tflops": round(flop / best["tn"] / 1e6, 1), "tn_share_of_bf16_peak": round(flop / best["tn"] / 1e6 / BF16_PEAK_TFLOPS, 3),
                          "composed_tflops": round(flop / best["composed"] / 1e6, 1), "faster": min(best, key=best.get),
                          "max_rel_diff": diff}), flush=True)
        del a, b, a_t, b_t, c_new, c_old, ws
    # the RMSNorm weight gradient: reads dy (bf16) and x (fp32) once
    R = 4096
    for D in {"1.5b": (1536,), "7b": (3584,)}[args.geometry]:
        dy = torch.randn(R, D, device="cuda").to(bf)
        x, rstd = torch.randn(R, D, device="cuda"), torch.rand(R, device="cuda")
        dw, ws = torch.empty(D, device="cuda"), torch.empty(RMS_WGRAD_SPLIT * D, device="cuda")
        fn = lambda: ops.rmsnorm_wgrad(dy, x, rstd, dw, ws)
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t = [timed(fn, args.reps) for _ in range(args.rounds)]
        print(json.dumps({"shape": "rmsnorm_wgrad", "R": R, "D": D, "us": [round(v, 1) for v in t],
                          "GBps": round(R * D * 6 / min(t) / 1e3, 1)}), flush=True)


if __name__ == "__main__":
    main()
