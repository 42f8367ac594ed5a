"""TEST HELPER (not a test, never shipped): the CPU double the whole fp32 training step (ps_slm_amd/train_fp32.py: forward_train_fp32 +
run_backward) runs on, every recipe.  Composed from the torch restatements the float64 kernel tests already carry -- F32TrainTorch
(tests/f32_train_ref64.py), F32Torch (tests/f32_ref64.py), the fp32 head-norm operators (tests/qwen3_f32_ops.py), QkWgradTorch
(tests/qwen3_full_ft_ops.py) -- on top of FullFtFakeOps; what was missing is added here in the same style: torch fp32, exact
products, and the kernel's stated sum order where csrc/wgrad_f32.hip states one.  The two plans that are host code in the library
(tasu_f32_gemm_tn_split, tasu_f32_ca_workspace_floats) are asked of the library itself.  FakeOps stays without f32_* operators:
tests/test_fp32_cpu.py relies on their absence."""
import torch

from f32_ref64 import F32Torch
from f32_train_ref64 import F32TrainTorch
from full_ft_ops import FullFtFakeOps
from ps_slm_amd.model import TasuModel
from qwen3_f32_ops import Qwen3F32FakeOps
from qwen3_full_ft_ops import QkWgradTorch

TN_STAGE = 16                 # rows per stage of tasu_f32_gemm_tn (csrc/wgrad_f32.hip TS)
RMS_WGRAD_SPLIT = 64          # include/tasu_hip.h TASU_RMS_WGRAD_SPLIT


def _in_order(parts):
    s = parts[0]
    for p in parts[1:]:
        s = s + p
    return s


class F32StepOps(QkWgradTorch, F32TrainTorch, F32Torch, Qwen3F32FakeOps, FullFtFakeOps):
    name = "f32step-cpu"

    @property
    def lib(self):
        from ps_slm_amd import _lib
        return _lib.load()

    def f32_gemm_tn_split(self, R, N, K):
        return int(self.lib.tasu_f32_gemm_tn_split(R, N, K))

    def f32_ca_workspace_floats(self, R, V, D, H):
        return int(self.lib.tasu_f32_ca_workspace_floats(R, V, D, H))

    def f32_gemm_tn(self, a, b, c, R, N, K, accumulate=False, nsplit=1, ws=None):
        """c [N, K] = or += a[:R, :N]^T b[:R, :K]: ``nsplit`` ranges of 16-row stages, one slab each, summed in slab order."""
        stages = (R + TN_STAGE - 1) // TN_STAGE
        assert N % 4 == 0 and K % 4 == 0 and 1 <= nsplit <= min(16, stages) and (nsplit == 1 or ws.numel() >= nsplit * N * K)
        cuts = [min(R, stages * i // nsplit * TN_STAGE) for i in range(nsplit + 1)]
        s = _in_order([a[lo:hi, :N].t() @ b[lo:hi, :K] for lo, hi in zip(cuts, cuts[1:])])
        c[:N, :K] = c[:N, :K] + s if accumulate else s

    def _slabs(self, t, accumulate, out):
        """rows r = y, y + SPLIT, ... make slab y; the slabs are added in slab order"""
        s = _in_order([t[y::RMS_WGRAD_SPLIT].sum(0) for y in range(RMS_WGRAD_SPLIT)])
        out.copy_(out + s if accumulate else s)

    def f32_rmsnorm_wgrad(self, dy, x, dw, ws, eps, rstd=None, accumulate=False):
        R, D = dy.shape
        assert ws.numel() >= RMS_WGRAD_SPLIT * D + (0 if rstd is not None else R)
        if rstd is None:                                   # recomputed as the kernel does: the sum of squares in double, rounded once
            rstd = (1.0 / torch.sqrt(x[:R, :D].double().pow(2).sum(-1) / D + float(eps))).float()
        self._slabs(dy * x[:R, :D] * rstd[:R, None], accumulate, dw[:D])

    def f32_colsum_split(self, x, out, ws, R, Cn, accumulate=False):
        assert ws.numel() >= RMS_WGRAD_SPLIT * Cn
        self._slabs(x[:R, :Cn], accumulate, out[:Cn])

    def embed_bwd(self, dx, rows, seg_start, seg_id, dtable, n_rows, n_seg):
        """dtable[seg_id[s]] += (the rows dx[rows[seg_start[s] : seg_start[s + 1]]] summed in list order); id < 0: skipped"""
        for s in range(n_seg):
            i, j0, j1 = int(seg_id[s]), max(int(seg_start[s]), 0), min(int(seg_start[s + 1]), n_rows)
            if not 0 <= i < dtable.shape[0] or j0 >= j1:
                continue
            acc = torch.zeros_like(dtable[i])
            for j in range(j0, j1):
                if 0 <= int(rows[j]) < dx.shape[0]:
                    acc = acc + dx[int(rows[j])]
            dtable[i] += acc


class F32StepModel(TasuModel):
    """A CPU model that lets full fine-tuning and use_emb select the fp32 step: F32StepOps has the operators the property asks for."""
    f32_wgrad_served = True


def f32_step_model(geo, sd, ops=None):
    """What model_factory builds for use_fp16 = false with the fp32 training step selected, on the double."""
    m = F32StepModel(geo, ops or F32StepOps(), "cpu")
    m.llm.keep_f32 = True
    m.arith = m.arith_train = "fp32"
    m.load_reference_state_dict(sd)
    return m
