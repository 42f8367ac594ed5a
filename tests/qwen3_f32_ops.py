"""TEST HELPER (not a test, never shipped): tests/qwen3_ops.py's CPU double with the three fp32 head-norm operators of the fp32
family (csrc/qk_norm.hip, csrc/fp32.hip) in torch fp32, in the arithmetic include/tasu_hip.h states: HF's Qwen3RMSNorm on fp32
tensors, y = w * (x * rsqrt(mean_128(x^2) + eps)), then the rotation; nothing rounded to bf16.  Its CLASS has the three methods,
which is what model_factory and LLMWeights probe before they serve a Qwen3 decoder with use_fp16=false."""
import torch

from fake_ops import HD
from qwen3_ops import Qwen3FakeOps


class Qwen3F32FakeOps(Qwen3FakeOps):
    @staticmethod
    def _w32(wq, wk, H, G):
        return torch.cat([wq.view(1, HD).expand(H, HD), wk.view(1, HD).expand(G, HD)])[None]

    def f32_qk_norm_rope(self, pre, wq, wk, cos, sin, out, rstd, M, H, G, eps, kc=None, vc=None, slot=None, ctx=0):
        x = pre[:M].view(M, H + 2 * G, HD).clone()
        r = torch.rsqrt(x[:, :H + G].pow(2).mean(-1, keepdim=True) + eps)
        y = self._w32(wq, wk, H, G) * (x[:, :H + G] * r)
        c, s = torch.cat([cos[:M], cos[:M]], -1)[:, None], torch.cat([sin[:M], sin[:M]], -1)[:, None]
        o = out[:M].view(M, H + 2 * G, HD)
        o[:, :H + G] = y * c + torch.cat([-y[..., 64:], y[..., :64]], -1) * s
        o[:, H + G:] = x[:, H + G:]
        if rstd is not None:
            rstd[:M].view(M, H + G).copy_(r[..., 0])
        if kc is not None:
            rows, sl = torch.arange(M), slot[:M].long()
            kc.view(-1, ctx, G * HD)[rows, sl] = o[:, H:H + G].reshape(M, -1)
            vc.view(-1, ctx, G * HD)[rows, sl] = o[:, H + G:].reshape(M, -1)

    def f32_qk_norm_bwd(self, dqkv, pre, wq, wk, rstd, M, H, G):
        x = pre[:M].view(M, H + 2 * G, HD)[:, :H + G]
        g = dqkv[:M].view(M, H + 2 * G, HD)
        r = rstd[:M].view(M, H + G, 1)
        wg, xn = self._w32(wq, wk, H, G) * g[:, :H + G], x * r
        g[:, :H + G] = r * (wg - xn * (wg * xn).mean(-1, keepdim=True))

    def f32_gemm_qkv_norm_rope(self, a, wqkv, bias, qkv, wq, wk, cos, sin, M, H, G, K, eps, ws, kc=None, vc=None, slot=None, ctx=0):
        v = a[:M, :K] @ wqkv[:(H + 2 * G) * HD, :K].t()
        qkv[:M] = v + bias if bias is not None else v
        self.f32_qk_norm_rope(qkv, wq, wk, cos, sin, qkv, None, M, H, G, eps, kc, vc, slot, ctx)
