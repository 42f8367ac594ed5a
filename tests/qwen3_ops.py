"""TEST HELPER (not a test, never shipped): the CPU double of tests/fake_ops.py (through its decode-knob subclasses: the record of
operator calls, the penalty and sampling operators) with Qwen3's three operators (csrc/qk_norm.hip) in torch, in the arithmetic
include/tasu_hip.h states: statistic and pre * r in fp32, ONE rounding to bf16, times the fp32 weight and rotated in fp32, ONE
rounding at the store; backward with the rounding of xn taken as the identity."""
import torch

from beam_sample_ops import BeamSampleFakeOps
from fake_ops import HD, _bf


class Qwen3FakeOps(BeamSampleFakeOps):
    def _qk_norm(self, pre, wq, wk, M, H, G, eps):
        """(w * bf16(pre * r) of the q and k heads [M, H+G, 128] fp32, r [M, H+G])"""
        x = pre[:M].view(M, H + 2 * G, HD)[:, :H + G].float()
        r = torch.rsqrt(x.pow(2).mean(-1) + eps)
        w = torch.cat([wq.view(1, HD).expand(H, HD), wk.view(1, HD).expand(G, HD)])[None]
        return w * _bf(x * r[..., None]).float(), r

    def qk_norm_rope_fwd(self, pre, wq, wk, cos, sin, out, rstd, M, H, G, eps):
        y, r = self._qk_norm(pre, wq, wk, M, H, G, eps)
        o = out[:M].view(M, H + 2 * G, HD)
        if out.data_ptr() != pre.data_ptr():
            o[:, H + G:] = pre[:M].view(M, H + 2 * G, HD)[:, H + G:]
        o[:, :H + G] = _bf(self._rot(y, cos[:M].view(M, 1, 64), sin[:M].view(M, 1, 64)))
        if rstd is not None:
            rstd[:M].view(M, H + G).copy_(r)

    def qk_norm_bwd(self, dqkv, pre, wq, wk, rstd, M, H, G):
        x = pre[:M].view(M, H + 2 * G, HD)[:, :H + G].float()
        g = dqkv[:M].view(M, H + 2 * G, HD)
        r = rstd[:M].view(M, H + G, 1)
        w = torch.cat([wq.view(1, HD).expand(H, HD), wk.view(1, HD).expand(G, HD)])[None]
        wg, xn = w * g[:, :H + G].float(), x * r
        g[:, :H + G] = _bf(r * (wg - xn * (wg * xn).mean(-1, keepdim=True)))

    def qk_norm_rope_append(self, qkv, wq, wk, cos, sin, kc, vc, pos, M, H, G, ctx, eps):
        self.qk_norm_rope_fwd(qkv, wq, wk, cos, sin, qkv, None, M, H, G, eps)
        self.kv_append(qkv, kc, vc, pos, M, H, G, ctx)
