"""TEST HELPER (not a test, never shipped): the CPU double for full fine-tuning of a Qwen3 decoder -- tests/qwen3_ops.py (the head
norm's operators) + tests/full_ft_ops.py (the decoder's weight gradients) + the q_norm / k_norm weight gradients of
csrc/qk_norm.hip in torch, in the arithmetic include/tasu_hip.h states: xn = bf16(pre * rstd) (fp32 family: pre * rstd), exact
products, fp32 sums; the v block is never read.  Also the golden cases of tools/make_golden_qwen3_full_ft.py."""
import torch

from conftest import load_npz
from fake_ops import HD, _bf
from full_ft_ops import FullFtFakeOps
from qwen3_ops import Qwen3FakeOps

GOLDENS = ("mid_qwen3_full_ft", "mid_qwen3_full_ft_untied")


class QkWgradTorch:
    """tasu_qk_norm_wgrad / tasu_f32_qk_norm_wgrad restated; ``mutant``: one of the three mistakes tests/test_qk_wgrad_ref64_cpu.py
    must see ("swap": dwq and dwk exchanged, "no-round": the bf16 rounding of xn dropped, "v": the v block summed into dwk)."""
    mutant = None

    def _qk_wgrad(self, dqkv, pre, rstd, dwq, dwk, M, H, G, accumulate, rounded):
        NQK = H + G
        upto = H + 2 * G if self.mutant == "v" else NQK
        x = pre[:M].view(M, H + 2 * G, HD)[:, :upto].float()
        g = dqkv[:M].view(M, H + 2 * G, HD)[:, :upto].float()
        r = rstd[:M].view(M, NQK, 1)
        if upto > NQK:
            r = torch.cat([r, r[:, H:]], 1)
        xn = x * r
        if rounded and self.mutant != "no-round":
            xn = _bf(xn).float()
        t = g * xn
        sq, sk = t[:, :H].sum((0, 1)), t[:, H:].sum((0, 1))
        if self.mutant == "swap":
            sq, sk = sk, sq
        dwq.copy_(dwq + sq if accumulate else sq)
        dwk.copy_(dwk + sk if accumulate else sk)

    def qk_norm_wgrad(self, dqkv, pre, rstd, dwq, dwk, ws, M, H, G, accumulate=False):
        assert ws.numel() >= 512 * 2 * HD and dqkv.data_ptr() != pre.data_ptr() and H % G == 0
        self._qk_wgrad(dqkv, pre, rstd, dwq, dwk, M, H, G, accumulate, True)

    def f32_qk_norm_wgrad(self, dqkv, pre, rstd, dwq, dwk, ws, M, H, G, accumulate=False):
        assert ws.numel() >= 512 * 2 * HD and dqkv.data_ptr() != pre.data_ptr() and H % G == 0
        self._qk_wgrad(dqkv, pre, rstd, dwq, dwk, M, H, G, accumulate, False)


class Qwen3FullFtFakeOps(QkWgradTorch, Qwen3FakeOps, FullFtFakeOps):
    """the operator set a Qwen3 model with freeze_llm=false runs on, on the CPU"""


def golden_case(name):
    """(fixture, geometry, state dict, batch) of a Qwen3 full-FT golden: the seeds, weight scale and batch of mid_qwen3_step."""
    import dataclasses

    import qwen3_ref as R
    from ps_slm_amd.synthetic import qwen3_state_dict, synthetic_text_batch
    z = load_npz(name)
    geo = dataclasses.replace(R.mid_qwen3_geometry(), tied=bool(int(z["tied"])))
    sd = qwen3_state_dict(geo, int(z["seed_w"]), with_encoder=False, scale=float(z["scale"]))
    batch = synthetic_text_batch(geo, 3, seed=int(z["seed_b"]), prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=12,
                                 noise=False, ragged=True)
    return z, geo, sd, batch


def build_ft(geo, sd, ops, device, fp32=False):
    """A TasuModel with the decoder in the bucket, the masters from the fp32 tensors; ``fp32``: what model_factory builds for
    use_fp16 = false (fp32 everywhere)."""
    from ps_slm_amd.model import TasuModel
    m = TasuModel(geo, ops, device)
    if fp32:
        m.llm.keep_f32 = True
        m.arith = m.arith_train = "fp32"
    m.load_reference_state_dict(sd)
    m.enable_llm_training(sd)
    return m


def n_llm_tensors(geo):
    """11 per layer (7 Linear weights, 2 layer norms, q_norm, k_norm; no bias), the final norm, the table, an untied head"""
    return 11 * geo.llm_layers + 2 + (0 if geo.tied else 1)


def check_step_against_golden(m, st, z, cos_min=0.995, norm_tol=5e-2, show=None):
    """The bars tests/test_full_ft_cpu.py applies to every Qwen2 tensor: |loss - ref| < 2e-2, logits within 3 % of the range,
    projector gradients cosine > 0.995, and EVERY tensor of the decoder -- q_norm and k_norm of every layer among them -- on the
    fixture's sub-grid: cosine > 0.995, full-tensor norm within 5 %."""
    from full_ft_ops import llm_grads, stored
    from test_lora_cpu import cosine
    res = st.dev["loss_out"].cpu()
    assert abs(float(res[0]) - float(z["loss"])) < 2e-2
    valid = torch.from_numpy(st.plan.key_mask[:, : st.S].astype(bool))
    cols = torch.from_numpy(z["cols"])
    lg = m.logits_view(st).float().cpu()
    ref = torch.from_numpy(z["logits_cols"])
    assert float((lg[:, :, cols] - ref)[valid].abs().max() / ref[valid].abs().max()) < 3e-2
    n = 0
    for k, g in m.projector_grads().items():
        short = "grad." + k[len("encoder_projector."):]
        if short in z:
            assert cosine(g, torch.from_numpy(z[short])) > cos_min, k
            n += 1
    assert n == 5
    gs = llm_grads(m)
    want = sorted(k[len("g."):] for k in z if k.startswith("g."))
    assert sorted(gs) == want and len(want) == n_llm_tensors(m.geo)
    assert sum(k.endswith(("q_norm.weight", "k_norm.weight")) for k in gs) == 2 * m.geo.llm_layers and not any(k.endswith(".bias") for k in gs)
    worst, heads = (2.0, None), (2.0, None)
    for k, g in gs.items():
        sub, ref = stored(g, z, k)
        c, rn = cosine(sub, ref), float(g.float().norm()) / float(z["gnorm." + k])
        worst = min(worst, (c, k))
        if k.endswith(("q_norm.weight", "k_norm.weight")):
            heads = min(heads, (c, k))
        assert c > cos_min and abs(rn - 1.0) < norm_tol, (k, c, rn)
    if show:
        print(f"{show}: loss {float(res[0]):.6f} (reference {float(z['loss']):.6f}); lowest gradient cosine {worst[0]:.6f} at {worst[1]}; "
              f"lowest of the head norms {heads[0]:.6f} at {heads[1]}")
