"""Test support for full fine-tuning of the LLM (freeze_llm=false): the CPU double's operators for csrc/wgrad.hip on top of
tests/fake_ops.py, and the golden cases of tools/make_golden_full_ft.py."""
import numpy as np
import torch

from conftest import load_npz
from fake_ops import FakeOps
from ps_slm_amd.model import Geometry, TasuModel
from ps_slm_amd.synthetic import MID_GEOMETRY, random_state_dict, synthetic_text_batch

GOLDENS = ("mid_text_full_ft", "mid_text_full_ft_untied")


class FullFtFakeOps(FakeOps):
    """FakeOps + the decoder's weight-gradient operators, the arithmetic of the kernels in torch (exact products of the bf16
    operands, fp32 sums)."""

    def gemm_tn_split(self, R, N, K):
        """tasu_gemm_tn_bf16_split restated (host code): about two 128 x 128-tile workgroups per CU, capped by the 64-row stages."""
        if R <= 0 or N <= 0 or K <= 0:
            return -1
        tiles = ((N + 127) // 128) * ((K + 127) // 128)
        return max(1, min(512 // tiles, 16, (R + 63) // 64))

    def gemm_tn(self, a, b, c, R, N, K, accumulate=False, nsplit=1, ws=None):
        assert N % 8 == 0 and K % 8 == 0 and 1 <= nsplit <= min(16, (R + 63) // 64)
        assert nsplit == 1 or ws.numel() >= nsplit * N * K
        acc = a[:R, :N].float().t() @ b[:R, :K].float()
        c[:N, :K] = c[:N, :K] + acc if accumulate else acc

    def colsum_split(self, x, out, ws, R, Cn, accumulate=False):
        s = x[:R, :Cn].float().sum(0)
        out[:Cn] = out[:Cn] + s if accumulate else s

    def rmsnorm_wgrad(self, dy, x, rstd, dw, ws, src_rows=None, accumulate=False):
        R, D = dy.shape
        if src_rows is not None:
            rows = src_rows[:R].long()
            ok = rows >= 0
            t = dy[:R].float()[ok] * x[rows[ok]] * rstd[:R][ok][:, None]
        else:
            t = dy.float() * x[:R] * rstd[:R, None]
        s = t.sum(0)
        dw.copy_(dw + s if accumulate else s)


def golden_case(name):
    """(fixture, geometry, state dict, batch) of a full-FT golden: the seeds and batch of mid_text_lora."""
    z = load_npz(name)
    geo = Geometry.from_dict(dict(MID_GEOMETRY, tied=bool(int(z["tied"]))))
    sd = random_state_dict(geo, int(z["seed_w"]), with_encoder=False)
    batch = synthetic_text_batch(geo, 3, seed=int(z["seed_b"]), prompt_len=9, n_audio=21, target_len=17, speech_pos=4,
                                 feat_frames=12, noise=True, drop_prob=0.15, ragged=True)
    batch["post_ids"] = [list(np.asarray(p)[np.asarray(k, dtype=bool)]) for p, k in zip(batch["post_ids"], batch["keeps"])]
    del batch["alphas"], batch["keeps"]
    return z, geo, sd, batch


def build_ft(geo, sd, ops, device):
    m = TasuModel(geo, ops, device)
    m.load_reference_state_dict(sd)
    m.enable_llm_training(sd)                          # the masters start from the fp32 tensors
    return m


def llm_grads(model):
    """Every LLM tensor's gradient under its checkpoint key (the embedding table included)."""
    from ps_slm_amd.full_ft import EMBED_KEY
    out = model.full_ft.grads()
    out[EMBED_KEY] = model.embed_grad()
    return out


def stored(g, z, key):
    """The fixture's sub-grid of gradient ``g`` of tensor ``key`` and the stored reference values (fp32)."""
    ref = torch.from_numpy(z["g." + key].astype(np.float32)) / float(z["gscale." + key])
    g = g.float().cpu()
    if key.endswith("embed_tokens.weight"):
        g = g[torch.from_numpy(z["egrad_rows"].astype(np.int64))]
    elif g.dim() == 2:
        g = g[::4, ::4]
    assert g.shape == ref.shape, (key, g.shape, ref.shape)
    return g, ref
