"""Test support for generate(do_sample=True, num_beams=1): the CPU double's operators for csrc/sample.hip on top of
tests/penalty_ops.py (torch float32, the arithmetic of the kernels; the uniforms in integer numpy)."""
import numpy as np
import torch

from penalty_ops import PenaltyFakeOps, penalise
from sample_ref64 import uniforms

POOL = 1024


class SampleFakeOps(PenaltyFakeOps):
    """PenaltyFakeOps + sample_uniform / sample_rows / f32_sample_rows."""

    def sample_uniform(self, seed, counter, M, u):
        u[:M] = torch.from_numpy(uniforms(int(seed[0]), int(counter[0]), M))

    def sample_rows(self, logits, M, V, u, banned, n_banned, hist, hist_len, penalty, temperature, top_k, top_p, out_val, out_idx):
        """tasu_sample_rows: penalty on the raw logits of the row's distinct history tokens, ban, s = x / T, top-k with ties kept,
        top-p on the ascending cumulative mass, inverse CDF in token-id order; slot 1 = (-inf, 0x7fffffff)."""
        assert 1 <= top_k <= POOL and temperature > 0 and top_p >= 0
        lg = logits[:M, :V].float().clone()
        if hist is not None:
            p = torch.tensor(float(penalty), dtype=torch.float32)
            for r in range(M):
                h = hist[r, :int(hist_len[r])].long().unique()
                lg[r, h] = penalise(lg[r, h], p)
        if n_banned:
            ban = banned[:n_banned].long()
            lg[:, ban[ban >= 0]] = float("-inf")
        s = lg / torch.tensor(float(temperature), dtype=torch.float32)
        s = torch.where(s == 0, torch.zeros_like(s), s)
        for r in range(M):
            row = s[r]
            order = torch.from_numpy(np.lexsort((np.arange(V), -row.numpy())))            # (s descending, id ascending)
            k = min(top_k, int((row > float("-inf")).sum()))
            n = min(int((row >= row[order[k - 1]]).sum()), POOL)
            ids = order[:n]
            w = torch.exp(row[ids] - row[ids[0]])
            if top_p < 1.0:
                sfx = torch.flip(torch.cumsum(torch.flip(w, [0]), 0), [0])
                gone = torch.nonzero((sfx <= (torch.tensor(1.0) - torch.tensor(float(top_p))) * sfx[0]) & (torch.arange(n) >= 1)).flatten()
                if len(gone):
                    ids, w = ids[:int(gone[0])], w[:int(gone[0])]
            o = torch.argsort(ids)
            ids, w = ids[o], w[o]
            C = torch.cumsum(w, 0)
            hit = torch.nonzero(C > u[r] * C[-1]).flatten()
            i = int(hit[0]) if len(hit) else len(ids) - 1
            out_val[r, 0] = (row[ids[i]] - row[order[0]]) - torch.log(C[-1])
            out_idx[r, 0] = int(ids[i])
            out_val[r, 1] = float("-inf")
            out_idx[r, 1] = 0x7fffffff

    f32_sample_rows = sample_rows
