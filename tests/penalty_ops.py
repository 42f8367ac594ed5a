"""Test support for generate(repetition_penalty): the CPU double's operators for csrc/topk_hist.hip on top of tests/fake_ops.py
(torch float32, the arithmetic of the kernels), and a record of the operator calls a decode issues."""
import torch

from fake_ops import FakeOps


def penalise(s, p):
    return torch.where(s < 0, s * p, s / p)


class PenaltyFakeOps(FakeOps):
    """FakeOps + logprob_topk_hist / beam_hist_update.  ``calls`` (a list, or None): receives the name of every operator called."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.calls = None

    def __getattribute__(self, name):
        attr = object.__getattribute__(self, name)
        if name.startswith("_") or not callable(attr):
            return attr
        calls = object.__getattribute__(self, "__dict__").get("calls")
        if calls is None:
            return attr

        def recorded(*a, **k):
            calls.append(name)
            return attr(*a, **k)
        return recorded

    def logprob_topk_hist(self, logits, M, V, k, banned, n_banned, hist, hist_len, penalty, mode, out_val, out_idx):
        """tasu_logprob_topk_hist: mode 1 penalises the raw logits of the row's history tokens before the softmax, mode 0 their
        log-probs after it (no renormalisation); once per distinct token; banned columns score -inf."""
        p = torch.tensor(float(penalty), dtype=torch.float32)
        lg = logits[:M, :V].float().clone()
        hs = [hist[r, :int(hist_len[r])].long().unique() for r in range(M)]
        if mode == 1:
            for r, h in enumerate(hs):
                lg[r, h] = penalise(lg[r, h], p)
        lp = lg - torch.logsumexp(lg, -1, keepdim=True)
        if mode == 0:
            for r, h in enumerate(hs):
                lp[r, h] = penalise(lp[r, h], p)
        if n_banned:
            ban = banned[:n_banned].long()
            lp[:, ban[ban >= 0]] = float("-inf")
        v, i = torch.sort(lp, dim=-1, descending=True, stable=True)
        out_val[:M] = v[:, :k]
        out_idx[:M] = i[:, :k].to(out_idx.dtype)

    def beam_hist_update(self, bs):
        """tasu_beam_hist_update: row m's history = its parent's + its new token; a no-op once the search is done."""
        n = int(bs.ctl[0])
        if int(bs.ctl[1]) or n < 1 or n > bs.max_new:
            return
        M = bs.B * bs.nb
        old = bs.hist.clone()
        bs.hist[:, :n - 1] = old[bs.next_src[:M].long(), :n - 1]
        bs.hist[:, n - 1] = bs.next_ids[:M]
        bs.hist_len[:M] = n
