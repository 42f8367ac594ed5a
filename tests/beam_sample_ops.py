"""Test support for generate(do_sample=True, num_beams > 1): the CPU double's operators for the beam-sample kernels of csrc/sample.hip
and csrc/beam.hip on top of tests/sample_ops.py (torch / numpy float32, the arithmetic of the kernels; the keys' RNG in integer numpy)."""
import numpy as np
import torch

from beam_sample_ref64 import gumbel32
from penalty_ops import penalise
from sample_ops import POOL, SampleFakeOps

NONE = 0x7fffffff


class BeamSampleFakeOps(SampleFakeOps):
    """SampleFakeOps + beam_sample_rows / f32_beam_sample_rows / beam_update_drawn."""

    def beam_sample_rows(self, logits, M, V, K, first, bs, n_banned, temperature, top_k, top_p, out_key, out_val, out_idx):
        """tasu_beam_sample_rows: log-softmax, the penalty on the log-probs of the row's distinct history tokens, ban, s = lp / T, top-k
        at max(top_k, 2) with ties kept, top-p that keeps the two largest, a = s + running score, key = a + G; per row the K largest
        keys in (key descending, id ascending) order, the rest (-inf, -inf, 0x7fffffff)."""
        assert 1 <= top_k <= POOL and temperature > 0 and top_p >= 0 and 1 <= K <= 32 and M == bs.B * bs.nb
        seed, t, nb = int(bs.seed[0]), int(bs.ctl[0]), bs.nb
        run = bs.run_scores.reshape(-1)
        ban = bs.banned[:n_banned].long() if n_banned else None
        for m in range(M):
            lg = logits[m // nb if first else m, :V].float()
            lp = lg - torch.logsumexp(lg, -1)
            if bs.hist is not None:
                h = bs.hist[m, :int(bs.hist_len[m])].long().unique()
                lp[h] = penalise(lp[h], torch.tensor(float(bs.penalty), dtype=torch.float32))
            if ban is not None:
                lp[ban[ban >= 0]] = float("-inf")
            row = lp / torch.tensor(float(temperature), dtype=torch.float32)
            row = torch.where(row == 0, torch.zeros_like(row), row)
            order = torch.from_numpy(np.lexsort((np.arange(V), -row.numpy())))            # (s descending, id ascending)
            k = min(max(top_k, 2), int((row > float("-inf")).sum()))
            n = min(int((row >= row[order[k - 1]]).sum()), POOL)
            ids = order[:n]
            if top_p < 1.0:
                w = torch.exp(row[ids] - row[ids[0]])
                sfx = torch.flip(torch.cumsum(torch.flip(w, [0]), 0), [0])
                gone = torch.nonzero((sfx <= (torch.tensor(1.0) - torch.tensor(float(top_p))) * sfx[0]) & (torch.arange(n) >= 2)).flatten()
                if len(gone):
                    ids = ids[:int(gone[0])]
            ids = ids.numpy()
            a = (row[ids] + run[m]).numpy().astype(np.float32)
            key = (a + gumbel32(seed, t, m * V + ids.astype(np.int64))).astype(np.float32)
            o = np.lexsort((ids, -key.astype(np.float64)))[:K]
            out_key[m], out_val[m], out_idx[m] = float("-inf"), float("-inf"), NONE
            out_key[m, :len(o)] = torch.from_numpy(key[o])
            out_val[m, :len(o)] = torch.from_numpy(a[o])
            out_idx[m, :len(o)] = torch.from_numpy(ids[o]).to(out_idx.dtype)

    f32_beam_sample_rows = beam_sample_rows

    def beam_update_drawn(self, keys, vals, idx, bs):
        """Scalar restatement of tasu_beam_update_drawn: the utterance's K candidates by (key descending, beam, token), then
        FakeOps.beam_update's steps on (accumulated score, beam, token) in that order (float32 arithmetic in the same order)."""
        f32 = np.float32
        NEG = f32(-1.0e9)
        if int(bs.ctl[1]):
            return
        B, nb, K, cur = bs.B, bs.nb, 2 * bs.nb, int(bs.ctl[0])
        KY, V, I = keys.numpy(), vals.numpy(), idx.numpy()
        unsat_any, stop_all = False, True
        lp_now = f32(bs.len_pow[cur + 1])
        for b in range(B):
            cand = []                                            # (key, beam, token, score)
            for j in range(nb):
                for k in range(K):
                    t = int(I[b * nb + j, k])
                    if t < 0 or t == NONE:
                        cand.append((f32(-np.inf), j, 0, f32(-np.inf)))
                    else:
                        cand.append((f32(KY[b * nb + j, k]), j, t, f32(V[b * nb + j, k])))
            cand.sort(key=lambda c: (-c[0], c[1], c[2]))
            top = [(s, j, t) for _, j, t, s in cand[:K]]
            stop = [t == bs.eos or cur + 1 >= bs.max_new for _, _, t in top]
            stop_all = stop_all and all(stop)
            run_lp = [f32(s + (NEG if st else f32(0))) for (s, _, _), st in zip(top, stop)]
            nxt = sorted(range(K), key=lambda i: (-run_lp[i], i))[:nb]
            for n, i in enumerate(nxt):
                bs.bp_tok[cur, b, n], bs.bp_par[cur, b, n] = top[i][2], top[i][1]
                m = b * nb + n
                bs.next_ids[m], bs.next_src[m] = top[i][2], b * nb + top[i][1]
                bs.next_pos[m], bs.next_slot[m], bs.next_lens[m] = int(bs.valid[b]) + cur, bs.S + cur, bs.S + cur + 1
            unsat = bool(bs.unsat[b])
            merged = [(f32(bs.fin_scores[b, j]), int(bs.fin_len[b, j]), int(bs.fin_par[b, j]), int(bs.fin_tok[b, j]),
                       int(bs.is_fin[b, j])) for j in range(nb)]
            for i, (s, bm, t) in enumerate(top):
                just = stop[i] and i < nb
                sc = f32(s / lp_now)
                sc = f32(sc + (f32(0) if unsat else NEG))
                sc = f32(sc + (f32(0) if just else NEG))
                merged.append((sc, cur + 1, bm, t, int(just)))
            keep = sorted(range(nb + K), key=lambda i: (-merged[i][0], i))[:nb]
            for n, i in enumerate(keep):
                bs.fin_scores[b, n] = float(merged[i][0])
                bs.fin_len[b, n], bs.fin_par[b, n], bs.fin_tok[b, n], bs.is_fin[b, n] = merged[i][1:]
                bs.run_scores[b, n] = float(run_lp[nxt[n]])
            best_run = f32(run_lp[nxt[0]] / lp_now)
            min_fin = min(merged[i][0] for i in keep)
            improve = any(best_run > (min_fin if merged[i][4] else NEG) for i in keep)
            bs.unsat[b] = int(unsat and improve)
            unsat_any = unsat_any or bool(bs.unsat[b])
        done = not (unsat_any and not stop_all)
        bs.ctl[0], bs.ctl[1] = cur + 1, int(done)
        bs.banned[0] = bs.eos if cur + 1 < bs.min_length else -1
        if bs.done_host is not None:
            bs.done_host[0] = cur + 1 if done else 0
