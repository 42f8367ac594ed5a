"""TEST INFRASTRUCTURE ONLY -- the wide-beam decode fixture and the scripted candidate streams of the wide beam update.

``wide_cases()``: tests/golden/mid_generate_wide.npz (tools/make_golden_generate_wide.py), num_beams 5..16 with the REAL reference's
tokens.  ``Script``: per-step top-K values / token ids [B * nb, K] that do not depend on the state (so every implementation can be
driven through the same stream and compared after every step), quantised to halves so that scores tie across beams and tokens."""
import numpy as np
import torch

NEG = np.float32(-1.0e9)


def wide_cases():
    """(geo, state dict, cases): each case dict(ids, am, post_ids, kw, tokens, bf16_stable, differs) -- kw includes repetition_penalty."""
    from conftest import load_npz, split_flat
    from ps_slm_amd.model import Geometry
    from ps_slm_amd.synthetic import MID_GEOMETRY, decode_fixture_state_dict

    z = load_npz("mid_generate_wide")
    geo = Geometry.from_dict(MID_GEOMETRY)
    sd = decode_fixture_state_dict(geo, int(z["seed_w"]))
    cases = []
    for n in range(int(z["n_cases"])):
        nb, new, min_len = (int(v) for v in z[f"c{n}_kw"])
        cases.append(dict(ids=torch.from_numpy(z[f"c{n}_input_ids"]), am=torch.from_numpy(z[f"c{n}_attention_mask"]),
                          post_ids=split_flat(z[f"c{n}_post_ids_flat"], z[f"c{n}_post_lens"]), tokens=z[f"c{n}_tokens"],
                          bf16_stable=bool(z["bf16_stable"][n]), differs=bool(z["differs_from_nb4"][n]),
                          kw=dict(num_beams=nb, max_new_tokens=new, min_length=min_len, length_penalty=float(z[f"c{n}_length_penalty"]),
                                  repetition_penalty=float(z[f"c{n}_repetition_penalty"]))))
    return geo, sd, cases


EOS = 7
KINDS = {"sparse": 0.6, "heavy": 1.0, "allstop": 2.0}          # script kind -> the length penalty it runs under


class Script:
    """Step t -> (vals [B * nb, K] float32 descending per row, idx [B * nb, K] int32).  Values are multiples of 0.5 in [-4, 0] (ties
    across beams and tokens at every step); tokens come from 8 .. 8 + 3 K (several rows of an utterance offer the same token).
      sparse   EOS only where scripted: step 3 the best candidate of beam 0 (inside the first nb), step 6 the last column of the last
               beam (outside), step 9 column 1 of every beam with equal scores; runs until max_new.
      heavy    from step 4 every row offers EOS among its first three columns: the heaps fill, utterances stop improving one by one.
      allstop  step 11: every candidate of utterance 0 ALONE is EOS (the batch goes on when B > 1); step 13: every candidate of every
               utterance is EOS -- done because every candidate stopped."""

    def __init__(self, kind, B, nb, seed):
        self.kind, self.B, self.nb, self.K, self.seed = kind, B, nb, 2 * nb, seed

    def step(self, t):
        B, nb, K = self.B, self.nb, self.K
        rng = np.random.default_rng(1000 * self.seed + t)
        vals = -np.sort(rng.integers(0, 9, (B * nb, K)), axis=1).astype(np.float32) / 2
        idx = np.stack([rng.permutation(3 * K)[:K] + 8 for _ in range(B * nb)]).astype(np.int32)
        v3, i3 = vals.reshape(B, nb, K), idx.reshape(B, nb, K)
        if self.kind == "sparse":
            if t == 3:
                i3[:, 0, 0], v3[:, 0, 0] = EOS, 0.0
            elif t == 6:
                i3[:, nb - 1, K - 1] = EOS
            elif t == 9:
                i3[:, :, 1], v3[:, :, :2] = EOS, 0.0
        elif self.kind == "heavy" and t >= 4:
            col = rng.integers(0, min(3, K), (B, nb))
            np.put_along_axis(i3, col[:, :, None], EOS, 2)
        elif self.kind == "allstop":
            if t == 11:
                i3[0] = EOS
            elif t == 13:
                i3[:] = EOS
        return vals, idx


def first_step_for_host(vals, idx, B, nb):
    """The first call hands the device B rows (only beam 0 exists); BeamState takes [B, nb, K]: the absent beams as the kernel
    sees them (NEG, token 0)."""
    K = vals.shape[1]
    v = np.full((B, nb, K), NEG, dtype=np.float32)
    i = np.zeros((B, nb, K), dtype=np.int64)
    v[:, 0], i[:, 0] = vals, idx
    return v, i


STATE = ("run_scores", "fin_scores", "fin_len", "fin_par", "fin_tok", "is_fin", "unsat", "ctl", "valid", "next_ids", "next_src", "next_pos",
         "next_slot", "next_lens", "banned")


def drive(ops, device, script, T, length_penalty, min_len, steps):
    """``steps`` calls of ops.beam_update (the HIP kernel or the CPU double) over a DeviceBeam fed by ``script``.  Returns (one dict of
    host copies of every state array per call -- bp_tok / bp_par: the step's row --, the DeviceBeam)."""
    from ps_slm_amd.decode import DeviceBeam
    from ps_slm_amd.model import Geometry, TasuModel
    from ps_slm_amd.synthetic import MID_GEOMETRY
    B, nb = script.B, script.nb
    model = TasuModel(Geometry.from_dict(dict(MID_GEOMETRY, llm_layers=0)), ops, device)
    dev = model.device
    bs = DeviceBeam(model, B, nb, T, EOS, length_penalty, min_len, S=5, valid=[3 + b % 3 for b in range(B)])
    bs.bp_tok.zero_()
    bs.bp_par.zero_()
    snaps = []
    for t in range(steps):
        vals, idx = script.step(t)
        if t == 0:
            vals, idx = vals.reshape(B, nb, -1)[:, 0], idx.reshape(B, nb, -1)[:, 0]
        ops.beam_update(torch.from_numpy(np.ascontiguousarray(vals)).to(dev), torch.from_numpy(np.ascontiguousarray(idx)).to(dev), bs, t == 0)
        snap = {n: getattr(bs, n).cpu().numpy().reshape(getattr(bs, n).shape).copy() for n in STATE}
        bpt, bpp = bs.bp_tok.cpu().numpy().copy(), bs.bp_par.cpu().numpy().copy()
        snap.update(bp_tok=bpt[min(t, T - 1)], bp_par=bpp[min(t, T - 1)], bp_tok_all=bpt, bp_par_all=bpp)
        snaps.append(snap)
    return snaps, bs


def check_against_beam_state(snaps, state, script, steps):
    """Drives ``state`` through ``script`` and compares it with the recorded device state after every step (bit for bit); calls
    after done must leave the device state as it is.  Returns the number of steps until done."""
    B, nb = state.B, state.nb
    n_steps = 0
    for t in range(steps):
        s = snaps[t]
        if state.done:
            for name, arr in snaps[t - 1].items():
                if name not in ("bp_tok", "bp_par"):
                    assert np.array_equal(arr, s[name]), (t, name, "a call after done changed the state")
            continue
        vals, idx = script.step(t)
        if t == 0:
            v, i = first_step_for_host(vals.reshape(B, nb, -1)[:, 0], idx.reshape(B, nb, -1)[:, 0], B, nb)
        else:
            v, i = vals.reshape(B, nb, -1), idx.reshape(B, nb, -1).astype(np.int64)
        tok, par = state.update(v, i)
        n_steps += 1
        for name, want in (("run_scores", state.run_scores), ("fin_scores", state.fin_scores), ("fin_len", state.fin_len),
                           ("is_fin", state.is_fin.astype(np.int64)), ("unsat", state.unsat.astype(np.int64)),
                           ("ctl", np.array([state.cur, int(state.done)])), ("next_ids", tok.reshape(-1)),
                           ("next_src", (np.arange(B)[:, None] * nb + par).reshape(-1)), ("bp_tok", tok), ("bp_par", par),
                           ("next_slot", np.full(B * nb, 5 + t)), ("next_lens", np.full(B * nb, 5 + t + 1)),
                           ("next_pos", np.repeat(s["valid"] + t, nb)), ("banned", np.array([EOS if state.cur < 2 else -1]))):
            got = s[name]
            assert got.shape == np.asarray(want).shape and np.array_equal(got, want), (t, name, got, want)
    return n_steps
