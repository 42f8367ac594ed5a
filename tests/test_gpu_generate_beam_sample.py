"""generate(do_sample=True, num_beams > 1) on the GPU: the row kernels tasu_beam_sample_rows / tasu_f32_beam_sample_rows against the
float64 restatement and its derived bound (tests/beam_sample_ref64.py), the tie rule and the pool's id cut, tasu_beam_update_drawn
against BeamState.update_drawn after every step, argument rejection, and the decode paths end to end against the REAL reference's
tokens (tests/golden/mid_generate_beam_sample.npz)."""
import types

import numpy as np
import pytest
import torch

import beam_sample_ref64 as R64
from beam_sample_ref import beam_sample_cases, same
from wide_cases import EOS, KINDS, STATE, Script

pytestmark = pytest.mark.gpu
I32 = torch.int32
NONE = 0x7fffffff


@pytest.fixture(scope="module")
def ops():
    from ps_slm_amd.ops import HipOps
    return HipOps()


def row_state(M, nb, seed, t, run, hist=None, hist_len=None, banned=-1, penalty=1.0):
    """The part of a DeviceBeam the row kernels read."""
    return types.SimpleNamespace(B=M // nb, nb=nb, seed=torch.tensor([seed], dtype=torch.int64, device="cuda"),
                                 ctl=torch.tensor([t, 0], dtype=I32, device="cuda"), run_scores=torch.as_tensor(run, dtype=torch.float32).cuda(),
                                 banned=torch.tensor([banned], dtype=I32, device="cuda"), penalty=penalty,
                                 hist=None if hist is None else torch.as_tensor(hist, dtype=I32).cuda(),
                                 hist_len=None if hist_len is None else torch.as_tensor(hist_len, dtype=I32).cuda())


def device_logits(x, dtype):
    R, V = x.shape
    ld = -(-V // 64) * 64 if dtype == torch.bfloat16 else V              # the decode buffers' leading dimensions
    lg = torch.zeros(R, ld, dtype=dtype)
    lg[:, :V] = torch.from_numpy(x).to(dtype)
    assert torch.equal(lg[:, :V].double(), torch.from_numpy(x))          # the grid is exact in both types
    return lg.cuda()


def run_rows(ops, dtype, lg, M, V, K, first, bs, T, top_k, top_p):
    """Two launches with a guard row behind the outputs -> (key, val, idx) of the first, after asserting equal bits."""
    fn = ops.beam_sample_rows if dtype == torch.bfloat16 else ops.f32_beam_sample_rows
    outs = []
    for _ in range(2):
        key, val = torch.full((M + 1, K), 7.0, device="cuda"), torch.full((M + 1, K), 7.0, device="cuda")
        idx = torch.full((M + 1, K), -7, dtype=I32, device="cuda")
        fn(lg, M, V, K, first, bs, 1, T, top_k, top_p, key, val, idx)
        torch.cuda.synchronize()
        outs.append((key.cpu(), val.cpu(), idx.cpu()))
    (key, val, idx), (key2, val2, idx2) = outs
    assert torch.equal(idx, idx2) and torch.equal(key.view(I32), key2.view(I32)) and torch.equal(val.view(I32), val2.view(I32))
    assert (idx[M] == -7).all() and (key[M] == 7.0).all() and (val[M] == 7.0).all()       # the guard row
    return key[:M].numpy(), val[:M].numpy(), idx[:M].numpy()


# ------------------------------------------------------------------------------------------ 1. the row kernels against float64
@pytest.mark.parametrize("n", range(len(R64.KERNEL_CASES)))
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_row_kernels_vs_float64(ops, dtype, n):
    """Every slot of every row: a float64 survivor, its accumulated score and key inside their bounds, the slots in (key, id) order,
    nothing clearly better left out, fillers behind; a row without an ambiguous class: exactly the reference's tokens in its order.
    At most 10 % of a case's rows are ambiguous."""
    c = R64.KERNEL_CASES[n]
    d = R64.kernel_inputs(c)
    rows = R64.kernel_rows(c, dtype == torch.bfloat16)
    bs = row_state(c.M, c.nb, R64.KERNEL_SEED, c.t, d["run"], d["hist"] if c.hist else None, d["hist_len"] if c.hist else None,
                   d["banned"] if c.hist else -1, R64.KERNEL_PENALTY if c.hist else 1.0)
    key, val, idx = run_rows(ops, dtype, device_logits(d["x"], dtype), c.M, c.V, c.K, c.first, bs, c.T, c.top_k, c.top_p)
    ambiguous = sum(r.ambiguous for r in rows)
    print(f"{dtype} {c}: {ambiguous} of {c.M} rows ambiguous")
    assert ambiguous <= R64.AMBIGUOUS_CAP * c.M
    for m, r in enumerate(rows):
        why = r.check(key[m], val[m], idx[m])
        assert why is None, (dtype, c, m, why)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_eight_tied_maxima_at_top_k_four_all_stay_and_a_row_of_ties_is_cut_by_id(ops, dtype):
    """Eight logits tied at the row's maximum, top_k = 4: HF keeps all eight (ties at the threshold stay); their scores are equal bit for
    bit, so with K = 10 the row hands over exactly those eight in the order of their Gumbel keys -- the float32 keys of the
    restatement up to logf's last bit -- and two fillers.  A constant row ties V columns at top_k = 4: the pool keeps the first 1024
    by id (the documented departure from HF), and the K best keys come from those."""
    V, M, nb, K, seed, t = 151936, 6, 2, 10, 987654321, 5
    g = np.random.default_rng(8)
    x = np.clip(np.round(g.normal(size=(M, V)) * 16) / 8, -12, 7.5)
    tied = []
    for r in range(M - 1):
        cols = sorted(([0, V - 1] + (g.permutation(V - 2)[:6] + 1).tolist()) if r % 2 else (g.permutation(V - 2)[:8] + 1).tolist())
        x[r, cols] = 9.0
        tied.append(cols)
    x[M - 1] = 1.5                                                                         # the constant row
    run = (-g.random(M) * 5).astype(np.float32)
    bs = row_state(M, nb, seed, t, run)
    key, val, idx = run_rows(ops, dtype, device_logits(x, dtype), M, V, K, False, bs, 0.7, 4, 1.0)
    for r in range(M - 1):
        assert sorted(idx[r, :8].tolist()) == tied[r] and idx[r, 8:].tolist() == [NONE] * 2, r
        assert len(set(val[r, :8].tolist())) == 1 and np.isneginf(key[r, 8:]).all() and np.isneginf(val[r, 8:]).all()
        G = R64.gumbel32(seed, t, r * V + idx[r, :8].astype(np.int64))
        want = (val[r, :8] + G).astype(np.float32)
        assert (np.abs(key[r, :8].astype(np.float64) - want) <= 4 * R64.e * (1 + np.abs(G) + np.abs(want))).all(), r
        assert (np.diff(key[r, :8]) <= 0).all()
    r = M - 1
    assert (idx[r] < 1024).all() and len(set(idx[r].tolist())) == K and len(set(val[r].tolist())) == 1
    ids = np.arange(1024)
    k32 = (val[r, 0] + R64.gumbel32(seed, t, r * V + ids)).astype(np.float32)
    best = ids[np.lexsort((ids, -k32.astype(np.float64)))[:K]]
    assert len(set(best.tolist()) & set(idx[r].tolist())) >= K - 1                         # (logf's last bit may swap the K-th)


def test_keys_follow_seed_and_position_under_graph_replay(ops):
    """Seed and position are device words: ONE captured launch gives other keys at another position and under another seed, each the
    restatement's within the bound."""
    c = R64.KERNEL_CASES[0]
    d = R64.kernel_inputs(c)
    lg = device_logits(d["x"], torch.float32)
    bs = row_state(c.M, c.nb, 11, 0, d["run"])
    K = c.K
    key, val, idx = (torch.zeros(c.M, K, device="cuda"), torch.zeros(c.M, K, device="cuda"), torch.zeros(c.M, K, dtype=I32, device="cuda"))
    ops.f32_beam_sample_rows(lg, c.M, c.V, K, False, bs, 1, c.T, c.top_k, c.top_p, key, val, idx)        # (eager first)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.f32_beam_sample_rows(lg, c.M, c.V, K, False, bs, 1, c.T, c.top_k, c.top_p, key, val, idx)
    seen = []
    for seed, t in ((11, 0), (11, 1), (-12, 1)):
        bs.seed.fill_(seed)
        bs.ctl[0] = t
        g.replay()
        torch.cuda.synchronize()
        for m in range(c.M):
            r = R64.Row(d["x"][m], None, [], 1.0, c.T, c.top_k, c.top_p, d["run"][m], seed, t, m, K, False)
            why = r.check(key[m].cpu().numpy(), val[m].cpu().numpy(), idx[m].cpu().numpy())
            assert why is None, (seed, t, m, why)
        seen.append(key.cpu().clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


def test_row_kernels_and_the_drawn_update_reject_bad_arguments(ops):
    from ps_slm_amd.ops import TasuOpError
    lg = torch.zeros(4, 1024, dtype=torch.bfloat16, device="cuda")
    lf = torch.zeros(4, 1000, dtype=torch.float32, device="cuda")
    key, val, idx = torch.zeros(4, 34, device="cuda"), torch.zeros(4, 34, device="cuda"), torch.zeros(4, 34, dtype=I32, device="cuda")
    hist, hl = torch.zeros(4, 8, dtype=I32), torch.zeros(4, dtype=I32)
    good = dict(M=4, V=1000, K=4, nb=2, T=1.0, top_k=50, top_p=1.0, hist=None, hl=None, penalty=1.0)
    bad = [dict(top_k=0), dict(top_k=1025), dict(T=0.0), dict(T=float("inf")), dict(top_p=-0.1), dict(top_p=float("nan")), dict(M=0), dict(M=258, nb=2),
           dict(M=3), dict(V=0), dict(V=1025), dict(K=0), dict(K=33), dict(nb=0), dict(penalty=1.3), dict(hist=hist, hl=hl, penalty=0.0)]
    for fn, logits in ((ops.beam_sample_rows, lg), (ops.f32_beam_sample_rows, lf)):
        for over in [{}] + bad:
            a = dict(good, **over)
            bs = row_state(4, max(a["nb"], 1), 1, 0, np.zeros(4, np.float32), a["hist"], a["hl"], -1, a["penalty"])
            bs.nb = a["nb"]
            call = lambda: fn(logits, a["M"], a["V"], a["K"], False, bs, 1, a["T"], a["top_k"], a["top_p"], key, val, idx)  # noqa: E731
            if over:
                with pytest.raises(TasuOpError):
                    call()
            else:
                call()
    bs = row_state(4, 2, 1, 0, np.zeros(4, np.float32))
    with pytest.raises(TasuOpError):                                      # a leading dimension that is no multiple of the vector width
        ops.beam_sample_rows(torch.zeros(4, 1004, dtype=torch.bfloat16, device="cuda"), 4, 1000, 4, False, bs, 1, 1.0, 50, 1.0, key, val, idx)
    with pytest.raises(TasuOpError):
        ops.f32_beam_sample_rows(torch.zeros(4, 1002, device="cuda"), 4, 1000, 4, False, bs, 1, 1.0, 50, 1.0, key, val, idx)
    _, dbs = drive_drawn(ops, "cuda", Script("sparse", 1, 16, seed=1), 4, 1.0, 0, 1)
    dbs.nb = 17
    with pytest.raises(TasuOpError):
        ops.beam_update_drawn(torch.zeros(17, 34, device="cuda"), torch.zeros(17, 34, device="cuda"), torch.zeros(17, 34, dtype=I32, device="cuda"), dbs)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ 2. the drawn beam update
def drawn_step(script, t):
    """Step t of a scripted stream for the drawn update: the script's values as ACCUMULATED scores and its tokens, keys that are
    multiples of 0.5 drawn independently of the scores (so the draw order is not the score order, and keys tie across beams and
    tokens), and from step 2 on one filler per utterance."""
    vals, idx = script.step(t)
    rng = np.random.default_rng(7000 * script.seed + t)
    keys = (rng.integers(0, 12, vals.shape) / 2).astype(np.float32)
    if t >= 2:
        k3, v3, i3 = (a.reshape(script.B, script.nb, script.K) for a in (keys, vals, idx))
        k3[:, -1, -1], v3[:, -1, -1], i3[:, -1, -1] = -np.inf, -np.inf, NONE
    return keys, vals, idx


def drive_drawn(ops, device, script, T, length_penalty, min_len, steps):
    """tests/wide_cases.py::drive for ops.beam_update_drawn."""
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
        keys, vals, idx = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in drawn_step(script, t))
        ops.beam_update_drawn(keys, vals, idx, bs)
        snap = {n: getattr(bs, n).cpu().numpy().reshape(getattr(bs, n).shape).copy() for n in STATE}
        bpt, bpp = bs.bp_tok.cpu().numpy().copy(), bs.bp_par.cpu().numpy().copy()
        snap.update(bp_tok=bpt[min(t, T - 1)], bp_par=bpp[min(t, T - 1)])
        snaps.append(snap)
    return snaps, bs


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("nb", [2, 5, 6, 16])
def test_drawn_beam_update_follows_beam_state_after_every_step(ops, nb, kind):
    """20 scripted steps (+ 2 calls after done) at B = 3: every state array after every step equals BeamState.update_drawn's and, bit
    for bit (fin_par / fin_tok too), the CPU double's; calls after done leave the state alone."""
    from beam_sample_ops import BeamSampleFakeOps
    from ps_slm_amd.decode import BeamState
    B, T, steps, lp, min_len = 3, 20, 22, KINDS[kind], 2
    script = Script(kind, B, nb, seed=nb)
    got, bs = drive_drawn(ops, "cuda", script, T, lp, min_len, steps)
    torch.cuda.synchronize()
    state = BeamState(B, nb, T, EOS, EOS, lp, min_len)
    n_steps = 0
    for t in range(steps):
        s = got[t]
        if state.done:
            for name, arr in got[t - 1].items():
                if name not in ("bp_tok", "bp_par"):
                    assert np.array_equal(arr, s[name]), (t, name, "a call after done changed the state")
            continue
        keys, vals, idx = drawn_step(script, t)
        tok, par = state.update_drawn(keys.reshape(B, nb, -1), vals.reshape(B, nb, -1), idx.reshape(B, nb, -1))
        n_steps += 1
        for name, want in (("run_scores", state.run_scores), ("fin_scores", state.fin_scores), ("fin_len", state.fin_len),
                           ("is_fin", state.is_fin.astype(np.int64)), ("unsat", state.unsat.astype(np.int64)),
                           ("ctl", np.array([state.cur, int(state.done)])), ("next_ids", tok.reshape(-1)),
                           ("next_src", (np.arange(B)[:, None] * nb + par).reshape(-1)), ("bp_tok", tok), ("bp_par", par),
                           ("next_slot", np.full(B * nb, 5 + t)), ("next_lens", np.full(B * nb, 5 + t + 1)),
                           ("next_pos", np.repeat(s["valid"] + t, nb)), ("banned", np.array([EOS if state.cur < 2 else -1]))):
            assert s[name].shape == np.asarray(want).shape and np.array_equal(s[name], want), (t, name, s[name], want)
    assert 2 <= n_steps <= T and same(bs.result(EOS).numpy(), state.result())
    fake, _ = drive_drawn(BeamSampleFakeOps(), "cpu", script, T, lp, min_len, steps)
    for t in range(steps):
        for name, arr in fake[t].items():
            assert np.array_equal(arr, got[t][name]), (t, name, arr, got[t][name])


# ------------------------------------------------------------------------------------------ 3. end to end, mid geometry
@pytest.fixture(scope="module")
def fixture(ops):
    from ps_slm_amd.model import TasuModel
    geo, sd, cases = beam_sample_cases()
    gm = TasuModel(geo, ops, "cuda")
    gm.llm.keep_f32 = True                                    # what model_factory does for train_config.use_fp16 = false
    gm.arith = "fp32"
    gm.load_reference_state_dict(sd)
    return geo, cases, gm


def gen(gm, geo, c, fp32, graphs=True, manual_seed=None, **over):
    from ps_slm_amd.decode import beam_search_generate, check_sampling
    from ps_slm_amd.decode_fp32 import beam_search_generate_fp32
    kw = dict(c["kw"], **over)
    kw.update(sampling=check_sampling(kw.pop("temperature"), kw.pop("top_k"), kw.pop("top_p")))
    st = gm.prepare_text(c["ids"], c["am"], None, c["post_ids"], None, None)
    keep, gm.decode_graphs = gm.decode_graphs, graphs
    torch.manual_seed(c["manual_seed"] if manual_seed is None else manual_seed)
    try:
        if fp32:
            out = beam_search_generate_fp32(gm, st, eos_token_id=geo.eos_id, pad_token_id=geo.eos_id, **kw).numpy()
        else:
            gm.forward_projector_text(st)
            out = beam_search_generate(gm, st, eos_token_id=geo.eos_id, pad_token_id=geo.eos_id, **kw).numpy()
    finally:
        gm.decode_graphs = keep
    if manual_seed is None:
        assert int(gm._last_beam.seed[0]) == c["seed"]
    return out


def test_fp32_path_equals_the_reference_on_every_fp32_stable_case(fixture):
    """use_fp16 = false: token-exact on every fp32_stable case; on EVERY case decode graphs on and off give the same tokens."""
    geo, cases, gm = fixture
    assert gm.decode_graphs
    bad, differ, exact = [], [], 0
    for n, c in enumerate(cases):
        t = gen(gm, geo, c, True)
        exact += int(same(t, c["tokens"]))
        if c["fp32_stable"] and not same(t, c["tokens"]):
            bad.append((n, c["kw"], t.tolist(), c["tokens"].tolist()))
        if not same(gen(gm, geo, c, True, graphs=False), t):
            differ.append(n)
    print(f"fp32 path: {exact} / {len(cases)} cases exact ({sum(c['fp32_stable'] for c in cases)} flagged stable)")
    assert not bad, bad
    assert not differ, differ


def test_bf16_path_equals_the_reference_on_every_bf16_stable_case(fixture):
    """The bf16 path: token-exact on every bf16_stable case (the flag is the restatement's); on EVERY case decode graphs on and off
    give the same tokens."""
    geo, cases, gm = fixture
    bad, differ, exact = [], [], 0
    for n, c in enumerate(cases):
        t = gen(gm, geo, c, False)
        exact += int(same(t, c["tokens"]))
        if c["bf16_stable"] and not same(t, c["tokens"]):
            bad.append((n, c["kw"], t.tolist(), c["tokens"].tolist()))
        if not same(gen(gm, geo, c, False, graphs=False), t):
            differ.append(n)
    print(f"bf16 path: {exact} / {len(cases)} cases exact ({sum(c['bf16_stable'] for c in cases)} flagged stable)")
    assert not bad, bad
    assert not differ, differ


@pytest.mark.parametrize("fp32", [True, False])
def test_manual_seed_reproduces_a_call_and_other_seeds_differ(fixture, fp32):
    geo, cases, gm = fixture
    c = next(c for c in cases if c["kw"]["top_k"] == 50 and c["kw"]["num_beams"] == 4 and c["kw"]["top_p"] == 1.0)
    a = gen(gm, geo, c, fp32)
    assert same(a, gen(gm, geo, c, fp32))                                                  # the graph captured by the first call, replayed
    assert any(not same(a, gen(gm, geo, c, fp32, manual_seed=c["manual_seed"] + 1 + i)) for i in range(4))


def test_plugin_generate_at_the_default_four_beams_returns_tokens(ops):
    """The reference's own keyword set, ``generate(**batch, do_sample=True, top_p=0.9)``: num_beams defaults to 4."""
    from ps_slm_amd.config import ModelConfig, TrainConfig
    from ps_slm_amd.ps_slm import model_factory
    from ps_slm_amd.synthetic import synthetic_text_batch
    tc = TrainConfig(freeze_llm=True, freeze_encoder=True, gt_emb=True, gt_emb_noise=False, ctc_posterior=True, do_psd=True)
    mc = ModelConfig(llm_path="synthetic:mid", encoder_projector="linear-silu", llm_dim=256)
    model, _ = model_factory(tc, mc, device="cuda", ops=ops, init_seed=1234)
    raw = synthetic_text_batch(model.core.geo, 2, seed=3, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=8, noise=False)
    call = dict(input_ids=raw["input_ids"], attention_mask=raw["attention_mask"], input_features=raw["input_features"],
                input_feature_length=raw["input_feature_length"], targets=["ab cd"] * 2)
    model.eval()
    torch.manual_seed(3)
    out = model.generate(**call, max_new_tokens=6, do_sample=True, top_p=0.9)
    assert out.shape[0] == 2 and 1 <= out.shape[1] <= 6 and model.core._last_beam.nb == 4
    torch.manual_seed(3)
    assert same(model.generate(**call, max_new_tokens=6, do_sample=True, top_p=0.9).numpy(), out.numpy())
