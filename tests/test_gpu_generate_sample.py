"""generate(do_sample=True, num_beams=1) on the GPU (csrc/sample.hip): the uniform kernel bit for bit against integer numpy (eager and
under one captured-and-replayed graph), the row samplers against the float64 restatement and its derived bound
(tests/sample_ref64.py), an exact case (tie rule, id order and RNG in one assertion), argument rejection, and the decode paths end
to end against the REAL reference's tokens (tests/golden/mid_generate_sample.npz)."""
import numpy as np
import pytest
import torch

import sample_ref64 as R64
from sample_ref import draw_seed, same, sample_cases, sampled_tokens_on_weights

pytestmark = pytest.mark.gpu
I32 = torch.int32
POOL = 1024
NONE = 0x7fffffff


@pytest.fixture(scope="module")
def ops():
    from ps_slm_amd.ops import HipOps
    return HipOps()


# ------------------------------------------------------------------------------------------ 1. the uniform kernel
@pytest.mark.parametrize("M", [1, 3, 256])
def test_uniform_kernel_is_the_integer_restatement_bit_for_bit(ops, M):
    for seed in (0, 12345678901234567, -3, 2 ** 63 - 1, -2 ** 63):
        sd = torch.tensor([seed], dtype=torch.int64, device="cuda")
        for t in (0, 1, 199):
            ctl = torch.tensor([t, 0], dtype=I32, device="cuda")
            u = torch.full((M + 2,), -7.0, device="cuda")
            ops.sample_uniform(sd, ctl, M, u)
            torch.cuda.synchronize()
            got = u.cpu().numpy()
            assert np.array_equal(got[:M].view(np.int32), R64.uniforms(seed, t, M).view(np.int32)), (seed, t)
            assert (got[M:] == -7.0).all()


def test_uniform_kernel_draws_fresh_numbers_under_graph_replay(ops):
    """Seed and counter are device words: ONE captured launch gives position 5, 6, 7 and another call's seed on replay."""
    M, seed = 16, 987654321987
    sd = torch.tensor([seed], dtype=torch.int64, device="cuda")
    ctl = torch.tensor([5, 0], dtype=I32, device="cuda")
    u = torch.zeros(M, device="cuda")
    ops.sample_uniform(sd, ctl, M, u)                                     # (eager first: nothing lazy inside a capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.sample_uniform(sd, ctl, M, u)
    for s, t in ((seed, 5), (seed, 6), (seed, 7), (-seed, 7)):
        sd.fill_(s)
        ctl[0] = t
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(u.cpu().numpy().view(np.int32), R64.uniforms(s, t, M).view(np.int32)), (s, t)


# ------------------------------------------------------------------------------------------ 2. the samplers against float64
U_GRID = [0.0, 1 - 2.0 ** -24] + [(i + 0.5) / 14 for i in range(14)]      # 16 values
ROWS = 16
PENALTY = 1.3


def sampler_inputs(V, dtype, seed):
    """16 rows of N(0, 2.5^2) logits in ``dtype``, histories of 0, 1 and 37 tokens by row (length 1: the row's argmax; 37: the row's
    eight best, repeats of them and background columns; entries past the length are valid ids that must be ignored), and one banned
    id: row 0's argmax."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(ROWS, V, generator=g) * 2.5).to(dtype)
    hist = torch.randint(0, V, (ROWS, 64), generator=g, dtype=I32)
    hl = torch.zeros(ROWS, dtype=I32)
    for r in range(ROWS):
        best = torch.topk(x[r].float(), 8)[1].tolist()
        if r % 3 == 1:
            hist[r, 0], hl[r] = best[0], 1
        elif r % 3 == 2:
            h = (best + best[:3] + torch.randint(0, V, (26,), generator=g).tolist())[:37]
            hist[r, :37], hl[r] = torch.tensor(h, dtype=I32), 37
    banned = torch.tensor([int(x[0].float().argmax())], dtype=I32)
    ld = -(-V // 64) * 64 if dtype == torch.bfloat16 else V             # the decode buffers' leading dimensions
    lg = torch.zeros(ROWS, ld, dtype=dtype)
    lg[:, :V] = x
    return x.float().numpy(), lg.cuda(), hist, hl, banned


@pytest.mark.parametrize("V", [1000, 151936])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_samplers_vs_float64(ops, dtype, V):
    """M in {1, 3, 16} x top_k in {1, 2, 50, pool} x top_p in {1.0, 0.9, 0.5} (T = 1.0, 0.7, 1.5 with them) x with / without history
    and ban; u on the 16-value grid (0 and 1 - 2^-24 included), shifted row by row over four launches.  Every token must be a
    float64 survivor with u Z inside [C_{i-1} - delta, C_i + delta] and its log-probability inside its bound; the filler slot is
    (-inf, 0x7fffffff); two launches give the same bits."""
    x, lg, hist, hl, banned = sampler_inputs(V, dtype, seed=31)
    hist_d, hl_d, ban_d, none_d = hist.cuda(), hl.cuda(), banned.cuda(), torch.tensor([-1], dtype=I32, device="cuda")
    fn = ops.sample_rows if dtype == torch.bfloat16 else ops.f32_sample_rows
    hists = [hist[r, :int(hl[r])].tolist() for r in range(ROWS)]
    rows_total = ambiguous = 0
    for with_hist in (False, True):
        for (top_p, T) in ((1.0, 1.0), (0.9, 0.7), (0.5, 1.5)):
            s = R64.scores32(x, hists if with_hist else None, banned.tolist() if with_hist else [], PENALTY if with_hist else 1.0, T)
            for top_k in (1, 2, 50, POOL):
                ref = [R64.Row(s[r], top_k, top_p) for r in range(ROWS)]
                rows_total += ROWS
                ambiguous += sum(r.ambiguous for r in ref)
                for M in (1, 3, 16):
                    for shift in range(4 if M == 16 else 2):
                        u = np.array([U_GRID[(5 * r + 4 * shift + M) % 16] for r in range(M)], dtype=np.float32)
                        u_d = torch.from_numpy(u).cuda()
                        outs = []
                        for _ in range(2):
                            val = torch.full((M + 1, 2), 7.0, device="cuda")
                            idx = torch.full((M + 1, 2), -7, dtype=I32, device="cuda")
                            fn(lg, M, V, u_d, ban_d if with_hist else none_d, 1, hist_d if with_hist else None, hl_d if with_hist else None,
                               PENALTY if with_hist else 1.0, T, top_k, top_p, val, idx)
                            torch.cuda.synchronize()
                            outs.append((val.cpu(), idx.cpu()))
                        (val, idx), (val2, idx2) = outs
                        assert torch.equal(idx, idx2) and torch.equal(val.view(I32), val2.view(I32))
                        assert idx[M].tolist() == [-7, -7] and val[M].tolist() == [7.0, 7.0]              # the guard row
                        assert idx[:M, 1].tolist() == [NONE] * M and (val[:M, 1] == float("-inf")).all()
                        for r in range(M):
                            why = ref[r].check(int(idx[r, 0]), u[r], float(val[r, 0]))
                            assert why is None, (dtype, V, with_hist, top_p, T, top_k, M, r, float(u[r]), why)
                            if u[r] == 0.0:                                # u = 0: the first survivor by id, whatever the weights
                                assert any(int(idx[r, 0]) == int(np.sort(ref[r].desc[:c])[0]) for c in ref[r].alternatives)
    print(f"{dtype} V={V}: {rows_total} reference rows, {ambiguous} with a top-p ratio inside the bound of its threshold")
    assert ambiguous <= 0.05 * rows_total, (ambiguous, rows_total)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_eight_tied_maxima_top_k_four_draws_the_floor_8u_th_by_id(ops, dtype):
    """Eight logits tied at the row's maximum, top_k = 4: HF keeps all eight (ties at the threshold stay), their weights are exactly
    1, the prefix sums exactly 1..8 and u Z = 8 u exactly, so the token is EXACTLY the floor(8 u)-th tied column in id order, u the
    uniform kernel's own output for (seed, position, row): tie rule, id order and RNG in one assertion."""
    V, M, seed = 151936, 256, -424242424242
    fn = ops.sample_rows if dtype == torch.bfloat16 else ops.f32_sample_rows
    g = torch.Generator().manual_seed(8)
    x = (torch.randn(M, V, generator=g) * 2).clamp(max=7.5)
    tied = []
    for r in range(M):
        cols = torch.randperm(V - 2, generator=g)[:8].add(1).tolist()             # odd rows: the first and the last column among them
        cols = sorted([0, V - 1] + cols[:6]) if r % 2 else sorted(cols)
        x[r, torch.tensor(cols)] = 9.0
        tied.append(cols)
    lg = x.to(dtype).cuda()
    sd = torch.tensor([seed], dtype=torch.int64, device="cuda")
    none_d = torch.tensor([-1], dtype=I32, device="cuda")
    for t in (0, 3, 199):
        ctl = torch.tensor([t, 0], dtype=I32, device="cuda")
        u_d = torch.zeros(M, device="cuda")
        val, idx = torch.zeros(M, 2, device="cuda"), torch.zeros(M, 2, dtype=I32, device="cuda")
        ops.sample_uniform(sd, ctl, M, u_d)
        fn(lg, M, V, u_d, none_d, 1, None, None, 1.0, 0.7, 4, 1.0, val, idx)
        torch.cuda.synchronize()
        u = R64.uniforms(seed, t, M).astype(np.float64)
        want = [tied[r][int(np.floor(8 * u[r]))] for r in range(M)]
        assert idx[:, 0].tolist() == want, t
        # (s - max) - logf(8) = -logf(8): logf's 1 ulp = 2 e |log 8|, the subtraction's e |log 8|
        assert float((val[:, 0].cpu().double() + np.log(8.0)).abs().max()) <= 3 * R64.e * np.log(8.0)
    assert len({i for i in idx[:, 0].tolist()}) > 100                     # (the rows do not all draw the same rank)


def test_samplers_reject_bad_arguments(ops):
    from ps_slm_amd.ops import TasuOpError
    lg = torch.zeros(2, 1024, dtype=torch.bfloat16, device="cuda")
    lf = torch.zeros(2, 1000, dtype=torch.float32, device="cuda")
    u = torch.zeros(257, device="cuda")
    hist, hl = torch.zeros(2, 8, dtype=I32, device="cuda"), torch.zeros(2, dtype=I32, device="cuda")
    val, idx, ban = torch.zeros(2, 2, device="cuda"), torch.zeros(2, 2, dtype=I32, device="cuda"), torch.zeros(1, dtype=I32, device="cuda")
    good = dict(M=2, V=1000, hist=None, hl=None, penalty=1.0, T=1.0, top_k=50, top_p=1.0)
    bad = [dict(top_k=0), dict(top_k=POOL + 1), dict(top_k=-1), dict(T=0.0), dict(T=-1.0), dict(T=float("inf")), dict(top_p=-0.1),
           dict(top_p=float("nan")), dict(M=0), dict(M=257), dict(V=0), dict(V=1025), dict(V=196609), dict(penalty=1.3),
           dict(hist=hist, hl=hl, penalty=0.0), dict(hist=hist, hl=None, penalty=1.3)]
    for fn, logits in ((ops.sample_rows, lg), (ops.f32_sample_rows, lf)):
        for over in [{}] + bad:
            a = dict(good, **over)
            call = lambda: fn(logits, a["M"], a["V"], u, ban, 1, a["hist"], a["hl"], a["penalty"], a["T"], a["top_k"], a["top_p"], val, idx)  # noqa: E731
            if over:
                with pytest.raises(TasuOpError):
                    call()
            else:
                call()
    with pytest.raises(TasuOpError):                                      # a leading dimension that is no multiple of the vector width
        ops.sample_rows(torch.zeros(2, 1004, dtype=torch.bfloat16, device="cuda"), 2, 1000, u, ban, 1, None, None, 1.0, 1.0, 50, 1.0, val, idx)
    with pytest.raises(TasuOpError):
        ops.f32_sample_rows(torch.zeros(2, 1002, device="cuda"), 2, 1000, u, ban, 1, None, None, 1.0, 1.0, 50, 1.0, val, idx)
    sd, ctl = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(2, dtype=I32, device="cuda")
    for M in (0, 257):
        with pytest.raises(TasuOpError):
            ops.sample_uniform(sd, ctl, M, u)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ 3. end to end, mid geometry
def fp32_model(geo, sd, ops, cfg=None, lsd=None):
    from ps_slm_amd.model import TasuModel
    gm = TasuModel(geo, ops, "cuda")
    gm.llm.keep_f32 = True                                    # what model_factory does for train_config.use_fp16 = false
    gm.arith = "fp32"
    gm.load_reference_state_dict(sd)
    if cfg is not None:
        gm.enable_lora(cfg)
        gm.lora.load_state_dict(lsd)
        gm.sync_projector_copies()
    return gm


@pytest.fixture(scope="module")
def fixture(ops):
    geo, sd, cases = sample_cases()
    return geo, cases, fp32_model(geo, sd, ops)


def gen(gm, geo, c, fp32, graphs=True, sampled=True, **over):
    from ps_slm_amd.decode import beam_search_generate, check_sampling
    from ps_slm_amd.decode_fp32 import beam_search_generate_fp32
    kw = dict(c["kw"], **over)
    T, top_k, top_p = kw.pop("temperature"), kw.pop("top_k"), kw.pop("top_p")
    kw.update(num_beams=1, sampling=check_sampling(T, top_k, top_p) if sampled else None)
    st = gm.prepare_text(c["ids"], c["am"], None, c["post_ids"], None, None)
    keep, gm.decode_graphs = gm.decode_graphs, graphs
    torch.manual_seed(c["manual_seed"])
    try:
        if fp32:
            out = beam_search_generate_fp32(gm, st, eos_token_id=geo.eos_id, pad_token_id=geo.eos_id, **kw).numpy()
        else:
            gm.forward_projector_text(st)
            out = beam_search_generate(gm, st, eos_token_id=geo.eos_id, pad_token_id=geo.eos_id, **kw).numpy()
    finally:
        gm.decode_graphs = keep
    if sampled:
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
    """The bf16 path: token-exact on every bf16_stable case (the flag is the restatement's, tools/make_golden_generate_sample.py); on
    EVERY case decode graphs on and off give the same tokens."""
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
def test_top_k_one_and_a_tiny_top_p_equal_greedy(fixture, ops, fp32):
    """top_p = 1e-6 keeps the largest only: the greedy decode.  top_k = 1 keeps every token TIED at the maximum (HF's rule), so it is
    the greedy decode unless a row's two best logits are equal at some position (bf16 logits: it happens) -- told by the logits the
    sampler received in an eager decode and left out.  No penalty and no ban here: the scores are the logits over T."""
    geo, cases, gm = fixture
    name = "f32_sample_rows" if fp32 else "sample_rows"
    orig, compared = getattr(ops, name), 0
    for c in cases[:8]:
        plain = dict(repetition_penalty=1.0, min_length=1)
        greedy = gen(gm, geo, c, fp32, sampled=False, **plain)
        assert same(gen(gm, geo, c, fp32, top_p=1e-6, **plain), greedy)
        tied = []

        def spy(lg, M, V, *a):
            top2 = torch.topk(lg[:M, :V].float(), 2, dim=-1)[0]
            tied.append(bool((top2[:, 0] == top2[:, 1]).any()))
            return orig(lg, M, V, *a)
        setattr(ops, name, spy)
        try:
            t = gen(gm, geo, c, fp32, graphs=False, top_k=1, **plain)
        finally:
            delattr(ops, name)
        if not any(tied):
            compared += 1
            assert same(t, greedy), (c["kw"], t.tolist(), greedy.tolist())
            assert same(gen(gm, geo, c, fp32, top_k=1, **plain), greedy)                  # ... and graph-replayed
    assert compared >= (8 if fp32 else 4)


def test_lora_merged_model_in_fp32_equals_the_restatement_on_the_merged_weights(ops):
    """One adapted-decoder case (generate() runs on the merged W + s B A): the first case of mid_generate_lora_margin.npz, sampled with
    top_k = 8, top_p = 0.9, T = 0.7, on which the restatement draws the same tokens from the float32 and the float64 merged weights
    (a case that flips between the two is a near-tie no fp32 implementation can be held to)."""
    from conftest import decode_lora_margin_cases
    from fp32_oracle_cases import lora_merged_double
    geo, cfg, sd, lsd, cases = decode_lora_margin_cases()
    W64 = lora_merged_double(sd, lsd, cfg)
    skw = dict(max_new_tokens=8, min_length=1, top_k=8, temperature=0.7, top_p=0.9, repetition_penalty=1.3)
    for n, c in enumerate(cases):
        manual_seed = 5100 + n
        seed = draw_seed(manual_seed)
        t32 = sampled_tokens_on_weights(W64, geo, c["ids"], c["am"], c["post_ids"], skw, seed, torch.float32)
        t64 = sampled_tokens_on_weights(W64, geo, c["ids"], c["am"], c["post_ids"], skw, seed, torch.float64)
        if same(t32, t64):
            break
    else:
        pytest.fail("no case on which the restatement's float32 and float64 runs agree")
    gm = fp32_model(geo, sd, ops, cfg, lsd)
    t = gen(gm, geo, dict(c, kw=skw, manual_seed=manual_seed, seed=seed), True)
    assert same(t, t64), (t.tolist(), t64.tolist())
