"""generate(repetition_penalty = p) on the GPU (csrc/topk.hip, csrc/beam.hip): the history top-k kernels against a float64 restatement, the
history kernel against numpy (eager and under one captured-and-replayed graph), and the decode paths end to end against the REAL
reference's tokens (tests/golden/mid_generate_penalty.npz)."""
import types

import numpy as np
import pytest
import torch

from penalty_ref import penalty_cases, same, tokens_on_weights

pytestmark = pytest.mark.gpu
I32 = torch.int32
# the bars of the unpenalised kernels' own tests: tests/test_gpu_ops.py (bf16 logits, 1e-4) and tests/test_gpu_fp32_ops.py (2e-5)
BAR = {torch.bfloat16: 1e-4, torch.float32: 2e-5}


@pytest.fixture(scope="module")
def ops():
    from ps_slm_amd.ops import HipOps
    return HipOps()


# ------------------------------------------------------------------------------------------ 1. the top-k kernels
def crafted(M, V, dtype, seed):
    """Logits, histories and the banned id of the kernel test.  Background: N(0, 1.5^2) capped at 3; 24 special columns per row
    hold 6.0, 6.25, ... in a per-row order (a quarter apart: exact in bf16; with p = 1.37 or 0.71 two of them are at least
    1 / (16 * 137) = 4.6e-4 apart after the penalty on raw logits -- 100 n = 137 m has no solution on the grid; on log-probs the
    gaps depend on the row's lse, and the test asserts on the float64 reference that they exceed the bar).  ODD rows are shifted by
    -16, so their specials are NEGATIVE raw logits (mode 1 multiplies them, and divides the even rows').  Specials: column 0, column V - 1, one column in each of the 16 column parts and
    6 free ones.  History lengths 0, 1, 37 by row: length 1 = the row's unpenalised argmax; length 37 = the 18 placed specials (the
    argmax and the banned id among them), repeats of them, and background columns; entries past the length are valid ids that must
    be ignored."""
    g = torch.Generator().manual_seed(seed)
    vec = 8 if dtype == torch.bfloat16 else 4
    n_chunks = -(-V // vec)
    part_cols = -(-n_chunks // 16) * vec                              # columns per part, as the kernels split a row
    placed = [0, V - 1] + [p * part_cols + 5 for p in range(16) if p * part_cols + 5 < V - 1]
    free = [c for c in torch.randperm(V - 2, generator=g)[:40].add(1).tolist() if c not in placed][:6]
    special = placed + free
    x = (torch.randn(M, V, generator=g) * 1.5).clamp(max=3.0)
    hist = torch.randint(0, V, (M, 64), generator=g, dtype=torch.int32)
    hl = torch.zeros(M, dtype=torch.int32)
    banned = torch.tensor([placed[7]], dtype=torch.int32)
    for r in range(M):
        order = torch.randperm(len(special), generator=g).tolist()
        vals = 6.0 + 0.25 * torch.arange(len(special), dtype=torch.float32)
        x[r, torch.tensor(special)] = vals[torch.tensor(order)]
        top = special[order.index(len(special) - 1)]                   # the row's unpenalised argmax
        if r % 2:
            x[r] -= 16.0
        if r % 3 == 1:
            hist[r, 0], hl[r] = top, 1
        elif r % 3 == 2:
            back = torch.randint(0, V, (8,), generator=g).tolist()
            h = placed + [top] + placed[:5] + back + [placed[7], top, placed[0], 0, V - 1]
            h = (h + placed)[:37]
            hist[r, :37], hl[r] = torch.tensor(h, dtype=torch.int32), 37
    ld = -(-V // 64) * 64 if dtype == torch.bfloat16 else V             # the decode buffers' padded leading dimension
    lg = torch.zeros(M, ld, dtype=dtype)
    lg[:, :V] = x.to(dtype)
    return lg.cuda(), hist.cuda(), hl.cuda(), banned.cuda()


def reference(lg, V, hist, hl, banned, p, mode):
    """float64: HF's rule once per distinct history token -- on the raw logits (mode 1) or on the log-probs (mode 0) -- then the ban."""
    x = lg[:, :V].double()
    hs = [hist[r, :int(hl[r])].long().unique() for r in range(x.shape[0])]
    pen = lambda s: torch.where(s < 0, s * p, s / p)  # noqa: E731
    if mode == 1:
        for r, h in enumerate(hs):
            x[r, h] = pen(x[r, h])
    lp = x - torch.logsumexp(x, -1, keepdim=True)
    if mode == 0:
        for r, h in enumerate(hs):
            lp[r, h] = pen(lp[r, h])
    lp[:, banned.long()] = float("-inf")
    return lp


@pytest.mark.parametrize("M,V", [(5, 1000), (64, 151936)])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_history_topk_kernels_vs_float64(ops, dtype, mode, M, V):
    lg, hist, hl, banned = crafted(M, V, dtype, seed=21)
    assert sorted(set(hl.tolist())) == [0, 1, 37]
    bar = BAR[dtype]
    for p in (1.37, 0.71):
        lp = reference(lg, V, hist, hl, banned, p, mode)
        for k in (2, 8, 10):
            want_v, want_i = torch.topk(lp, k + 1, dim=-1)
            gaps = (want_v[:, :-1] - want_v[:, 1:]).min()
            assert float(gaps) > bar, (float(gaps), "the crafted scores must be further apart than the bar")
            val = torch.full((M, k), 7.0, device="cuda")
            idx = torch.full((M, k), -7, dtype=I32, device="cuda")
            ws = torch.full((M * 16 * (2 + 2 * k),), float("nan"), device="cuda")
            if dtype == torch.bfloat16:
                ops.topk_ws[:ws.numel()] = ws
                ops.logprob_topk_hist(lg, M, V, k, banned, 1, hist, hl, p, mode, val, idx)
            else:
                ops.f32_logprob_topk_hist(lg, M, V, k, banned, 1, hist, hl, p, mode, val, idx, ws=ws)
            torch.cuda.synchronize()
            assert torch.equal(idx.long(), want_i[:, :k]), (p, k, idx[:3], want_i[:3, :k])
            err = float((val.double() - want_v[:, :k]).abs().max())
            print(f"{dtype} mode {mode} M={M} V={V} p={p} k={k}: max |value - float64| = {err:.3g} (bar {bar:g}), min gap {float(gaps):.3g}")
            assert err < bar, (p, k, err)
            assert all(len(set(row)) == k for row in idx.tolist())            # a token appears at most once
            assert int(banned[0]) not in set(idx.flatten().tolist())


def test_history_topk_rejects_bad_arguments(ops):
    lg = torch.zeros(2, 1024, dtype=torch.bfloat16, device="cuda")
    hist, hl = torch.zeros(2, 8, dtype=I32, device="cuda"), torch.zeros(2, dtype=I32, device="cuda")
    val, idx, ban = torch.zeros(2, 4, device="cuda"), torch.zeros(2, 4, dtype=I32, device="cuda"), torch.zeros(1, dtype=I32, device="cuda")
    from ps_slm_amd.ops import TasuOpError
    for p, mode in ((0.0, 0), (-1.0, 1), (1.3, 2)):
        with pytest.raises(TasuOpError):
            ops.logprob_topk_hist(lg, 2, 1000, 4, ban, 1, hist, hl, p, mode, val, idx)


# ------------------------------------------------------------------------------------------ 2. the history kernel
@pytest.mark.parametrize("graph", [False, True])
def test_history_kernel_follows_the_parents(ops, graph):
    """M = 12 rows (3 utterances x 4 beams), 20 scripted steps; every step two rows of an utterance share a parent."""
    B, nb, max_new, steps = 3, 4, 24, 20
    M = B * nb
    rng = np.random.default_rng(3)
    bs = types.SimpleNamespace(B=B, nb=nb, max_new=max_new, hist=torch.full((M, max_new), -5, dtype=I32, device="cuda"),
                               hist_len=torch.zeros(M, dtype=I32, device="cuda"), ctl=torch.zeros(2, dtype=I32, device="cuda"),
                               next_src=torch.zeros(M, dtype=I32, device="cuda"), next_ids=torch.zeros(M, dtype=I32, device="cuda"))
    ref = np.full((M, max_new), -5, dtype=np.int64)
    g = None
    for t in range(steps):
        par = rng.integers(0, nb, (B, nb))
        par[:, 1] = par[:, 0]                                             # two rows share a parent
        src = (np.arange(B)[:, None] * nb + par).reshape(-1)
        ids = rng.integers(0, 1000, M)
        new = ref[src].copy()
        new[:, t] = ids
        ref = new
        bs.ctl.copy_(torch.tensor([t + 1, 0], dtype=I32))
        bs.next_src.copy_(torch.from_numpy(src.astype(np.int32)))
        bs.next_ids.copy_(torch.from_numpy(ids.astype(np.int32)))
        if not graph or t == 0:
            ops.beam_hist_update(bs)                                      # (eager first: nothing lazy inside a capture)
        elif g is None:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                ops.beam_hist_update(bs)
            g.replay()
        else:
            g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bs.hist.cpu().numpy()[:, :t + 1], ref[:, :t + 1]), t
        assert bs.hist_len.tolist() == [t + 1] * M
    before = bs.hist.clone()
    bs.ctl.copy_(torch.tensor([steps + 1, 1], dtype=I32))                 # done: a no-op
    ops.beam_hist_update(bs)
    torch.cuda.synchronize()
    assert torch.equal(bs.hist, before) and bs.hist_len.tolist() == [steps] * M


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
    geo, sd, cases = penalty_cases()
    return geo, cases, fp32_model(geo, sd, ops)


def gen(gm, geo, c, fp32, graphs=True, **over):
    from ps_slm_amd.decode import beam_search_generate
    from ps_slm_amd.decode_fp32 import beam_search_generate_fp32
    st = gm.prepare_text(c["ids"], c["am"], None, c["post_ids"], None, None)
    keep, gm.decode_graphs = gm.decode_graphs, graphs
    try:
        if fp32:
            return beam_search_generate_fp32(gm, st, eos_token_id=geo.eos_id, pad_token_id=geo.eos_id, **dict(c["kw"], **over)).numpy()
        gm.forward_projector_text(st)
        return beam_search_generate(gm, st, eos_token_id=geo.eos_id, pad_token_id=geo.eos_id, **dict(c["kw"], **over)).numpy()
    finally:
        gm.decode_graphs = keep


def test_fp32_path_equals_the_reference_on_every_case(fixture):
    """use_fp16 = false: token-exact on all fixture cases, none skipped; decode graphs on and off give the same tokens."""
    geo, cases, gm = fixture
    assert gm.decode_graphs
    bad, differ = [], []
    for n, c in enumerate(cases):
        t = gen(gm, geo, c, True)
        if not same(t, c["tokens"]):
            bad.append((n, c["kw"], t.tolist(), c["tokens"].tolist()))
        if not same(gen(gm, geo, c, True, graphs=False), t):
            differ.append(n)
    assert not bad, bad
    assert not differ, differ


def test_bf16_path_equals_the_reference_on_every_stable_case(fixture):
    """The bf16 path: token-exact on every bf16_stable case (the flag is the restatement's, tools/make_golden_generate_penalty.py);
    on EVERY case decode graphs on and off give the same tokens."""
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


def test_lora_merged_model_in_fp32_equals_the_restatement_on_the_merged_weights(ops):
    """One adapted-decoder case (generate() runs on the merged W + s B A): the first case of mid_generate_lora_margin.npz, at p = 1.3,
    on which the restatement decodes the same tokens from the float32 and the float64 merged weights (a case that flips between the
    two is a near-tie no fp32 implementation can be held to)."""
    from conftest import decode_lora_margin_cases
    from fp32_oracle_cases import lora_merged_double
    geo, cfg, sd, lsd, cases = decode_lora_margin_cases()
    W64 = lora_merged_double(sd, lsd, cfg)
    for c in cases:
        kw = dict(c["kw"], repetition_penalty=1.3)
        t32 = tokens_on_weights(W64, geo, c["ids"], c["am"], c["post_ids"], kw, torch.float32)
        t64 = tokens_on_weights(W64, geo, c["ids"], c["am"], c["post_ids"], kw, torch.float64)
        if same(t32, t64) and not same(t64, c["tokens"]):              # (and the penalty changes what the case decodes)
            break
    else:
        pytest.fail("no case on which the restatement's float32 and float64 runs agree")
    gm = fp32_model(geo, sd, ops, cfg, lsd)
    t = gen(gm, geo, dict(c, kw=kw), True)
    assert same(t, t64), (t.tolist(), t64.tolist())


def test_penalty_one_is_the_call_without_the_argument(ops):
    from conftest import decode_fp32_cases
    geo, sd, cases, _ = decode_fp32_cases()
    gm = fp32_model(geo, sd, ops)
    for c in cases[:3]:
        for fp32 in (True, False):
            assert same(gen(gm, geo, c, fp32), gen(gm, geo, c, fp32, repetition_penalty=1.0))
        assert same(gen(gm, geo, c, True), c["tokens"])
