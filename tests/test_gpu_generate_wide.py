"""generate(num_beams = 5 .. 16) on the GPU: the four top-k entry points at k up to 32 against a float64 restatement, the wide beam
update (csrc/beam.hip::beam_update_wide_kernel) against BeamState and the CPU double after every step of scripted candidate
streams, the wide history kernel against numpy, and the decode paths end to end against the REAL reference's tokens
(tests/golden/mid_generate_wide.npz)."""
import types

import numpy as np
import pytest
import torch

from penalty_ops import PenaltyFakeOps
from penalty_ref import same
from wide_cases import EOS, KINDS, Script, check_against_beam_state, drive, wide_cases

pytestmark = pytest.mark.gpu
I32 = torch.int32
NONE = 0x7fffffff
# the bars of the project's top-k tests (tests/test_gpu_generate_penalty.py): bf16 logits 1e-4, fp32 logits 2e-5
BAR = {torch.bfloat16: 1e-4, torch.float32: 2e-5}
KS = (10, 12, 14, 20, 24, 32)


@pytest.fixture(scope="module")
def ops():
    from ps_slm_amd.ops import HipOps
    return HipOps()


# ------------------------------------------------------------------------------------------ 1. the top-k kernels
def crafted(M, V, dtype, seed):
    """Logits [M, ld], histories and the banned id.  Background N(0, 1.5^2) capped at 3.  40 special columns -- column 0, column
    V - 1, one in each of the 16 column parts, the rest free -- hold 6.0, 6.25, ... (exact in bf16) in a per-row order; the banned
    column is the special that holds the LARGEST value in every row.  Row kinds, (r + M) % 5:
      0  as described;   4  the same, shifted by -16 (negative raw logits: mode 1 multiplies them);
      1  ties: 12 columns (column 0 and V - 1 among them) hold 20.0 -- the order among them is the column's;
      2  a constant row (every column ties at every threshold: the parts' overflow path); top-k = the first selectable columns;
      3  fewer than k finite columns: 7 finite (one of them the banned column), the rest -inf.
    Histories: length 0 / 1 / 37 by r % 3 (specials, repeats, background columns, the banned id)."""
    g = torch.Generator().manual_seed(seed)
    vec = 8 if dtype == torch.bfloat16 else 4
    part_cols = -(-(-(-V // vec)) // 16) * vec                          # columns per part, as the kernels split a row
    placed = [0, V - 1] + [p * part_cols + 5 for p in range(16) if 0 < p * part_cols + 5 < V - 1]
    free = [c for c in torch.randperm(V - 2, generator=g)[:80].add(1).tolist() if c not in placed][:40 - len(placed)]
    special = placed + free
    assert len(special) == 40 and len(set(special)) == 40
    ban = placed[7]
    x = (torch.randn(M, V, generator=g) * 1.5).clamp(max=3.0)
    hist = torch.randint(0, V, (M, 64), generator=g, dtype=torch.int32)
    hl = torch.zeros(M, dtype=torch.int32)
    for r in range(M):
        kind = (r + M) % 5
        order = torch.randperm(len(special) - 1, generator=g).tolist()
        others = [c for c in special if c != ban]
        x[r, torch.tensor(others)] = 6.0 + 0.25 * torch.tensor(order, dtype=torch.float32)
        x[r, ban] = 6.0 + 0.25 * 39
        if kind == 4:
            x[r] -= 16.0
        elif kind == 1:
            x[r, torch.tensor(placed[:2] + free[:10])] = 20.0
        elif kind == 2:
            x[r] = 1.5
        elif kind == 3:
            keep = torch.tensor([ban] + others[:6])
            vals = x[r, keep].clone()
            x[r] = float("-inf")
            x[r, keep] = vals
        if r % 3 == 1:
            hist[r, 0], hl[r] = others[order.index(38)], 1             # the row's best selectable special
        elif r % 3 == 2:
            back = torch.randint(0, V, (8,), generator=g).tolist()
            h = (placed + placed[:6] + back + [ban, 0, V - 1] + free)[:37]
            hist[r, :37], hl[r] = torch.tensor(h, dtype=torch.int32), 37
    ld = -(-V // 64) * 64 if dtype == torch.bfloat16 else V             # the decode buffers' padded leading dimension
    lg = torch.zeros(M, ld, dtype=dtype)
    lg[:, :V] = x.to(dtype)
    return lg.cuda(), hist.cuda(), hl.cuda(), torch.tensor([ban], dtype=torch.int32).cuda()


def reference(lg, V, hist, hl, banned, p, mode):
    """float64 (on the device): HF's rule once per distinct history token -- on the raw logits (mode 1) or on the log-probs (mode 0),
    ``p`` None: no penalty -- then the ban; sorted (value descending, column ascending): (values, columns) [M, 33]."""
    x = lg[:, :V].double()
    pen = lambda s: torch.where(s < 0, s * p, s / p)  # noqa: E731
    hs = [hist[r, :int(hl[r])].long().unique() for r in range(x.shape[0])] if p is not None else []
    if mode == 1:
        for r, h in enumerate(hs):
            x[r, h] = pen(x[r, h])
    lp = x - torch.logsumexp(x, -1, keepdim=True)
    if mode == 0:
        for r, h in enumerate(hs):
            lp[r, h] = pen(lp[r, h])
    lp[:, banned.long()] = float("-inf")
    v, i = torch.sort(lp, dim=-1, descending=True, stable=True)
    v, i = v[:, :33], i[:, :33]
    return v, torch.where(torch.isinf(v), torch.full_like(i, NONE), i)


def check_topk(call, lg, V, banned, want_v, want_i, k, bar, tag):
    M = lg.shape[0]
    gaps = want_v[:, :k] - want_v[:, 1:k + 1]
    gaps = gaps[torch.isfinite(gaps) & (gaps != 0)]
    assert gaps.numel() == 0 or float(gaps.min()) > bar, (tag, float(gaps.min()), "unequal crafted scores must be further apart than the bar")
    val = torch.full((M, k), 7.0, device="cuda")
    idx = torch.full((M, k), -7, dtype=I32, device="cuda")
    ws = torch.full((M * 16 * (2 + 2 * k),), float("nan"), device="cuda")
    call(k, val, idx, ws)
    torch.cuda.synchronize()
    assert torch.equal(idx.long(), want_i[:, :k]), (tag, k, [(r, idx[r].tolist(), want_i[r, :k].tolist()) for r in range(M)
                                                             if not torch.equal(idx[r].long(), want_i[r, :k])][:2])
    fin = torch.isfinite(want_v[:, :k])
    assert torch.equal(torch.isfinite(val), fin), (tag, k)
    err = float((val.double() - want_v[:, :k])[fin].abs().max())
    print(f"{tag} k={k}: max |value - float64| = {err:.3g} (bar {bar:g})")
    assert err < bar, (tag, k, err)
    assert int(banned[0]) not in set(idx.flatten().tolist())


@pytest.mark.parametrize("M", [1, 3, 70])
@pytest.mark.parametrize("V", [1000, 151936])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_plain_topk_kernels_vs_float64(ops, dtype, V, M):
    """tasu_logprob_topk / tasu_f32_logprob_topk.  V = 1000: 16 parts of ~63 columns hold fewer than k = 32 selectable columns each.
    (k = 10 on bf16 logits is the unpenalised five-beam width that had no instantiation.)"""
    lg, hist, hl, banned = crafted(M, V, dtype, seed=31)
    want_v, want_i = reference(lg, V, hist, hl, banned, None, -1)
    for k in KS:
        def call(k, val, idx, ws):
            if dtype == torch.bfloat16:
                ops.topk_ws[:ws.numel()] = ws
                ops.logprob_topk(lg, M, V, k, banned, 1, val, idx)
            else:
                ops.f32_logprob_topk(lg, M, V, k, banned, 1, val, idx, ws=ws)
        check_topk(call, lg, V, banned, want_v, want_i, k, BAR[dtype], f"{dtype} M={M} V={V}")


def test_plain_topk_bf16_part_longer_than_the_register_window(ops):
    """tasu_logprob_topk at V = 196,672: 16 parts of 1537 chunks of 8 columns, one more than the 256 x 6 chunks the part scan holds
    in registers, so the first 15 parts take the per-thread lists (csrc/topk.hip::topk_part_lists) for the whole part, the loop past
    the register window included; the last part holds the remaining 1529 chunks and runs the threshold form.  M = 5: every row kind of ``crafted``, the constant row and the row with fewer than k finite columns among them."""
    M, V = 5, 196672
    lg, hist, hl, banned = crafted(M, V, torch.bfloat16, seed=31)
    assert lg.shape[1] == V and -(-(-(-V // 8)) // 16) == 256 * 6 + 1
    want_v, want_i = reference(lg, V, hist, hl, banned, None, -1)
    for k in (4, 10, 32):
        def call(k, val, idx, ws):
            ops.topk_ws[:ws.numel()] = ws
            ops.logprob_topk(lg, M, V, k, banned, 1, val, idx)
        check_topk(call, lg, V, banned, want_v, want_i, k, BAR[torch.bfloat16], f"bf16 long parts M={M} V={V}")


@pytest.mark.parametrize("M", [1, 3, 70])
@pytest.mark.parametrize("V", [1000, 151936])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_history_topk_kernels_vs_float64(ops, dtype, mode, V, M):
    """tasu_logprob_topk_hist / tasu_f32_logprob_topk_hist, penalty on the log-probs (mode 0) and on the raw logits (mode 1).  (Seed:
    the first from 32 on whose float64 reference keeps unequal penalised scores more than 4e-4 apart in every parametrisation; on the
    log-probs the gaps depend on the row's log-sum-exp.)"""
    lg, hist, hl, banned = crafted(M, V, dtype, seed=36)
    for p in (1.37, 0.71):
        want_v, want_i = reference(lg, V, hist, hl, banned, p, mode)
        for k in KS:
            def call(k, val, idx, ws):
                if dtype == torch.bfloat16:
                    ops.topk_ws[:ws.numel()] = ws
                    ops.logprob_topk_hist(lg, M, V, k, banned, 1, hist, hl, p, mode, val, idx)
                else:
                    ops.f32_logprob_topk_hist(lg, M, V, k, banned, 1, hist, hl, p, mode, val, idx, ws=ws)
            check_topk(call, lg, V, banned, want_v, want_i, k, BAR[dtype], f"{dtype} mode {mode} M={M} V={V} p={p}")


def test_topk_refuses_k_above_32(ops):
    from ps_slm_amd.ops import TasuOpError
    lg = torch.zeros(2, 1024, dtype=torch.bfloat16, device="cuda")
    lf = torch.zeros(2, 1024, device="cuda")
    hist, hl = torch.zeros(2, 8, dtype=I32, device="cuda"), torch.zeros(2, dtype=I32, device="cuda")
    val, idx, ban = torch.zeros(2, 34, device="cuda"), torch.zeros(2, 34, dtype=I32, device="cuda"), torch.zeros(1, dtype=I32, device="cuda")
    ws = torch.zeros(2 * 16 * 70, device="cuda")
    for k in (33, 34):
        for call in (lambda: ops.logprob_topk(lg, 2, 1000, k, ban, 1, val, idx),
                     lambda: ops.logprob_topk_hist(lg, 2, 1000, k, ban, 1, hist, hl, 1.3, 0, val, idx),
                     lambda: ops.f32_logprob_topk(lf, 2, 1000, k, ban, 1, val, idx, ws=ws),
                     lambda: ops.f32_logprob_topk_hist(lf, 2, 1000, k, ban, 1, hist, hl, 1.3, 0, val, idx, ws=ws)):
            with pytest.raises(TasuOpError):
                call()


# ------------------------------------------------------------------------------------------ 2. the beam update
def beam_update_case(ops, kind, nb, B):
    T, steps, lp, min_len = 20, 22, KINDS[kind], 2
    from ps_slm_amd.decode import BeamState
    script = Script(kind, B, nb, seed=nb)
    got, bs = drive(ops, "cuda", script, T, lp, min_len, steps)
    torch.cuda.synchronize()
    state = BeamState(B, nb, T, EOS, EOS, lp, min_len)
    n_steps = check_against_beam_state(got, state, script, steps)
    assert same(bs.result(EOS).numpy(), state.result())
    fake, _ = drive(PenaltyFakeOps(), "cpu", script, T, lp, min_len, steps)           # fin_par / fin_tok too, bit for bit
    for t in range(steps):
        for name, arr in fake[t].items():
            assert np.array_equal(arr, got[t][name]), (t, name, arr, got[t][name])
    return n_steps


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("B", [1, 3, 17])
@pytest.mark.parametrize("nb", [6, 8, 16])
def test_wide_beam_update_follows_beam_state_after_every_step(ops, nb, B, kind):
    """20 scripted steps (+ 2 calls after done): equal scores across beams and tokens, EOS inside and outside the first nb, every
    candidate stopping (one utterance alone, then all), max_new reached, three length penalties (tests/wide_cases.py::Script).
    Every state array after every step equals BeamState's and, bit for bit, the CPU double's."""
    n_steps = beam_update_case(ops, kind, nb, B)
    if kind == "sparse":
        assert n_steps == 20
    if kind == "allstop":
        assert n_steps == (12 if B == 1 else 14)


@pytest.mark.parametrize("nb", [1, 2, 3, 4, 5])
def test_narrow_beam_update_through_the_same_entry_point_is_unchanged(ops, nb):
    """nb 1..5 run today's one-wave kernel: the same streams, bit for bit the CPU double (the statement of that kernel) and BeamState."""
    for kind, B in (("sparse", 17), ("heavy", 3), ("allstop", 3)):
        beam_update_case(ops, kind, nb, B)


def test_beam_update_refuses_17_beams(ops):
    from ps_slm_amd.ops import TasuOpError
    script = Script("sparse", 1, 16, seed=1)
    _, bs = drive(ops, "cuda", script, 4, 1.0, 0, 1)
    bs.nb = 17
    v, i = torch.zeros(17, 34, device="cuda"), torch.zeros(17, 34, dtype=I32, device="cuda")
    with pytest.raises(TasuOpError):
        ops.beam_update(v, i, bs, False)


# ------------------------------------------------------------------------------------------ 3. the history kernel, every width
@pytest.mark.parametrize("nb", [1, 5, 6, 16])
def test_wide_history_kernel_follows_the_parents(ops, nb):
    """The rows are staged 512 positions at a time at every width: histories of 1, 2, 512, 513, 514, 1025 and 1300 positions (one, two and
    three passes), two rows of an utterance sharing a parent (nb > 1); columns past the history and a call after done stay untouched."""
    B, max_new = 3, 1300
    M = B * nb
    rng = np.random.default_rng(5)
    bs = types.SimpleNamespace(B=B, nb=nb, max_new=max_new, hist=torch.zeros((M, max_new), dtype=I32, device="cuda"),
                               hist_len=torch.zeros(M, dtype=I32, device="cuda"), ctl=torch.zeros(2, dtype=I32, device="cuda"),
                               next_src=torch.zeros(M, dtype=I32, device="cuda"), next_ids=torch.zeros(M, dtype=I32, device="cuda"))
    ref = rng.integers(0, 1000, (M, max_new)).astype(np.int32)
    bs.hist.copy_(torch.from_numpy(ref))
    for n in (1, 2, 512, 513, 514, 1025, 1300):
        par = rng.integers(0, nb, (B, nb))
        if nb > 1:
            par[:, 1] = par[:, 0]
        src = (np.arange(B)[:, None] * nb + par).reshape(-1)
        ids = rng.integers(0, 1000, M).astype(np.int32)
        new = ref.copy()
        new[:, :n - 1] = ref[src, :n - 1]
        new[:, n - 1] = ids
        ref = new
        bs.ctl.copy_(torch.tensor([n, 0], dtype=I32))
        bs.next_src.copy_(torch.from_numpy(src.astype(np.int32)))
        bs.next_ids.copy_(torch.from_numpy(ids))
        ops.beam_hist_update(bs)
        torch.cuda.synchronize()
        assert np.array_equal(bs.hist.cpu().numpy(), ref), n
        assert bs.hist_len.tolist() == [n] * M
    bs.ctl.copy_(torch.tensor([700, 1], dtype=I32))
    ops.beam_hist_update(bs)
    torch.cuda.synchronize()
    assert np.array_equal(bs.hist.cpu().numpy(), ref) and bs.hist_len.tolist() == [1300] * M


# ------------------------------------------------------------------------------------------ 4. end to end, mid geometry
@pytest.fixture(scope="module")
def fixture(ops):
    from ps_slm_amd.model import TasuModel
    geo, sd, cases = wide_cases()
    gm = TasuModel(geo, ops, "cuda")
    gm.llm.keep_f32 = True                                    # what model_factory does for train_config.use_fp16 = false
    gm.arith = "fp32"
    gm.load_reference_state_dict(sd)
    return geo, cases, gm


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
    """The bf16 path: token-exact on every bf16_stable case (the flag is the restatement's, tools/make_golden_generate_wide.py) -- 8
    and 16 beams and a penalised case among them; on EVERY case decode graphs on and off give the same tokens.  The unpenalised
    5-beam cases run tasu_logprob_topk at k = 10."""
    geo, cases, gm = fixture
    stable = [c["kw"] for c in cases if c["bf16_stable"]]
    assert len(stable) >= 10 and {8, 16} <= {k["num_beams"] for k in stable} and any(k["repetition_penalty"] != 1.0 for k in stable)
    bad, differ, exact = [], [], 0
    for n, c in enumerate(cases):
        t = gen(gm, geo, c, False)
        exact += int(same(t, c["tokens"]))
        if c["bf16_stable"] and not same(t, c["tokens"]):
            bad.append((n, c["kw"], t.tolist(), c["tokens"].tolist()))
        if not same(gen(gm, geo, c, False, graphs=False), t):
            differ.append(n)
    print(f"bf16 path: {exact} / {len(cases)} cases exact ({len(stable)} flagged stable)")
    assert not bad, bad
    assert not differ, differ


def test_72_rows_of_8_beams_equal_the_utterances_decoded_one_at_a_time(fixture):
    """9 utterances x 8 beams = 72 rows: the weight-streaming kernels run in two row chunks (64 + 8), the beam update in 9
    workgroups.  Row arithmetic does not depend on the batch a row sits in: EXACTLY the tokens of each utterance decoded alone."""
    from ps_slm_amd.decode import beam_search_generate
    from ps_slm_amd.synthetic import synthetic_text_batch
    geo, _, gm = fixture
    batch = synthetic_text_batch(geo, 9, seed=93, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=12, noise=False)
    ids, am = batch["input_ids"][:, :9], batch["attention_mask"][:, :9]

    def decode(rows):
        st = gm.prepare_text(ids[rows], am[rows], None, [batch["post_ids"][r] for r in rows], None, None)
        gm.forward_projector_text(st)
        return beam_search_generate(gm, st, num_beams=8, max_new_tokens=10).numpy()
    g_all = decode(list(range(9)))
    assert g_all.shape[0] == 9
    for r in range(9):
        one = decode([r])
        n = one.shape[1]
        assert np.array_equal(g_all[r, :n], one[0]) and (g_all[r, n:] == geo.eos_id).all(), (r, g_all[r], one)


def test_prologue_paths(fixture, ops, monkeypatch):
    """Above 5 beams a position starts with the five separate set-up launches (the fused prologue stages n_beams * ctx ints in LDS and
    stays at n_beams <= 5); at 5 beams the fused launch and the five launches decode the same tokens, and switching the fused
    launch off changes nothing at 8 beams."""
    geo, cases, gm = fixture
    assert ops.dec_prologue
    c5 = next(c for c in cases if c["kw"]["num_beams"] == 5)
    c8 = next(c for c in cases if c["kw"]["num_beams"] == 8 and c["bf16_stable"])
    seen, now = [], []                                                    # (launch, n_beams) of every set-up launch
    chk, pro = ops._chk, ops.decode_step_prologue

    def spy_chk(rc, what):
        if now and what in ("tasu_decode_step_prologue", "tasu_kv_index_reorder"):
            seen.append((what, now[0]))
        return chk(rc, what)

    def spy_pro(*a):
        now[:] = [a[15]]
        try:
            return pro(*a)
        finally:
            now.clear()
    monkeypatch.setattr(ops, "_chk", spy_chk)
    monkeypatch.setattr(ops, "decode_step_prologue", spy_pro)
    t5, t8 = gen(gm, geo, c5, False, graphs=False), gen(gm, geo, c8, False, graphs=False)
    assert {("tasu_decode_step_prologue", 5), ("tasu_kv_index_reorder", 8)} == set(seen)
    monkeypatch.setattr(ops, "dec_prologue", False)
    del seen[:]
    assert same(gen(gm, geo, c5, False, graphs=False), t5) and same(gen(gm, geo, c8, False, graphs=False), t8)
    assert {("tasu_kv_index_reorder", 5), ("tasu_kv_index_reorder", 8)} == set(seen)
    assert same(t8, c8["tokens"])


def test_kv_cache_that_does_not_fit_is_refused_before_the_prefill(fixture, monkeypatch):
    from ps_slm_amd.decode import check_kv_cache_fits
    geo, cases, gm = fixture
    c = next(c for c in cases if c["kw"]["num_beams"] == 16)
    need = check_kv_cache_fits(gm, 2, 16, 64, 2, ("dec_kc", "dec_vc"))
    assert need == geo.llm_layers * 2 * 16 * 64 * geo.llm_kv_heads * 128 * 2 * 2
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a: (0, 1 << 40))
    monkeypatch.setattr(torch.cuda, "memory_reserved", lambda *a: 0)
    monkeypatch.setattr(torch.cuda, "memory_allocated", lambda *a: 0)
    called = []
    monkeypatch.setattr(gm, "forward_llm", lambda *a, **k: called.append(1))
    big = dict(c, kw=dict(c["kw"], max_new_tokens=1500))                  # larger than any cache the module has grown
    for fp32 in (False, True):
        with pytest.raises(ValueError, match=r"num_beams=16 x \d+ utterances at context \d+: the KV cache takes \d+ bytes"):
            gen(gm, geo, big, fp32)
    assert not called
