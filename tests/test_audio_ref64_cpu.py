"""CPU checks of the float64 references of the audio front end, the PSD plan and the merge kernels and of their allowances
(tests/audio_ref64.py), which tests/test_gpu_audio_f64.py holds the HIP kernels to:

* every case of the shared lists through the torch double (tests/fake_ops.py) under the same checks: the bits of the integer and
  data-movement outputs, 1.0 x E on the arithmetic ones, NaN / -7 guards.  For fbank the double takes its DFT in float64, so the
  numpy fp32 restatement of the kernel's own network (`fb_restatement_f32`: fp32 twiddles, fp32 butterflies) is held to E as well;
* the conditions on the inputs: the share of fbank elements with E <= 1e-4 (white noise at least 95 %, the golden waveform at
  least 80 %), no PSD segment mean within fp32 rounding of the threshold on any plan case or on the chain, the constructed
  threshold case exact; the case lists sit on the kernels' switches;
* the references are the operations: fbank against oracle/fbank_oracle.py, lfr_cmvn against its apply_lfr / apply_cmvn, the plan
  and the gather against oracle/tasu_oracle.py's psd(), rne_bf16 against torch's cast;
* the checks have teeth: the mutants of the issue, restated on the CPU, fail them (MUTANT lines).

Measured here (the AUDIO64 lines of this file; 150 tests, 6 s).  Largest |err| / E: fbank double 0.509, fp32 restatement 0.515
(both on the sine through the identity matrix), psd_gather 0.783, the chain 0.663, posterior_build 0.916 (one rounding of a / V);
lfr_cmvn, psd_frame_stats, psd_plan, embed_merge and merge_bwd are bits.  Share of fbank elements with E <= 1e-4: white noise
(12000 samples, 73 x 80) 95.7 %, median E 1.3e-5; golden waveform (12000 samples) 86.4 %, median E 3.6e-5 -- the lowest mel
bins after pre-emphasis and the floor-level frames are cancellation residues.  rms error over those elements, double / fp32
restatement: white noise 6.9e-7 / 1.1e-6, golden 9.3e-7 / 1.3e-6.  Smallest distance of a PSD segment mean from the threshold:
3.5e3 fp32 roundings over the plan cases, 1.9e4 on the chain.  Mutants (MUTANT lines): the window read one index off 2.1e3 E, mel
weights 0.1 % off 107 E (1.2e-3 under the old absolute measure, inside its 2e-3), bin 256 dropped 4.7e6 E through the identity
matrix and invisible (0.08 E) through the Kaldi matrix, whose Nyquist column is zero; a plan without the carried count or with a
forced start at frame 256, a gather that divides single frames only, a truncating cast: wrong bits; pad = lfr_m / 2 fails at
lfr_m = 4 and equals (lfr_m - 1) / 2 at 7 and 1; last-index ties: 7 wrong frame ids at V = 1000."""
import numpy as np
import pytest
import torch

import audio_ref64 as A
from fake_ops import FakeOps
from oracle import fbank_oracle as fo

F64, F32, BF, I32 = torch.float64, torch.float32, torch.bfloat16, torch.int32


@pytest.fixture(scope="module")
def fake():
    return FakeOps()


_worst = {}


def hold(op, what, got, ref):
    w = A.check(got, ref, f"{op} {what}")
    _worst[op] = max(_worst.get(op, 0.0), w)
    print(f"AUDIO64 {op} {what} |err| / E {w:.3f} (largest so far for {op}: {_worst[op]:.3f})")
    return w


# ------------------------------------------------------------------------------------------------ fbank
@pytest.fixture(scope="module")
def fb_refs():
    """(inputs, Ref) of every fbank case, computed once"""
    out = {}
    for c in A.FB_CASES:
        d = A.fb_inputs(c)
        out[c] = (d, A.fb_reference(d))
    return out


@pytest.mark.parametrize("case", A.FB_CASES, ids=A.case_id)
def test_fbank_double_and_fp32_restatement_inside_the_bound(fake, fb_refs, case):
    d, ref = fb_refs[case]
    got = A.run_fbank(fake, d)
    if d["T"] == 0:
        assert got["out"].shape[0] == 0 and not ref.tol
        return
    hold("fbank[double]", A.case_id(case), got, ref)
    f32 = {"out": A.fb_restatement_f32(d)}
    hold("fbank[fp32]", A.case_id(case), f32, ref)
    k, share = A.fb_sharp_rms(got["out"], ref)
    r, _ = A.fb_sharp_rms(f32["out"], ref)
    print(f"AUDIO64RMS fbank {A.case_id(case)}: share of E <= 1e-4 {100 * share:.1f} %, rms error there double {k:.2e}, fp32 restatement {r:.2e}")


def test_fbank_allowance_is_sharp_where_the_issue_asks(fb_refs):
    for c in A.FB_CASES:
        if c.n == 12000:
            E = fb_refs[c][1].tol["out"][1]
            share = float((E <= A.FB_SHARP).double().mean())
            print(f"AUDIO64SHARE fbank {c.wave}: {100 * share:.1f} % of {E.numel()} elements have E <= {A.FB_SHARP:g}, median E {float(E.median()):.2e}")
            assert share >= A.FB_SHARE[c.wave], (c.wave, share)


def test_fbank_reference_is_the_oracle_and_silence_is_the_floor(fb_refs):
    wave = np.load(A.GOLDEN)["wave"][:12000]
    c = next(c for c in A.FB_CASES if c.wave == "golden" and c.n == 12000)
    ref = fb_refs[c][1].tol["out"][0]
    assert float((ref - torch.from_numpy(fo.fbank(wave)).double()).abs().max()) < 1e-4       # the oracle frames in fp32
    s = next(c for c in A.FB_CASES if c.wave == "silence")
    want, E = fb_refs[s][1].tol["out"]
    assert bool((want == np.log(A.FLOOR)).all()) and float(E.max()) < 5e-6
    k = next(c for c in A.FB_CASES if c.wave == "const" and c.mel == "mel")
    want, E = fb_refs[k][1].tol["out"]
    assert bool((want == np.log(A.FLOOR)).all()) and float(E.min()) > 1e-4, "a constant frame: silent in float64, an honest residue in E"
    assert {c.win for c in A.FB_CASES} >= {255, 256, 257, 400, 512} and {c.n for c in A.FB_CASES} >= {399, 400, 401, 559, 560, 720, 12000}
    assert {c.shift for c in A.FB_CASES} >= {1, 160, 400} and {c.n_mels for c in A.FB_CASES} >= {1, 80, 257, 300}


def test_fbank_exact_properties_of_the_double(fake):
    c = next(c for c in A.FB_CASES if c.wave == "golden" and c.n == 12000)
    a = A.run_fbank(fake, A.fb_inputs(c))["out"]
    b = A.run_fbank(fake, A.fb_inputs(c, drop=3 * c.shift))["out"]
    A.same_bits(a[3:].contiguous(), b, "fbank with 3 hops dropped")
    s = A.run_fbank(fake, A.fb_inputs(next(c for c in A.FB_CASES if c.wave == "silence")))["out"]
    A.same_bits(s, torch.full_like(s, float(s[0, 0])), "silence")


# ------------------------------------------------------------------------------------------------ lfr_cmvn
@pytest.mark.parametrize("case", A.LFR_CASES, ids=A.case_id)
def test_lfr_cmvn_bits(fake, case):
    for T in A.LFR_T:
        d = A.lfr_inputs(case, T)
        ref = A.lfr_reference(d)
        hold("lfr_cmvn", f"{A.case_id(case)} T={T}", A.run_lfr(fake, d), ref)
        want = fo.apply_lfr(d["fb"][:T].numpy(), case.m, case.n)
        if case.cmvn:
            want = fo.apply_cmvn(want, d["means"].numpy(), d["scales"].numpy())
        A.same_bits(ref.exact["out"], torch.from_numpy(want), "the padded-sequence definition against the oracle")


# ------------------------------------------------------------------------------------------------ PSD
@pytest.mark.parametrize("case", A.STAT_CASES, ids=A.case_id)
def test_psd_frame_stats_bits(fake, case):
    d = A.stat_inputs(case)
    ref = A.stat_reference(d)
    hold("psd_frame_stats", A.case_id(case), A.run_stats(fake, d), ref)
    fid = ref.exact["fid"].view(d["B"], d["T"])
    for t, (name, cols) in enumerate(d["profiles"]):            # the first index wins
        assert int(fid[2, t]) == (cols[0] if cols else 0) or name == "none", (name, int(fid[2, t]))
    assert fid[0].tolist() == [-1] * d["T"] and fid[1, 1:].tolist() == [-1] * (d["T"] - 1)


def test_stat_cases_cross_lanes_waves_and_the_stride():
    names = {n for n, _ in A.tie_profiles(25055)}
    assert {"5=261", "63=64", "255=256", "0=25054", "70=582", "300=1068", "equal", "zero"} <= names
    assert {c.V for c in A.STAT_CASES} == {1, 255, 256, 257, 1000, 25055}


@pytest.mark.parametrize("name", A.PLAN_CASES)
def test_psd_plan_bits_and_margins(fake, name):
    d = A.plan_inputs(name)
    ref = A.plan_reference(d)
    hold("psd_plan", name, A.run_plan(fake, d), ref)
    margin, equal = A.plan_margins(d)
    print(f"AUDIO64 psd_plan {name}: new_lens {ref.exact['new_lens'][:d['B']].tolist()}, smallest |mean - thr| = {margin:.3g} roundings, {equal} means equal thr")
    if d["exact"]:
        assert equal == 3 and ref.exact["new_lens"][0] == 3 and ref.exact["seg_start"][:3].tolist() == [2, 5, 7]
    else:
        assert equal == 0 and margin > 100, "a segment mean within fp32 rounding of the threshold"
    if name == "identity":
        for b in range(d["B"]):
            L = int(d["lens"][b])
            assert int(ref.exact["new_lens"][b]) == L
            assert ref.exact["seg_start"][b * d["T"]:b * d["T"] + L].tolist() == list(range(L)) and bool((ref.exact["seg_len"][b * d["T"]:b * d["T"] + L] == 1).all())


def test_plan_cases_sit_on_the_chunk_and_wave_edges():
    seen_T = set()
    for name in A.PLAN_CASES:
        d = A.plan_inputs(name)
        seen_T |= {d["T"]} | set(d["lens"].tolist())
    assert seen_T >= {0, 1, 255, 256, 257, 504, 513, 769}
    segs = lambda name, b: [(int(s), int(n)) for s, n in zip(*(A.plan_reference(A.plan_inputs(name)).exact[k][b * 769:(b + 1) * 769] for k in ("seg_start", "seg_len"))) if s >= 0]
    cross = segs("cross", 0)
    assert (250, 12) in cross and (505, 15) in cross                                       # runs across 255|256 and 511|512, kept
    assert (250, 12) in segs("cross", 1) and not any(s == 505 for s, _ in segs("cross", 1))  # the second one dropped
    assert (100, 300) in segs("long", 0) and (99, 157) in segs("long", 1) and not any(s == 256 for s, _ in segs("long", 1))
    lanes = [s for s, _ in segs("lanes", 0)]
    assert 63 in lanes and 64 in lanes and 255 in lanes and 512 in lanes and not any(128 <= s < 192 or 256 <= s < 512 for s in lanes)
    d = A.plan_inputs("random769")
    assert all(int(d["fid"][b, L]) == int(d["fid"][b, L - 1]) for b, L in enumerate(d["lens"].tolist()) if 0 < L < 769)   # the last id repeats


@pytest.mark.parametrize("case", A.GATHER_CASES, ids=A.case_id)
def test_psd_gather_inside_the_bound(fake, case):
    d = A.gather_inputs(case)
    hold("psd_gather", A.case_id(case), A.run_gather(fake, d), A.gather_reference(d))
    mx = int(d["new_lens"].max())
    assert {"below": d["Tout"] < mx, "equal": d["Tout"] == mx, "above": d["Tout"] > mx}[case.tout]


def test_gather_cases():
    assert {(c.V, c.tout) for c in A.GATHER_CASES if c.plan == "hand"} == {(V, t) for V in (50, 203, 257, 560) for t in ("below", "equal", "above")}
    assert A.GATHER_W[560][0] != A.GATHER_W[560][1] and int(A.gather_inputs(A.GATHER_CASES[0])["seg_len"].max()) == 300


def test_psd_chain_against_the_oracle(fake):
    d = A.chain_inputs()
    ref, Tout = A.chain_reference(d)
    got, tout = A.run_chain(fake, d)
    assert tout == Tout
    hold("psd chain", "B=3 T=504 V=64", got, ref)
    margin, equal = A.plan_margins(A.chain_plan_inputs(d))
    nl = ref.exact["new_lens"].tolist()
    print(f"AUDIO64 psd chain: new_lens {nl} of lens {d['lens'].tolist()}, smallest |mean - thr| = {margin:.3g} roundings")
    assert equal == 0 and margin > 100
    assert all(0 < n < L for n, L in zip(nl, d["lens"].tolist())) and int(ref.exact["seg_len"].max()) > 1    # PSD merges and drops
    p = d["post3"].to(F64)
    top = p.topk(2, -1).values
    assert float((top[..., 0] - top[..., 1]).min()) > 1e-3, "an argmax decided by rounding"


# ------------------------------------------------------------------------------------------------ csrc/misc.hip
@pytest.mark.parametrize("case", A.POST_CASES, ids=A.case_id)
def test_posterior_build_inside_the_bound(fake, case):
    d = A.post_inputs(case)
    hold("posterior_build", A.case_id(case), A.run_post(fake, d), A.post_reference(d))


@pytest.mark.parametrize("case", A.MERGE_CASES, ids=A.case_id)
def test_embed_merge_and_backward_bits(fake, case):
    d = A.merge_inputs(case)
    hold("embed_merge", A.case_id(case), A.run_merge(fake, d), A.merge_reference(d))
    b = A.bwd_inputs(case)
    hold("merge_bwd", A.case_id(case), A.run_bwd(fake, b), A.bwd_reference(b))


def test_rne_is_the_cast_and_the_special_values_are_special():
    sp = A.bwd_special_values()
    A.same_bits(A.rne_bf16(sp), sp.to(BF), "rne_bf16 against torch's cast")
    x = torch.randn(4096) * torch.logspace(-30, 30, 4096)
    A.same_bits(A.rne_bf16(x), x.to(BF), "rne_bf16 on random values")
    r = A.rne_bf16(sp)
    assert bool(torch.isinf(r.float()).any()) and bool(torch.isfinite(sp).all())            # the largest finite value rounds to inf
    trunc = (sp.view(torch.int32) & -65536).view(F32).to(BF)
    assert int((A.bits(trunc) != A.bits(r)).sum()) >= 15                                  # truncation differs on the ties and above them
    assert {c.M for c in A.MERGE_CASES} >= {1, 3, 4, 5, 61} and {c.D for c in A.MERGE_CASES} >= {4, 252, 256, 260, 1536}
    d = A.merge_inputs(A.MergeCase(61, 256, "mixed"))
    assert set(d["kind"].tolist()) == {0, 1, 2} and set(A.merge_inputs(A.MergeCase(61, 256, "none"))["kind"].tolist()) == {0}


# ------------------------------------------------------------------------------------------------ mutants, restated on the CPU
def _mutant(name, ref, got):
    w = A.worst_of(got, ref)
    print(f"MUTANT {name}: worst |err| / E {w:.3g}")
    return w


def _fb_mutant(d, no_nyquist=False, window_off=False, mel_scale=1.0):
    """the fp32 restatement with one of the issue's errors"""
    d = dict(d)
    if window_off:
        w = d["window"].clone()
        w[1:] = d["window"][:-1]
        d["window"] = w
    if no_nyquist or mel_scale != 1.0:
        m = d["mel"].clone() * mel_scale
        if no_nyquist:
            m[:, 256] = 0
        d["mel"] = m
    return {"out": A.fb_restatement_f32(d)}, None


def test_mutants_of_fbank_fail(fb_refs):
    noise = next(c for c in A.FB_CASES if c.wave == "noise" and c.n == 12000)
    d, ref = fb_refs[noise]
    old = lambda got: float((got["out"].double() - ref.tol["out"][0]).abs().max())       # the old test's measure, limit 2e-3
    for name, kw in (("window read one index off", dict(window_off=True)), ("mel weights 0.1 % off", dict(mel_scale=1.001))):
        got, _ = _fb_mutant(d, **kw)
        w = _mutant(f"fbank {name} (old measure {old(got):.2e} against 2e-3)", ref, got)
        assert w > 3 * A.LIMIT, name
    eye = next(c for c in A.FB_CASES if c.wave == "alt" and c.mel == "eye")
    d, ref = fb_refs[eye]
    got, _ = _fb_mutant(d, no_nyquist=True)
    assert _mutant("fbank bin 256 dropped, identity mel matrix", ref, got) > 100
    alt = next(c for c in A.FB_CASES if c.wave == "alt" and c.mel == "mel")
    d, ref = fb_refs[alt]
    got, _ = _fb_mutant(d, no_nyquist=True)
    _mutant("fbank bin 256 dropped, the Kaldi mel matrix (its Nyquist column is zero: not visible)", ref, got)


def test_mutants_of_the_plan_the_gather_and_the_cast_fail(fake):
    class NoCarry(FakeOps):                                      # base_s not carried: each chunk numbers its segments from 0
        def psd_plan(self, fid, fblank, lens, ss, sl, nl, B, T, blank_id, thr):
            a, b, c = ss.clone(), sl.clone(), nl.clone()
            FakeOps.psd_plan(self, fid, fblank, lens, a, b, c, B, T, blank_id, thr)
            for u in range(B):
                n, k = int(c[u]), 0
                for j in range(n):
                    s = int(a[u * T + j])
                    k = k + 1 if j and s // 256 == int(a[u * T + j - 1]) // 256 else 1
                    ss[u * T + k - 1], sl[u * T + k - 1] = s, b[u * T + j]
                nl[u] = k if n else 0

    class ChunkStarts(FakeOps):                                  # a chunk's first frame always starts a segment
        def psd_plan(self, fid, fblank, lens, ss, sl, nl, B, T, blank_id, thr):
            f = fid.clone().view(B, T)
            f[:, 256::256] += 1000
            FakeOps.psd_plan(self, f.view(-1), fblank, lens, ss, sl, nl, B, T, blank_id, thr)

    for cls, names in ((NoCarry, ("random769", "t504", "t513", "cross")), (ChunkStarts, ("cross", "long"))):
        for name in names:
            d = A.plan_inputs(name)
            assert _mutant(f"psd_plan {cls.__name__} {name}", A.plan_reference(d), A.run_plan(cls(), d)) > A.LIMIT

    class DivideSingles(FakeOps):                                # the gather divides when len == 1 only
        def psd_gather(self, post, ss, sl, nl, out, B, T, bstride, Tout, V):
            FakeOps.psd_gather(self, post, ss, sl, nl, out, B, T, bstride, Tout, V)
            o = out[:B * Tout].view(B, Tout, -1)
            for b in range(B):
                for j in range(min(int(nl[b]), Tout)):
                    if int(sl.view(B, T)[b, j]) > 1:
                        o[b, j] *= int(sl.view(B, T)[b, j])

    d = A.gather_inputs(A.GATHER_CASES[0])
    assert _mutant("psd_gather divides single frames only", A.gather_reference(d), A.run_gather(DivideSingles(), d)) > 100

    class Truncate(FakeOps):
        def merge_bwd(self, dx, rows, dproj, n, D):
            FakeOps.merge_bwd(self, (dx.view(torch.int32) & -65536).view(F32), rows, dproj, n, D)

    b = A.bwd_inputs(A.MergeCase(5, 256, "mixed"))
    assert _mutant("merge_bwd truncates", A.bwd_reference(b), A.run_bwd(Truncate(), b)) > A.LIMIT

    class HalfPad(FakeOps):                                      # pad = lfr_m / 2
        def lfr_cmvn(self, fb, T, D, m, n, means, scales, out):
            Tl = (T + n - 1) // n
            f = torch.arange(Tl)[:, None] * n + torch.arange(m)[None, :] - m // 2
            v = fb[:T][f.clamp(0, T - 1)].reshape(Tl, m * D)
            out[:Tl] = v if means is None else (v + means[None]) * scales[None]

    hit = {}
    for c in A.LFR_CASES:
        d = A.lfr_inputs(c, 13)
        hit[c.m] = A.worst_of(A.run_lfr(HalfPad(), d), A.lfr_reference(d)) > A.LIMIT
    print(f"MUTANT lfr pad = lfr_m / 2: fails by lfr_m {hit}")
    assert hit[4] and not hit[7] and not hit[1]                  # (m - 1) / 2 == m / 2 for odd m: only the even lfr_m of this list sees it


def test_mutant_tie_rule_reversed(fake):
    d = A.stat_inputs(A.StatCase(1000, "first"))
    ref = A.stat_reference(d)
    rows = d["rows"].reshape(d["B"] * d["T"], -1)
    last = (rows.shape[1] - 1 - rows.flip(-1).argmax(-1)).view(d["B"], d["T"])
    live = torch.arange(d["T"])[None] < d["lens"][:, None]
    bad = torch.where(live, last, torch.full_like(last, -1)).reshape(-1).to(I32)
    wrong = int((bad != ref.exact["fid"]).sum())
    print(f"MUTANT psd_frame_stats takes the last index on ties: {wrong} wrong frame ids at V = 1000")
    assert wrong >= 6
