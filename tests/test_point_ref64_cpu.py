"""CPU checks of the float64 references of the rotary, pointwise and encoder-memory kernels and their bounds
(tests/point_ref64.py), which tests/test_gpu_point_f64.py holds the HIP kernels to:

* the bounds are honest: the torch double (tests/fake_ops.py, fp32 torch on the CPU) stays within 1.0 x E on every case of the
  shared lists, gives the bits of the exact profiles, and gives equal bits twice (the DOUBLE lines this file prints);
* the references are the operations: a Python loop over frames, channels and taps for the FSMN, torch.autograd in float64 for the
  derivatives (SiLU, SwiGLU, the rotation's adjoint), a loop over single pairs for RoPE, scalar `math` for the table and the PE,
  bf16r for the cast;
* the case lists sit on the kernels' switches (the thread map of rope_bwd_kernel, the grid-stride second pass, the FSMN routes);
* the checks have teeth: ten mutants of the double (MUTANT lines), each scored under the tensor-wide metric of
  tests/test_gpu_ops.py (max|a-b| / max|b| against that test's limit, on the same inputs) and under |err| / E.  The table is in
  DESIGN section 5; four of the ten pass the older metric (truncating SiLU store, SwiGLU without the intermediate rounding, the
  cast's ties, left = ks / 2 -- the older FSMN test has odd kernel sizes only)."""
import math

import pytest
import torch
import torch.nn.functional as F

import point_ref64 as P
from fake_ops import FakeOps, _bf

F64, F32, BF, I32 = torch.float64, torch.float32, torch.bfloat16, torch.int32


@pytest.fixture(scope="module")
def fake():
    return FakeOps()


def rel_err(a, b):
    """the tensor-wide metric of tests/test_gpu_ops.py"""
    a, b = a.float(), b.float()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def close(a, b, what, tol=1e-12):
    err = float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
    assert err < tol, (what, err)


# ------------------------------------------------------------------------------------------------ 1. the double inside the bounds
FAMILIES = {
    "rope_table": (P.TABLE_CASES, P.table_inputs, P.table_reference, P.run_table),
    "rope_fwd": (P.ROPE_FWD_CASES, P.rope_fwd_inputs, P.rope_fwd_reference, P.run_rope_fwd),
    "rope_bwd": (P.ROPE_BWD_CASES, P.rope_bwd_inputs, P.rope_bwd_reference, P.run_rope_bwd),
    "unary": (P.UNARY_CASES, P.unary_inputs, P.unary_reference, P.run_unary),
    "swiglu": (P.SWIGLU_CASES, P.swiglu_inputs, P.swiglu_reference, P.run_swiglu),
    "cast": (P.CAST_CASES, P.cast_inputs, P.cast_reference, P.run_cast),
    "sinusoid_pe": (P.PE_CASES, P.pe_inputs, P.pe_reference, P.run_pe),
    "fsmn_fwd": (P.FSMN_CASES, P.fsmn_inputs, P.fsmn_reference, P.run_fsmn),
}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_double_stays_inside_the_bound_on_every_case(fake, family):
    cases, inputs, reference, run = FAMILIES[family]
    worst = {}
    for c in cases:
        d = inputs(c)
        op = getattr(c, "op", family)
        w = P.check(run(fake, d), reference(d), f"double {family} {P.case_id(c)}")
        worst[op] = max(worst.get(op, 0.0), w)
    for op, w in worst.items():
        print(f"DOUBLE {op}: largest |err| / E {w:.3f}")
        assert w <= P.LIMIT


@pytest.mark.parametrize("case", P.FSMN_LN_CASES, ids=P.case_id)
def test_double_fsmn_ln(fake, case):
    d = P.fsmn_ln_inputs(case)
    out = P.run_fsmn_ln(fake, d)
    w = P.check({"xn": out["xn"]}, P.fsmn_ln_reference(d, out["x"]), f"double fsmn_ln_fwd {P.case_id(case)}")
    print(f"DOUBLE fsmn_ln_fwd xn: largest |err| / E {w:.3f}")


# ------------------------------------------------------------------------------------------------ 2. the references are the operations
def test_fsmn_reference_is_the_loop_over_frames_channels_and_taps():
    for case in (P.FsmnCase(8, 11, 19, 0, "n01"), P.FsmnCase(16, 4, 19, 0, "n01"), P.FsmnCase(16, 1, 16, 0, "exact"), P.FsmnCase(8, 11, 37, 0, "exact")):
        d = P.fsmn_inputs(case)
        B, T, D, ks = d["B"], d["T"], d["D"], d["ks"]
        v = d["vbuf"].view(B, T, -1)[..., 2 * D:].double()
        w = d["w"][:D * ks].double().view(D, ks)
        left = (ks - 1) // 2
        want = torch.zeros(B, T, D, dtype=F64)
        for b in range(B):
            n = int(d["lens"][b])
            for t in range(n):
                for ch in range(D):
                    acc = 0.0
                    for j in range(ks):
                        tt = t + j - left
                        if 0 <= tt < n:
                            acc += float(w[ch, j]) * float(v[b, tt, ch])
                    want[b, t, ch] = acc + float(v[b, t, ch])
        got, _ = P.fsmn_sums(d)
        assert not bool(torch.isnan(want).any())
        close(got, want, f"fsmn {P.case_id(case)}")


def test_activation_references_are_the_autograd_derivatives():
    d = P.unary_inputs(P.UnaryCase("silu_bwd", 1003))
    g = d["x"][:1003].double().requires_grad_()
    (dx,) = torch.autograd.grad(g * torch.sigmoid(g), g, d["dy"][:1003].double())
    ref = P.unary_reference(d).tol["y"][0][0]
    big = ref.abs() > 1e-30                                      # (autograd's sigmoid'(-80) underflows differently: compare where it matters)
    close(ref[big], dx[big], "silu_bwd", 1e-9)
    s = P.swiglu_inputs(P.SwigluCase("swiglu_bwd", 77, 512))
    gu = s["gu"][:77].double().requires_grad_()
    y = F.silu(gu[:, :512]) * gu[:, 512:]
    (dgu,) = torch.autograd.grad(y, gu, s["dact"][:77].double())
    ref = P.swiglu_reference(s).tol["dgu"][0]
    big = ref.abs() > 1e-30
    close(ref[big], dgu[big], "swiglu_bwd", 1e-9)
    f = P.swiglu_inputs(P.SwigluCase("swiglu_fwd", 77, 512))
    gf = f["gu"][:77].double()
    close(P.swiglu_reference(f, plain=True), F.silu(gf[:, :512]) * gf[:, 512:], "swiglu_fwd", 1e-9)
    want, E = P.swiglu_reference(f).tol["act"]
    assert float((E == 0).double().mean()) > 0.99                # nearly every element has ONE right answer ...
    assert float(((want - P.swiglu_reference(f, plain=True)).abs() / want.abs().clamp_min(1e-300)).max()) < 2 * P.U + P.U * P.U   # ... two roundings away
    u = P.unary_inputs(P.UnaryCase("silu_fwd", 1003))
    close(P.unary_reference(u).tol["y"][0][0], F.silu(u["x"][:1003].double()), "silu_fwd", 1e-9)


def test_rope_references_are_the_pair_loop_and_its_adjoint():
    d = P.rope_fwd_inputs(P.RopeCase(1, 65, 2, 1, "none"))
    M, H, G = d["M"], d["H"], d["G"]
    ref = P.rope_fwd_reference(d).tol["qk"][0].view(M, H + G, 128)
    x = d["qkv"].double().view(M, H + 2 * G, 128)
    for m in range(M):
        for h in range(H + G):
            for i in range(64):
                c, s = float(d["cos"][m, i]), float(d["sin"][m, i])
                x1, x2 = float(x[m, h, i]), float(x[m, h, i + 64])
                assert abs(float(ref[m, h, i]) - (x1 * c - x2 * s)) <= 1e-15 * (abs(x1 * c) + abs(x2 * s))
                assert abs(float(ref[m, h, i + 64]) - (x2 * c + x1 * s)) <= 1e-15 * (abs(x2 * c) + abs(x1 * s))
    # the backward is the adjoint of the forward, the k heads on the SUM of the group's partials, laid out as the double reads them
    b = P.rope_bwd_inputs(P.RopeBwdCase(28, 4, 7, "n01"))
    M, H, G, npg = b["M"], b["H"], b["G"], b["npg"]
    cs, sn = b["cos"][:M].double()[:, None], b["sin"][:M].double()[:, None]
    xx = torch.zeros(M, H + G, 128, dtype=F64, requires_grad=True)
    y = torch.cat([xx[..., :64] * cs - xx[..., 64:] * sn, xx[..., 64:] * cs + xx[..., :64] * sn], -1)
    dk = b["dk"][:M].double().view(M, G, npg, 128).sum(2)
    dy = torch.cat([b["dqkv"][:, :H * 128].double().view(M, H, 128), dk], 1)
    (dx,) = torch.autograd.grad(y, xx, dy)
    ref = P.rope_bwd_reference(b).tol["dqkv"][0].view(M, H + 2 * G, 128)
    close(ref[:, :H + G], dx, "rope_bwd q | k")
    close(ref[:, H + G:], b["dv"][:M].double().view(M, G, npg, 128).sum(2), "rope_bwd v")


def test_table_pe_and_cast_references_are_the_scalar_formulas():
    d = P.table_inputs(P.TableCase(1e6))
    ref = P.table_reference(d)
    for m in (1, 5, 7, 20, 48):
        for i in (0, 1, 31, 63):
            ang = int(d["pos"][m]) * math.pow(1e6, -i / 64)
            assert abs(float(ref.tol["cos"][0][m, i]) - math.cos(ang)) < 1e-9 and abs(float(ref.tol["sin"][0][m, i]) - math.sin(ang)) < 1e-9
    p = P.pe_inputs(P.PeCase(2, 37, 80, "zero"))
    y = P.pe_reference(p).tol["y"][0].view(2, 37, 80)
    inc = math.log(10000.0) / 39
    for t in (0, 1, 36):
        for k in (0, 1, 39):
            assert abs(float(y[1, t, k]) - math.sin((t + 1) * math.exp(-k * inc))) < 1e-12
            assert abs(float(y[0, t, 40 + k]) - math.cos((t + 1) * math.exp(-k * inc))) < 1e-12
    x = P.cast_inputs(P.CastCase(1003))["x"][:1003]
    ok = (x.abs() < 2.0 ** 120) & ((x == 0) | (x.abs() >= 2.0 ** -120))
    assert int(ok.sum()) > 900
    P.same_bits(P.cast_bits(x)[ok], P.bf16r(x[ok].double()).to(F32).to(BF), "cast_bits against bf16r")
    top = torch.tensor([0x7F7F7FFF, 0x7F7F0001], dtype=torch.int32).view(F32)
    assert bool(torch.isfinite(P.cast_bits(top).float()).all()) and float(P.cast_bits(top).float()[0]) == float(torch.finfo(BF).max)
    ties = torch.tensor([0x3F808000, 0x3F818000], dtype=torch.int32).view(F32)      # even kept bit: down; odd: up
    assert P.cast_bits(ties).view(torch.int16).tolist() == [0x3F80, 0x3F82]


# ------------------------------------------------------------------------------------------------ 3. the case lists sit on the switches
def test_case_lists_sit_on_the_kernels_switches():
    assert [P.thread_map(H, G) for H, G in P.ROPE_BWD_GEOMETRIES[:5]] == [(32, 8, 32, 1), (48, 5, 51, 1), (112, 2, 128, 1), (160, 1, 256, 1), (288, 1, 256, 2)]
    assert 5 * 51 == 255                                         # (4, 1): thread 255 idles
    assert [(H // G) // P.dkv_hpb(H // G) for H, G in P.ROPE_BWD_GEOMETRIES] == [1, 2, 5, 4, 7, 1, 2]
    assert {c.M for c in P.ROPE_BWD_CASES} == {1, 7, 23}
    assert {c.S for c in P.ROPE_FWD_CASES} == {1, 63, 64, 65, 100} and {(c.H, c.G) for c in P.ROPE_FWD_CASES} == {(2, 1), (4, 2), (12, 2), (28, 4)}
    assert {c.copies for c in P.ROPE_FWD_CASES} == {"all", "none", "kt"} and sum(c.B == 2 for c in P.ROPE_FWD_CASES) >= 2
    threads = 2048 * 256
    assert P.BIG_UNARY // 8 == threads + 1 and P.BIG_UNARY % 8 == 3 and P.BIG_CAST // 4 == threads + 1 and P.BIG_CAST % 4 == 3
    assert P.BIG_SWIGLU_I // 8 == threads + 1
    assert {n for n in P.UNARY_N} >= {1, 7, 8, 9, 1003} and {c.n for c in P.CAST_CASES} >= {1, 3, 4, 5, 1003}
    assert [P.fsmn_route(D, ks, 3 * D) for D, ks in P.FSMN_ROUTES] == ["vector", "vector", "vector", "scalar", "scalar", "scalar"]
    assert P.fsmn_lens(37) == [37, 0, 1, 5, 16, 17, 36] and P.fsmn_lens(1) == [1, 0, 1, 1, 1, 1, 0]
    assert len(P.edge_tuples(True, True)) == 13 * 36 - 4 + 13
    d = P.fsmn_inputs(P.FsmnCase(8, 11, 19, 0, "n01"))
    v = d["vbuf"].view(d["B"], 19, 24)
    assert bool(torch.isnan(v[..., :16]).all()) and bool(torch.isnan(v[1]).all()) and bool(torch.isnan(v[3, 5:]).all()) and not bool(torch.isnan(v[3, :5, 16:]).any())


# ------------------------------------------------------------------------------------------------ 4. mutants of the double
def _truncate(x):
    """fp32 -> bf16 by dropping the low 16 bits"""
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


class Mutants(FakeOps):
    def __init__(self, which):
        self.which = which

    def silu_fwd(self, x, y):
        if self.which == "silu truncates":
            return y.copy_(_truncate(F.silu(x.float())))
        super().silu_fwd(x, y)

    def silu_bwd(self, dy, x, dx):
        if self.which == "silu' without g (1 - sg)":
            return dx.copy_(_bf(dy.float() * torch.sigmoid(x.float())))
        super().silu_bwd(dy, x, dx)

    def swiglu_fwd(self, gu, act, M, I):
        if self.which == "swiglu without bf16(silu)":
            return act.copy_(_bf(F.silu(gu[:, :I].float()) * gu[:, I:].float()))
        super().swiglu_fwd(gu, act, M, I)

    def rope_bwd(self, dqkv, dk_part, dv_part, cos, sin, B, S, H, G):
        if self.which == "rope_bwd drops the last partial":
            rep = H // G
            npg, np_ = rep // P.dkv_hpb(rep), H // P.dkv_hpb(rep)
            dk_part, dv_part = dk_part.clone(), dv_part.clone()
            for t in (dk_part, dv_part):
                t[:B * S].view(B * S, G, npg, 128)[:, :, npg - 1] = 0
        super().rope_bwd(dqkv, dk_part, dv_part, cos, sin, B, S, H, G)

    def rope_fwd(self, qkv, cos, sin, qt, kt, vt, B, S, H, G):
        if self.which == "rope_fwd flips s on the upper half":
            v = qkv.view(B, S, H + 2 * G, 128)
            c, s = cos.view(B, S, 1, 64), sin.view(B, S, 1, 64)
            x = v[:, :, :H + G].float()
            v[:, :, :H + G] = _bf(torch.cat([x[..., :64] * c - x[..., 64:] * s, x[..., 64:] * c - x[..., :64] * s], -1))
            Spad = (S + 63) // 64 * 64
            for dst, lo, n in ((qt, 0, H), (kt, H, G), (vt, H + G, G)):
                if dst is not None:
                    dst.view(B, n, 128, Spad).zero_()
                    dst.view(B, n, 128, Spad)[..., :S] = v[:, :, lo:lo + n].permute(0, 2, 3, 1)
            return
        super().rope_fwd(qkv, cos, sin, qt, kt, vt, B, S, H, G)

    def cast_bf16(self, src, dst):
        if self.which == "cast rounds half away from zero":
            b = src.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
            r = (b + 0x8000) >> 16
            return dst.copy_((r - ((r >> 15) << 16)).to(torch.int16).view(BF))
        super().cast_bf16(src, dst)

    def fsmn_fwd(self, v, ldv, w, lens, out, B, T, D, ksize, accumulate):
        if self.which not in ("fsmn drops the tap at len - 1", "fsmn left = ks / 2"):
            return super().fsmn_fwd(v, ldv, w, lens, out, B, T, D, ksize, accumulate)
        vv = v.reshape(B, T, -1)[..., :D].float()
        tt = torch.arange(T)[None]
        live = (tt < lens[:, None])[..., None]
        vm = torch.where(live, vv, torch.zeros_like(vv))
        taps = torch.where((tt < lens[:, None] - 1)[..., None], vv, torch.zeros_like(vv)) if self.which.startswith("fsmn drops") else vm
        left = ksize // 2 if self.which == "fsmn left = ks / 2" else (ksize - 1) // 2
        xp = F.pad(taps.transpose(1, 2), (left, ksize - 1 - left))
        fs = F.conv1d(xp, w.view(D, 1, ksize), None, groups=D).transpose(1, 2)
        r = ((fs + vm) * live.float()).reshape(B * T, D)
        out.add_(r) if accumulate else out.copy_(r)

    def sinusoid_pe(self, x, y, B, T, D, scale):
        if self.which not in ("pe t for t + 1", "pe halves swapped"):
            return super().sinusoid_pe(x, y, B, T, D, scale)
        pos = torch.arange(0 if self.which == "pe t for t + 1" else 1, T + (0 if self.which == "pe t for t + 1" else 1), dtype=torch.float32)
        inv = torch.exp(torch.arange(D // 2, dtype=torch.float32) * (-(math.log(10000.0) / (D / 2 - 1))))
        st = pos[:, None] * inv[None]
        pe = torch.cat([st.cos(), st.sin()], 1) if self.which == "pe halves swapped" else torch.cat([st.sin(), st.cos()], 1)
        y.view(B, T, D).copy_(x.view(B, T, D) * scale + pe[None])


# mutant -> (family, case, the older test's limit for this output)
MUTANTS = {
    "silu truncates": ("unary", P.UnaryCase("silu_fwd", 1003), 1e-2),
    "silu' without g (1 - sg)": ("unary", P.UnaryCase("silu_bwd", 1003), 1e-2),
    "swiglu without bf16(silu)": ("swiglu", P.SwigluCase("swiglu_fwd", 77, 512), 1e-2),
    "rope_bwd drops the last partial": ("rope_bwd", P.RopeBwdCase(28, 4, 23, "n01"), 1e-2),
    "rope_fwd flips s on the upper half": ("rope_fwd", P.RopeCase(2, 100, 4, 2, "all"), 1e-2),
    "cast rounds half away from zero": ("cast", P.CastCase(1003), 0.0),
    "fsmn drops the tap at len - 1": ("fsmn_fwd", P.FsmnCase(512, 11, 37, 0, "n01"), 1e-5),
    "fsmn left = ks / 2": ("fsmn_fwd", P.FsmnCase(16, 4, 19, 0, "n01"), 1e-5),
    "pe t for t + 1": ("sinusoid_pe", P.PeCase(2, 37, 80, "n01"), 1e-5),
    "pe halves swapped": ("sinusoid_pe", P.PeCase(2, 37, 80, "n01"), 1e-5),
}


def _older_inputs(name, fake, mut):
    """the mutant's score on the OLDER test's own inputs where they differ in kind from this file's (the shapes and
    distributions of tests/test_gpu_ops.py): N(0, 1) without ties for the cast, ks = 11 for the FSMN's left"""
    if name == "cast rounds half away from zero":
        x = torch.randn(1000 * 37 + 3, generator=torch.Generator().manual_seed(6))
        a, b = torch.zeros_like(x, dtype=BF), torch.zeros_like(x, dtype=BF)
        fake.cast_bf16(x, a), mut.cast_bf16(x, b)
        return rel_err(b, a)
    if name == "fsmn left = ks / 2":
        g = torch.Generator().manual_seed(2)
        v, w, lens = torch.randn(74, 256, generator=g).to(BF), torch.randn(256, 11, generator=g) * 0.2, torch.tensor([37, 20], dtype=I32)
        a, b = torch.zeros(74, 256), torch.zeros(74, 256)
        fake.fsmn_fwd(v, 256, w, lens, a, 2, 37, 256, 11, False), mut.fsmn_fwd(v, 256, w, lens, b, 2, 37, 256, 11, False)
        return rel_err(b, a)
    return None


@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutant_fails_the_new_check(fake, name):
    family, case, old_limit = MUTANTS[name]
    _, inputs, reference, run = FAMILIES[family]
    d = inputs(case)
    ref = reference(d)
    good, mut = run(fake, d), run(Mutants(name), d)
    assert P.worst_of(good, ref) <= P.LIMIT
    w = P.worst_of(mut, ref)
    old = _older_inputs(name, fake, Mutants(name))
    if old is None:
        old = max(rel_err(mut[k], good[k]) for k in good)
    verdict = "passes" if old <= old_limit else "FAILS"
    line = f"MUTANT {name}: older metric {old:.2e} ({verdict} {old_limit:g}); new |err| / E {w:.3g}"
    if family in ("unary", "swiglu") and good[next(iter(good))].dtype == BF and ref.tol:
        (k, (want, E)), = ref.tol.items()
        rm, n = P.rms_stat(mut[k], want, E)
        rg, _ = P.rms_stat(good[k], want, E)
        line += f", rms {rm / max(rg, 1e-30):.2f} x the double's over {n} elements"
    print(line)
    assert w > P.LIMIT, f"{name}: the new check passes the mutant ({w:.3f} x E)"
