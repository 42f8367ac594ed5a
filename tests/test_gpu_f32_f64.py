"""The fp32 decode family (csrc/fp32.hip, every `tasu_f32_*` entry point) against float64 references, element by element
(tests/f32_ref64.py; its own checks and the mutants: tests/test_f32_ref64_cpu.py), through HipOps:

  GEMMs        tasu_f32_gemm_nt (one K step, ragged tiles, K-range slabs at ksplit 8 / 7 / 5 / 3 / 2 / 1 and one the workspace
               forces, act x bias x in-place residual, leading dimensions above the widths, a 32 MB matrix on the dispatcher's
               streaming route), tasu_f32_gemm_stream (every KS x row-block count x ksplit 1 / 2 / 16, walks of 1 .. 7 tiles per
               workgroup from the device's CU count, N = 1 .. 31, the fragment-order copy, every refusal), the three finishers on
               both routes
  rows         tasu_f32_rmsnorm, _rope, _kv_fill, _swiglu, _embed_merge, _fsmn
  attention    tasu_f32_attn_prefill (causal REP 1 .. 8, S = 1 .. 257 and 2048, kstart; the klen form; the bidirectional kernel) and
               tasu_f32_attn_decode (REP 1 .. 8, 1 .. 328 visible keys, an empty row between live ones, a scattered beam index,
               ctx = 2048)
  loss         tasu_f32_ce

Every output, workspace and cache starts as NaN (integers -7), every operand has NaN guard rows and NaN in the gap of its leading
dimension; everything outside what a call owes must keep its bits.  Every element within 1.0 x E of the float64 value, exactly the
reference's value where E = 0; the exact-integer GEMM profiles, the copies and RoPE bit for bit; calls with a workspace twice, equal bits.

Measured on MI355X (199 tests, 3.0 s for the file; the slowest, prefill at S = 2048, 1.0 s): every check passes.  Largest |err| / E
per operation (the F64WORST lines), kernel / the torch fp32 restatement on the CPU:
    gemm_nt 0.874 / 0.493   gemm_stream 0.217 / 0.217   gemm_resid_rmsnorm 0.165 / 0.211   gemm_swiglu 0.857 / 0.270
    gemm_qkv_rope 0.034 / 0.059   rmsnorm 0.149 / 0.193   swiglu 0.796 / 0.343   fsmn 0.377 / 0.377   ce 0.580 / 0.580
    attn_prefill causal 0.019, klen 0.015, bidirectional 0.018 / 0.058   attn_decode 0.011 / 0.024
The first run missed one bound: SiLU on an exact sum at x = -45, 8.7 x (5 e |silu|): expf as compiled here carries e |x| relative
(-ffp-contract=fast contracts a step of its expansion; tests/f32_ref64.py's header and DESIGN section 5), so expf's argument
allowance e |d| now stands in the SiLU bound as it does in the softmax and cross-entropy bounds.  No kernel needed a fix beyond the
three changes made with this file (the decode kernel's empty key range, the refusal of ldx != N before the launch, klen clamped to S).
Mutants through the restatement (older tensor-wide metric -> new): one lost a_k w_k in one element under an outlier residual column
9.5e-6 (passes 2e-5) -> 59 E; on all rows 6.4e-5 -> 513 E; a slab summed in bf16 6.9e-6 (passes) -> 60 E; bias after SiLU 1.8e-3 ->
1.0e4 E; the newest of 321 keys dropped 1.4e-2 -> 2.2e3 E; a key from the wrong beam row 5.1e-3 -> 807 E; slot off by one, a pad
column of dlogits unwritten: guards; RMSNorm over a padded D 4.9e-4 -> 432 E; argmax ties to the last column 9.1e-8 (passes) -> wrong
index.  Not reached: scratch mutants of the kernels themselves, S / ctx between 329 and 2047, N(0, 1) GEMMs above K = 512, lens > ctx
and index entries outside the cache (the entry points cannot see them), the dispatcher's lab-only switches."""
import pytest
import torch

import f32_ref64 as R

pytestmark = pytest.mark.gpu
F64, F32, I32 = torch.float64, torch.float32, torch.int32
HD = R.HD


@pytest.fixture(scope="module")
def hip():
    from ps_slm_amd.ops import HipOps
    return HipOps()


def cuda(t):
    return t.cuda()


def sync():
    torch.cuda.synchronize()


def nan(*shape):
    return R.nan(*shape).cuda()


_worst = {}


def hold(op, case, got, ref):
    what = f"{op} {R.case_id(case)}"
    w = R.check(got, ref, what)
    _worst[op] = max(_worst.get(op, 0.0), w)
    print(f"F64WORST {what} |err| / E {w:.3f} (largest so far for {op}: {_worst[op]:.3f})")


def refused(call, *outs):
    from ps_slm_amd.ops import TasuOpError
    with pytest.raises(TasuOpError, match="bad argument"):
        call()
    sync()
    for o in outs:
        assert R.untouched(o.cpu()), "a refused call wrote to its output"


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------------------------------------ the tile kernel
@pytest.mark.parametrize("case", R.TILE_CASES, ids=R.case_id)
def test_gemm_nt(hip, case):
    d = R.gemm_inputs(case)
    assert hip.lib.tasu_f32_gemm_streams(case.M, case.N, case.K, R.ws_floats(case) if case.ws else 0) == 0
    hold("gemm_nt", case, R.run_gemm(hip, d, cuda, sync), R.gemm_reference(d))


def test_gemm_nt_sends_a_32_mb_matrix_to_the_streaming_kernel(hip):
    """N = 2048, K = 4096 (32 MB): the dispatcher's streaming route, asserted; exact on the integer profile at 64 rows and at 1;
    on N(0, 1) inputs the row alone has the bits it has among 64"""
    N, K = 2048, 4096
    g = R.gen(3, N, K)
    w = torch.randint(-4, 5, (N, K), generator=g).to(F32)
    a = torch.randint(-4, 5, (64, K), generator=g).to(F32)
    ws_n = 16 * 64 * N
    want = (a.to(F64) @ w.to(F64).t()).to(F32)
    wd = R.operand(w, K, cuda)
    for M in (64, 1):
        assert hip.lib.tasu_f32_gemm_streams(M, N, K, ws_n) == 1
        rows = a[64 - M:]
        res = []
        for _ in range(2):
            ws = nan(ws_n)
            full, cv = R.output(M, N, N + 4, cuda)
            hip.f32_gemm(R.operand(rows, K + 4, cuda), wd, cv, M, N, K, ws=ws)
            sync()
            res.append(R.owed(full, M, N, f"gemm_nt streamed, M = {M}"))
        R.same_bits(res[0], want[64 - M:], f"gemm_nt streamed, exact profile, M = {M}")
        R.same_bits(res[1], res[0], "gemm_nt streamed, second run")
    an, wn = torch.randn(64, K, generator=g), R.operand(torch.randn(N, K, generator=g) * K ** -0.5, K, cuda)
    c64, c1, ws = nan(64, N), nan(1, N), nan(ws_n)
    hip.f32_gemm(an.cuda(), wn, c64, 64, N, K, ws=ws)
    hip.f32_gemm(an[63:].cuda(), wn, c1, 1, N, K, ws=ws)
    sync()
    R.same_bits(c1.cpu()[0], c64.cpu()[63], "a row alone against the same row among 64")


# ------------------------------------------------------------------------------------------------ the streaming kernel
@pytest.mark.parametrize("ks", range(1, 7))
def test_gemm_stream_every_row_block_and_split_exact(hip, ks):
    """KS x M = 1, 16, 17, 32, 33, 48, 49, 64 x ksplit 1, 2, 16 on the integer profile: bit for bit"""
    for case in (c for c in R.STREAM_EXACT if c.route == ks):
        d = R.gemm_inputs(case)
        hold("gemm_stream", case, R.run_gemm(hip, d, cuda, sync), R.gemm_reference(d))


@pytest.mark.parametrize("case", R.STREAM_N01 + R.STREAM_NS, ids=R.case_id)
def test_gemm_stream(hip, case):
    d = R.gemm_inputs(case)
    hold("gemm_stream", case, R.run_gemm(hip, d, cuda, sync), R.gemm_reference(d))


@pytest.mark.parametrize("length", R.STREAM_WALKS)
def test_gemm_stream_walk_lengths(hip, length):
    """every workgroup walks `length` tiles on the ring of three (1, 2, 4, 5: spare slots in the last trip), the last tile partial;
    N from the device's CU count at ksplit = 16 and, for the short walks, at ksplit = 1"""
    n_cu = cus()
    todo = [(16, R.walk_N(length, n_cu, 16), M) for M in (64, 17)]
    if length <= 3:
        todo.append((1, R.walk_N(length, n_cu, 1), 33))
    for ksplit, N, M in todo:
        nbx, walks = R.stream_walks(N, ksplit, n_cu)
        assert walks == {length} and nbx == max(1, n_cu // ksplit)
        case = R.Gemm(1, M, N, 128 * ksplit, 0, True, False, "exact", 0, 0, 0, -1)
        d = R.gemm_inputs(case)
        hold("gemm_stream", case, R.run_gemm(hip, d, cuda, sync), R.gemm_reference(d))
    N = 16 * (max(1, n_cu // 16) * length) + 16 * 3 - 5          # a ragged walk: three workgroups walk one tile more
    _, walks = R.stream_walks(N, 16, n_cu)
    assert walks == ({length, length + 1} if n_cu // 16 > 3 else walks)
    case = R.Gemm(1, 49, N, 128 * 16, 0, False, False, "exact", 0, 0, 0, -1)
    d = R.gemm_inputs(case)
    hold("gemm_stream", case, R.run_gemm(hip, d, cuda, sync), R.gemm_reference(d))


@pytest.mark.parametrize("M,N,K,ks,ldw", [(33, 20, 256, 2, 4), (64, 100, 768, 3, 0), (1, 1, 128, 1, 8), (17, 31, 2048, 1, 0)])
def test_gemm_stream_on_the_fragment_order_copy(hip, M, N, K, ks, ldw):
    """the copy is the permutation the header defines (rows >= N zero, ldw > K), nothing behind it is written, and the product on
    it has the bits of the product on the row-major matrix"""
    g = R.gen(5, M, N, K)
    w, a = torch.randn(N, K, generator=g), torch.randn(M, K, generator=g)
    wd = R.operand(w, K + ldw, cuda)
    n_out = (N + 15) // 16 * 16 * K
    out = nan(n_out + 64)
    from ps_slm_amd.ops import F32Fragments
    assert hip.lib.tasu_f32_to_fragment_order(wd.data_ptr(), wd.stride(0), out.data_ptr(), N, K, hip._stream()) == 0
    sync()
    o = out.cpu()
    R.same_bits(o[:n_out], R.fragment_order(w), "fragment-order copy")
    assert R.untouched(o[n_out:])
    fr = F32Fragments(out[:n_out], N, K, wd)
    ad = R.operand(a, K, cuda)
    res = []
    for wt in (wd, fr):
        ws = nan(16 * 64 * N)
        full, cv = R.output(M, N, N + 1, cuda)
        hip.f32_gemm_stream(ad, wt, cv, M, N, K, ks, ws=ws)
        sync()
        res.append(R.owed(full, M, N, "gemm_stream"))
    R.same_bits(res[1], res[0], "the product on the fragment-order copy against the row-major one")
    c = nan(M, N)
    refused(lambda: hip.f32_gemm(ad, fr, c, M, N, K, ws=nan(16 * 64 * N)), c)        # the tile kernel does not serve the copy


def test_gemm_stream_refuses_what_it_does_not_serve(hip):
    a, w = torch.ones(70, 1024, device="cuda"), torch.ones(20, 1024, device="cuda")
    c, ws = nan(70, 24), nan(16 * 64 * 20)

    def call(M=16, N=20, K=256, ks=2, A=a, W=w, C=c, act=0, ws=ws):
        return lambda: hip.f32_gemm_stream(A, W, C, M, N, K, ks, act=act, ws=ws)

    refused(call(M=65), c, ws)
    refused(call(M=0), c, ws)
    refused(call(ks=0), c, ws)
    refused(call(ks=7), c, ws)
    refused(call(K=384, ks=2), c, ws)                                   # K no multiple of 128 ks
    refused(call(K=48), c, ws)                                          # K no multiple of 32
    refused(call(act=3), c, ws)
    refused(call(act=-1), c, ws)
    refused(call(K=512, ks=2, ws=None), c)                              # two K ranges, no workspace
    refused(call(K=512, ks=2, ws=ws[:2 * 16 * 20 - 1]), c, ws)          # ... a workspace one float short
    refused(call(K=128 * 17, ks=1, A=torch.ones(16, 128 * 17, device="cuda"), W=torch.ones(20, 128 * 17, device="cuda")), c, ws)   # 17 ranges
    refused(call(A=torch.as_strided(a, (16, 256), (258, 1))), c, ws)    # lda % 4
    refused(call(W=torch.as_strided(w, (20, 256), (252, 1))), c, ws)    # ldw < K
    refused(call(C=torch.as_strided(c, (16, 20), (16, 1))), c, ws)      # ldc < N
    refused(call(A=a.view(-1)[1:1 + 16 * 1024].view(16, 1024)), c, ws)  # A not 16-byte aligned
    refused(lambda: hip.f32_gemm(a, w, c, 16, 20, 48), c)               # (the tile kernel: K % 32)


# ------------------------------------------------------------------------------------------------ the finishers
@pytest.mark.parametrize("case", R.FIN_CASES + R.FIN_STREAM, ids=R.case_id)
def test_gemm_finishers(hip, case):
    d = R.fin_inputs(case)
    NN = 2 * case.N if case.op == "swiglu" else case.N
    assert hip.lib.tasu_f32_gemm_streams(case.M, NN, case.K, R.fin_ws(case, NN)) == (1 if case.route == "stream" else 0)
    ref = R.fin_reference(d)
    hold(f"gemm_{case.op}", case, R.run_fin(hip, d, cuda, sync), ref)
    if case.route == "slabs" and case.op == "norm":              # the split route serves ldx > N
        hold(f"gemm_{case.op}", case, R.run_fin(hip, d, cuda, sync, ldx=5), ref)
    if case.route == "slabs" and case.op == "swiglu":            # ... and leaves a gu scratch it is given alone
        ref.tol.pop("gu", None)
        hold(f"gemm_{case.op}", case, R.run_fin(hip, d, cuda, sync, gu_none=False), ref)


@pytest.mark.parametrize("case", R.QKV_CASES + [R.QKV_STREAM], ids=R.case_id)
def test_gemm_qkv_rope(hip, case):
    d = R.qkv_inputs(case)
    N = (case.H + 2 * case.G) * HD
    assert hip.lib.tasu_f32_gemm_streams(case.M, N, case.K, 16 * 64 * N if R.split(case) else 0) == (1 if case.route == "stream" else 0)
    hold("gemm_qkv_rope", case, R.run_qkv(hip, d, cuda, sync), R.qkv_reference(d))


def test_finishers_refuse_before_they_launch(hip):
    M, N, K = 5, 70, 64
    a, w, nw = torch.ones(M, K, device="cuda"), torch.ones(N, K, device="cuda"), torch.ones(N, device="cuda")
    xf, xv = R.output(M, N, N + 5, cuda)
    y = nan(M, N)
    refused(lambda: hip.f32_gemm_resid_rmsnorm(a, w, xv, nw, y, M, N, K, R.EPS, None), xf, y)      # unsplit route, ldx != N
    act = nan(M, N)
    refused(lambda: hip.f32_gemm_swiglu(a, torch.ones(2 * N, K, device="cuda"), None, act, M, N, K, None), act)   # unsplit route, no gu
    q = nan(M, 4 * HD)
    cs = torch.ones(M, 64, device="cuda")
    refused(lambda: hip.f32_gemm_qkv_rope(a, torch.ones(4 * HD, K, device="cuda"), None, q, cs, cs, M, 3, 2, K, None), q)   # H % G


# ------------------------------------------------------------------------------------------------ row and pointwise kernels
@pytest.mark.parametrize("case", R.RMS_CASES, ids=R.case_id)
def test_rmsnorm(hip, case):
    d = R.rms_inputs(case)
    got = R.run_rms(hip, d, cuda, sync)
    hold("rmsnorm", case, got, R.rms_reference(d))
    if case.profile == "zero_row":
        assert bool((got["y"][1] == 0).all())


@pytest.mark.parametrize("case", R.ROPE_CASES, ids=R.case_id)
def test_rope_has_the_bits_of_torch_eager(hip, case):
    R.same_bits(*R.run_rope(hip, case, cuda, sync), f"rope {R.case_id(case)}")


def test_kv_fill_and_embed_merge_copy(hip):
    for case in R.FILL_CASES:
        R.run_kv_fill(hip, case, cuda, sync)
    for case in R.EMB_CASES:
        R.run_embed(hip, case, cuda, sync)
    kc, vc = nan(2, 4, HD), nan(2, 4, HD)
    refused(lambda: hip.f32_kv_fill(torch.ones(10, 4 * HD, device="cuda"), kc, vc, 2, 5, 2, 1, 1, 4), kc, vc)      # S > ctx


def test_swiglu_and_fsmn(hip):
    for case in R.SWI_CASES:
        d = R.swi_inputs(case)
        got = R.run_swi(hip, d, cuda, sync)
        hold("swiglu", case, got, R.swi_reference(d))
        assert float(got["act"][0, 0]) == 0.0
    for case in R.FSMN_CASES:
        d = R.fsmn_inputs(case)
        hold("fsmn", case, R.run_fsmn(hip, d, cuda, sync), R.fsmn_reference(d))


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("case", R.PRE_CASES + [R.PRE_LONG], ids=R.case_id)
def test_attn_prefill(hip, case):
    d = R.pre_inputs(case)
    hold("attn_prefill[" + ("bidir" if case.mode == "klen" and case.H == case.G else case.mode) + "]", case, R.run_pre(hip, d, cuda, sync),
         R.pre_reference(d))


@pytest.mark.parametrize("case", R.DEC_CASES + [R.DEC_LONG], ids=lambda c: f"{c.H}x{c.G}-ctx{c.ctx}-{len(c.rows)}rows-{c.profile}")
def test_attn_decode(hip, case):
    d = R.dec_inputs(case)
    hold("attn_decode", case._replace(rows=len(case.rows)), R.run_dec(hip, d, cuda, sync), R.dec_reference(d))


def test_attention_refuses_what_it_does_not_serve(hip):
    z = torch.zeros(1, dtype=I32, device="cuda")
    one = torch.ones(1, dtype=I32, device="cuda")
    out = nan(1, 9 * HD)
    q = torch.ones(1, 11 * HD, device="cuda")
    kc = torch.ones(1, 4, HD, device="cuda")
    idx = torch.zeros(1, 2049, dtype=I32, device="cuda")
    refused(lambda: hip.f32_attn_decode(q, kc, kc, idx, z, one, out, 1, 9, 1, 4, 1.0), out)                      # H / G = 9
    refused(lambda: hip.f32_attn_decode(q, kc, kc, idx, z, one, out, 1, 8, 1, 2049, 1.0), out)                   # ctx = 2049
    refused(lambda: hip.f32_attn_prefill(q, z, out, 1, 1, 9, 1, 1.0), out)
    refused(lambda: hip.f32_attn_prefill(q, z, out, 1, 2049, 1, 1, 1.0), out)
    refused(lambda: hip.f32_attn_prefill(q, None, out, 1, 1, 1, 1, 1.0), out)                                    # neither kstart nor klen


# ------------------------------------------------------------------------------------------------ cross-entropy
@pytest.mark.parametrize("case", R.CE_CASES, ids=R.case_id)
def test_ce(hip, case):
    d = R.ce_inputs(case)
    hold("ce", case, R.run_ce(hip, d, cuda, sync), R.ce_reference(d))


def test_ce_refuses_what_it_does_not_serve(hip):
    x, lab = torch.zeros(2, 8, device="cuda"), torch.zeros(2, dtype=I32, device="cuda")
    rl, rh, dl = nan(2), torch.full((2,), -7, dtype=I32, device="cuda"), nan(2, 8)
    refused(lambda: hip.f32_ce(x, lab, 2, 9, rl, rh), rl, rh)                                                   # ld < V
    refused(lambda: hip.f32_ce(x, lab, 2, 8, rl, rh, dlogits=dl), rl, rh, dl)                                   # no inv_count
