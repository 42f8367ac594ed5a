"""The kernels that carry audio from the waveform to the decoder's input rows against float64 references, element by element
(tests/audio_ref64.py; its own checks: tests/test_audio_ref64_cpu.py), through HipOps like tests/test_gpu_ops.py:

  csrc/frontend.hip     fbank_kernel (n_samples 399 ... 12000, win 255 ... 512 on both sides of the second-sample branch, shift 1 /
                        160 / 400, n_mels 1 / 80 / 300 and the 257 x 257 identity matrix that holds every DFT bin on its own,
                        preemph 0, scale 1; the golden waveform, white noise, a sine on a bin centre, alternating samples,
                        impulses at sample 0 and win - 1, a constant frame, silence), lfr_cmvn_kernel ((7, 6), (1, 1), (4, 3),
                        (7, 1) x T = 1 ... 13, 100 x D = 80, 8, with and without CMVN)
  csrc/encoder_aux.hip  psd_frame_stats_kernel (V = 1 ... 25055, ties across lanes, waves and the 256-stride loop, dead frames),
                        psd_plan_kernel (T and lens 1 ... 769: runs across 255|256 and 511|512, a run of 300, lanes 63 and 64 kept,
                        an empty wave, an empty chunk, blank_id < 0, a mean equal to the threshold), psd_gather_kernel (a segment
                        of 300 frames, Tout below / equal / above max(new_lens), widths 50 ... 560, ldp != ldo), and the chain
                        stats -> plan -> gather at B = 3, T = 504 against oracle/tasu_oracle.py's psd()
  csrc/misc.hip         posterior_kernel, embed_merge_kernel, merge_bwd_kernel (M = 1 ... 61 x D = 4 ... 1536; bf16 ties, the
                        largest finite value, subnormals, -0.0)

Every output and workspace starts as NaN (integers: -7); guard rows keep their bits; operands are poisoned inside their
allocations (NaN behind n_samples and behind lens[b], 2.0 in the posterior's pad columns).  Integer outputs and data movement bit
for bit; arithmetic within 1.0 x E on every element.  fbank also: silence is the floor with equal bits everywhere, dropping 3 hops
shifts the rows bit for bit, two runs give equal bits.  The AUDIO64RMS lines print, per profile, the kernel's rms error over the
elements with E <= 1e-4 next to the numpy fp32 restatement's on the same frames (reported, not asserted).

Measured on MI355X (168 tests, 1.3 s for the file, the slowest test 0.09 s): every check passes.  Largest |err| / E per operation (the
F64WORST lines): fbank 0.504 (the sine through the identity matrix; 0.438 on the golden waveform, 0.396 on white noise),
psd_gather 0.783, the chain 0.663, posterior_build 0.916; lfr_cmvn, psd_frame_stats, psd_plan, embed_merge, merge_bwd: bits.
fbank allowance shares (elements with E <= 1e-4): white noise 95.7 %, golden waveform 86.4 %.  rms error over those elements,
kernel / numpy fp32 restatement: white noise 1.69e-6 / 1.11e-6, golden 1.60e-6 / 1.32e-6 (reported, not asserted).  No kernel
needed a fix.  Scratch mutants of the kernels: one was run on the GPU -- psd_plan_kernel numbering each chunk's
segments from 0 fails 10 tests of this file (all plan cases with more than 256 frames and the chain); the other eight of the issue
were built but not run on the GPU, and are held by their CPU restatements in tests/test_audio_ref64_cpu.py only."""
import pytest
import torch

import audio_ref64 as A

pytestmark = pytest.mark.gpu
F64, F32, BF, I32 = torch.float64, torch.float32, torch.bfloat16, torch.int32


@pytest.fixture(scope="module")
def hip():
    from ps_slm_amd.ops import HipOps
    return HipOps()


def cuda(t):
    return t.cuda()


_worst = {}


def hold(op, what, got, ref):
    w = A.check(got, ref, f"{op} {what}")
    _worst[op] = max(_worst.get(op, 0.0), w)
    print(f"F64WORST {op} {what} |err| / E {w:.3f} (largest so far for {op}: {_worst[op]:.3f})")


# ------------------------------------------------------------------------------------------------ csrc/frontend.hip
@pytest.mark.parametrize("case", A.FB_CASES, ids=A.case_id)
def test_fbank(hip, case):
    d = A.fb_inputs(case)
    ref = A.fb_reference(d)
    got = A.run_fbank(hip, d, cuda)
    if d["T"] == 0:                                              # no frame: the NaN output was checked untouched
        return
    hold("fbank", A.case_id(case), got, ref)
    k, share = A.fb_sharp_rms(got["out"], ref)
    r, _ = A.fb_sharp_rms(A.fb_restatement_f32(d), ref)
    print(f"AUDIO64RMS fbank {A.case_id(case)}: share of E <= 1e-4 {100 * share:.1f} %, rms error there kernel {k:.2e}, fp32 restatement {r:.2e}")
    A.same_bits(A.run_fbank(hip, d, cuda)["out"], got["out"], "fbank, second run")
    if case.wave == "silence":
        A.same_bits(got["out"], torch.full_like(got["out"], float(got["out"][0, 0])), "fbank of silence")


def test_fbank_frames_depend_on_their_own_samples_only(hip):
    c = next(c for c in A.FB_CASES if c.wave == "golden" and c.n == 12000)
    a = A.run_fbank(hip, A.fb_inputs(c), cuda)["out"]
    b = A.run_fbank(hip, A.fb_inputs(c, drop=3 * c.shift), cuda)["out"]
    A.same_bits(a[3:].contiguous(), b, "fbank with 3 hops dropped")


@pytest.mark.parametrize("case", A.LFR_CASES, ids=A.case_id)
def test_lfr_cmvn(hip, case):
    for T in A.LFR_T:
        d = A.lfr_inputs(case, T)
        hold("lfr_cmvn", f"{A.case_id(case)} T={T}", A.run_lfr(hip, d, cuda), A.lfr_reference(d))


# ------------------------------------------------------------------------------------------------ csrc/encoder_aux.hip
@pytest.mark.parametrize("case", A.STAT_CASES, ids=A.case_id)
def test_psd_frame_stats(hip, case):
    d = A.stat_inputs(case)
    hold("psd_frame_stats", A.case_id(case), A.run_stats(hip, d, cuda), A.stat_reference(d))


@pytest.mark.parametrize("name", A.PLAN_CASES)
def test_psd_plan(hip, name):
    d = A.plan_inputs(name)
    hold("psd_plan", name, A.run_plan(hip, d, cuda), A.plan_reference(d))


@pytest.mark.parametrize("case", A.GATHER_CASES, ids=A.case_id)
def test_psd_gather(hip, case):
    d = A.gather_inputs(case)
    hold("psd_gather", A.case_id(case), A.run_gather(hip, d, cuda), A.gather_reference(d))


def test_psd_chain_against_the_oracle(hip):
    d = A.chain_inputs()
    ref, Tout = A.chain_reference(d)
    got, tout = A.run_chain(hip, d, cuda)
    assert tout == Tout
    hold("psd chain", "B=3 T=504 V=64", got, ref)


# ------------------------------------------------------------------------------------------------ csrc/misc.hip
@pytest.mark.parametrize("case", A.POST_CASES, ids=A.case_id)
def test_posterior_build(hip, case):
    d = A.post_inputs(case)
    hold("posterior_build", A.case_id(case), A.run_post(hip, d, cuda), A.post_reference(d))


@pytest.mark.parametrize("case", A.MERGE_CASES, ids=A.case_id)
def test_embed_merge(hip, case):
    d = A.merge_inputs(case)
    hold("embed_merge", A.case_id(case), A.run_merge(hip, d, cuda), A.merge_reference(d))


@pytest.mark.parametrize("case", A.MERGE_CASES, ids=A.case_id)
def test_merge_bwd(hip, case):
    d = A.bwd_inputs(case)
    hold("merge_bwd", A.case_id(case), A.run_bwd(hip, d, cuda), A.bwd_reference(d))
