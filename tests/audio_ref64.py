"""TEST HELPER (not a test, never shipped): plain float64 restatements of the kernels that carry audio from the waveform to the
decoder's input rows -- the log-mel filterbank and LFR / CMVN (csrc/frontend.hip), PSD's frame statistics, plan and gather
(csrc/encoder_aux.hip), the text posterior, the embedding merge and its backward (csrc/misc.hip) -- on the exact input values,
with a bound E for every arithmetic element and the bits of everything else.  Nothing is shared with the kernels or with
tests/fake_ops.py.  `Ref`, `check`, `untouched`, `same_bits`, `nan`, `case_id` are those of tests/row_ref64.py; e = 2^-24.

RULES.  Every output and workspace starts as NaN (integers: -7) with guard rows that must keep their bits; operands carry poison
inside their allocation (NaN behind the waveform's n_samples, behind lens[b] and in front of the body view; 2.0 in the
posterior's pad columns; garbage or the repeated last id in `fid` behind lens[b]).  Integers and pure data movement: the
reference's bits.  Arithmetic: |got - ref| <= 1.0 E on every element, exactly the reference where E = 0.

fbank.  The reference is float64 throughout on the fp32 operands as given (wave, window, mel matrix; scale is a power of two, so
x = wave * scale is exact): frame, subtract the mean, d_i = c_i - p c_max(i-1, 0), v = d w, zero-pad to 512, DFT, |X|^2, mel,
max(., 2^-23), log.  E is first order in e and built from the float64 intermediates of the same radix-2 decimation-in-time
network the kernel runs (bit-reversed input, nine stages; `_fft_stages`):
    mean        block_sum<4> of a0 + a1: 1 + 6 shuffle levels + 4 waves, the division: E_mu = 12 e sum |x| / win.  A mean error
                moves every d_i by (1 - p) E_mu TOGETHER: it reaches bin k as (1 - p) E_mu |W_k|, W the window's DFT.  This is
                the term that scales with the frame's magnitude before DC removal: a constant frame is silent in float64 and
                leaves this residue on the device.
    roundings   of c_i (which is in d_i and, times p, in d_(i+1)), p c_(i-1), d_i, v_i (each e relative), of every butterfly
                (re cs, im sn, their difference, and the same for the imaginary part: squares that add up to 2 |b|^2; none in
                stages 0 and 1 whose twiddles are 1 and -i; each sum e |out|): the roundings that reach bin k are independent
                of each other, every one bounded by e |t|.  They enter as 4 e sqrt(sum t^2), t over
                the elements of each stage that feed bin k (one per group): a rounding error has standard deviation at most
                e |t| / sqrt 3, so this is 6.9 standard deviations of their sum (Hoeffding: exceeded with probability below
                7e-4 by any distribution inside the bounds; the Gaussian tail is 5e-12).  The worst case sum e |t| is larger by
                about the square root of the number of terms (400 inputs, 512 / 2^(s+1) groups per stage) and cannot meet the
                share condition below; LAMBDA = 4 is fixed here and not fitted to any result.
    twiddles    sincospif of an exact argument, 2 ulp: |dw| <= 4 e.  Bin k meets ONE twiddle per stage, the same in every
                group, so its error is systematic: 4 e |T_(s, k)|, T the part of X_k that passes through the twiddled inputs of
                stage s, evaluated exactly in float64 (`_fft_stages`), summed over stages 2..8 without cancellation.
    power       2 e |X|^2 + 2 |X| E_X + E_X^2;  mel: linear over the bins (their errors share sources), (n_nz + 1) e mel for the
                serial sum over the non-zero weights;  floor and log: with b = max(mel, 2^-23),
                E = max(log1p(d / b), min(-log1p(-d / b), log(b / 2^-23))) + 4 e |log b|   (two ulp of logf)
                -- rigorous for any d: below the floor the result cannot move down.
Mel bins that are cancellation residues get a large E; tests/test_audio_ref64_cpu.py asserts the share of elements with
E <= 1e-4 on the white-noise and the golden waveform (`FB_SHARE`) and records the shares reached.

lfr_cmvn: bits of (fb[clamp(i n + j - (m - 1) // 2)] + mean) * scale in fp32 (the sum and the product cannot contract).
psd_frame_stats: first index of the row maximum, the operand's bits at blank_id; -1 / 0 for dead frames.
psd_plan: a sequential scan, the run sum in fp32 in frame order (the kernel's order): integers.  `plan_margins` is the float64
side check: no segment mean within fp32 rounding of the threshold unless the case constructs it.
psd_gather: s = sum_t x_t serially, / len: E = ((len - 1) e sum |x_t| ) / len + e |out|; len == 1: the operand's bits.
posterior_build: a / V one rounding, (1 - a) + a / V two; exact 0 / 1 where alpha is None or 0, a row of zeros behind id < 0.
embed_merge: bits.  merge_bwd: bits of round-to-nearest-even of the fp32 value (`rne_bf16`, integer arithmetic)."""
import collections
import math
import os

import numpy as np
import torch

from row_ref64 import (F32, F64, BF, I32, GUARD, LIMIT, NAN, Ref, _back, _call, bits, case_id, cdiv, check, e, first_argmax,  # noqa: F401
                       gen, nan, same_bits, untouched, worst_of)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fbank_kaldi_hf.npz")
NFFT, NBIN = 512, 257
FLOOR = 2.0 ** -23
LAMBDA = 4.0
FB_SHARE = {"noise": 0.95, "golden": 0.80}                      # least share of elements with E <= FB_SHARP
FB_SHARP = 1e-4


def ints(*shape):
    return torch.full(shape, -7, dtype=I32)


# ================================================================================================ fbank
FbCase = collections.namedtuple("FbCase", "wave n win shift n_mels preemph scale mel")


def _fb_cases():
    d = dict(win=400, shift=160, n_mels=80, preemph=0.97, scale=32768.0, mel="mel")
    C = lambda wave, n, **kw: FbCase(wave=wave, n=n, **dict(d, **kw))
    out = [C("golden", n) for n in (399, 400, 401, 559, 560, 720, 12000)]
    out += [C("noise", 12000)]
    out += [C("noise", 2000, win=w) for w in (255, 256, 257, 512)]
    out += [C("noise", 420, shift=1), C("noise", 2000, shift=400)]
    out += [C("noise", 2000, n_mels=1), C("noise", 2000, n_mels=300)]
    out += [C("noise", 2000, preemph=0.0), C("noise", 2000, scale=1.0), C("golden", 2000, preemph=0.0, scale=1.0)]
    out += [C(w, 720) for w in ("sine", "alt", "imp0", "impw", "const", "silence")]
    out += [C(w, 720, n_mels=NBIN, mel="eye") for w in ("noise", "sine", "alt", "imp0", "impw", "const")]
    out += [C("impw", 600, win=w, n_mels=NBIN, mel="eye") for w in (256, 257, 512)]
    return out


FB_CASES = _fb_cases()
FB_TAIL = 64                                                     # NaN samples behind n_samples


def hamming(win):
    n = np.arange(win, dtype=np.float64)
    return (0.54 - 0.46 * np.cos(2.0 * np.pi * n / (win - 1))).astype(np.float32)


def mel_matrix(n_mels):
    from oracle import fbank_oracle as fo
    return fo.mel_banks(n_mels, NFFT, 16000.0)


def fb_wave(c, drop=0):
    """the fp32 samples of a case (`drop`: samples left out at the front)"""
    n, i = c.n, np.arange(c.n, dtype=np.float64)
    if c.wave == "golden":
        w = np.load(GOLDEN)["wave"][:n].astype(np.float32)
        assert len(w) == n
    elif c.wave == "noise":
        w = 0.1 * np.random.default_rng(7).standard_normal(n)
    elif c.wave == "sine":                                       # the centre of bin 37
        w = 0.3 * np.sin(2 * np.pi * 37 * i / NFFT)
    elif c.wave == "alt":                                        # all energy in bin 256
        w = 0.2 * (1 - 2 * (i % 2))
    elif c.wave in ("imp0", "impw"):
        w = np.zeros(n)
        w[0 if c.wave == "imp0" else c.win - 1] = 0.5
    elif c.wave == "const":
        w = np.full(n, 0.25)
    else:
        w = np.zeros(n)
    return np.asarray(w, dtype=np.float32)[drop:]


def fb_inputs(c, drop=0):
    w = fb_wave(c, drop)
    n = len(w)
    buf = nan(n + FB_TAIL)
    buf[:n] = torch.from_numpy(w)
    mel = np.eye(NBIN, dtype=np.float32) if c.mel == "eye" else mel_matrix(c.n_mels)
    assert math.log2(c.scale) == int(math.log2(c.scale)), "scale must be a power of two (x = wave * scale is taken as exact)"
    T = 0 if n < c.win else 1 + (n - c.win) // c.shift
    return dict(wave=buf, n=n, win=c.win, shift=c.shift, n_mels=mel.shape[0], preemph=c.preemph, scale=c.scale, T=T,
                window=torch.from_numpy(hamming(c.win)), mel=torch.from_numpy(mel))


def _frames(d, dtype):
    idx = np.arange(d["win"])[None, :] + d["shift"] * np.arange(d["T"])[:, None]
    return d["wave"][:d["n"]].numpy().astype(dtype)[idx] * dtype(d["scale"])


BITREV = np.array([int(format(i, "09b")[::-1], 2) for i in range(NFFT)])


def _fft_stages(v):
    """the kernel's network on float64 rows [F, 512] (natural order in): X [F, 512], and per stage s the rows' intermediates
    (b = the twiddled inputs [F, 512 / 2^(s+1), 2^s], out = the stage's outputs in groups [F, 512 / 2^(s+1), 2^(s+1)])"""
    z = v[:, BITREV].astype(np.complex128)
    F = z.shape[0]
    st = []
    for s in range(9):
        half = 1 << s
        g = z.reshape(F, NFFT // (2 * half), 2, half)
        w = np.exp(-1j * np.pi * np.arange(half) / half)
        a, b = g[:, :, 0], g[:, :, 1]
        wb = w * b
        out = np.concatenate([a + wb, a - wb], -1)              # [F, groups, 2 half]
        st.append((b, out))
        z = out.reshape(F, NFFT)
    return z, st


def _through_b(st, s):
    """|T_(s, k)| [F, 512]: the modulus of the part of X_k that passes through the twiddled inputs of stage s"""
    b, out = st[s]
    F, half = b.shape[0], 1 << s
    w = np.exp(-1j * np.pi * np.arange(half) / half)
    z = np.concatenate([w * b, -(w * b)], -1).reshape(F, NFFT)  # the a inputs zeroed
    for t in range(s + 1, 9):
        h = 1 << t
        g = z.reshape(F, NFFT // (2 * h), 2, h)
        wb = np.exp(-1j * np.pi * np.arange(h) / h) * g[:, :, 1]
        z = np.concatenate([g[:, :, 0] + wb, g[:, :, 0] - wb], -1).reshape(F, NFFT)
    return np.abs(z)


def fb_reference(d):
    """Ref of one case: out [T, n_mels] with its E"""
    T, win, p = d["T"], d["win"], float(np.float32(d["preemph"]))
    if T == 0:
        return Ref({}, {})
    x = _frames(d, np.float64)
    w = d["window"].numpy().astype(np.float64)
    M = d["mel"].numpy().astype(np.float64)
    mu = x.mean(1, keepdims=True)
    c = x - mu
    pv = np.concatenate([c[:, :1], c[:, :-1]], 1)
    dd = c - p * pv
    v = np.zeros((T, NFFT))
    v[:, :win] = dd * w
    X, st = _fft_stages(v)
    assert np.allclose(X[:, :NBIN], np.fft.rfft(v, axis=1), rtol=0, atol=1e-9 * (1 + np.abs(v).sum(1, keepdims=True)))
    # --- systematic: the mean, the twiddles
    E_mu = 12 * e * np.abs(x).sum(1, keepdims=True) / win
    wz = np.zeros(NFFT)
    wz[:win] = w
    sysm = abs(1 - p) * E_mu * np.abs(np.fft.fft(wz))[None, :]
    for s in range(2, 9):
        sysm = sysm + 4 * e * _through_b(st, s)
    # --- independent roundings, squared: the inputs, then every stage's products and sums
    wn = np.concatenate([w[1:], [0.0]])                          # the rounding of c_i is in d_i and, times p, in d_(i+1)
    r2 = ((c * (w + p * wn)) ** 2 + (w ** 2) * ((p * pv) ** 2 + dd ** 2) + v[:, :win] ** 2).sum(1, keepdims=True)
    r2 = np.broadcast_to(r2, (T, NFFT)).copy()
    for s, (b, out) in enumerate(st):
        half = 1 << s
        t2 = (np.abs(out) ** 2).sum(1)                           # [F, 2 half]: one element per group feeds bin k
        if s >= 2:
            t2 = t2 + 2 * np.tile((np.abs(b) ** 2).sum(1), (1, 2))
        r2 += np.tile(t2, (1, NFFT // (2 * half)))
    E_X = (sysm + LAMBDA * e * np.sqrt(r2))[:, :NBIN]
    aX = np.abs(X[:, :NBIN])
    P = aX ** 2
    E_P = 2 * e * P + 2 * aX * E_X + E_X ** 2
    mel = P @ M.T
    nnz = (M != 0).sum(1)[None, :]
    dm = E_P @ np.abs(M).T + (nnz + 1) * e * (P @ np.abs(M).T)
    b = np.maximum(mel, FLOOR)
    r = dm / b
    with np.errstate(divide="ignore", invalid="ignore"):
        down = np.where(r < 1, -np.log1p(-np.minimum(r, 1 - 1e-16)), np.inf)
    ref = np.log(b)
    E = np.maximum(np.log1p(r), np.minimum(down, np.log(b / FLOOR))) + 4 * e * np.abs(ref)
    return Ref({"out": (torch.from_numpy(ref), torch.from_numpy(E))}, {})


def fb_restatement_f32(d):
    """the kernel's arithmetic in numpy fp32 (serial sums where the kernel reduces in a tree): the yardstick of the rms line, and
    in tests/test_audio_ref64_cpu.py a second fp32 implementation that E has to cover"""
    f = np.float32
    T, win, p = d["T"], d["win"], f(d["preemph"])
    x = _frames(d, np.float32)
    c = x - (x.sum(1, keepdims=True, dtype=f) / f(win))
    pv = np.concatenate([c[:, :1], c[:, :-1]], 1)
    v = np.zeros((T, NFFT), dtype=f)
    v[:, :win] = (c - p * pv) * d["window"].numpy()
    re, im = v[:, BITREV].copy(), np.zeros((T, NFFT), dtype=f)
    for s in range(9):
        half = 1 << s
        ang = -(np.arange(half, dtype=np.float64) / half) * np.pi
        cs, sn = np.cos(ang).astype(f), np.sin(ang).astype(f)
        R, I = re.reshape(T, -1, 2, half), im.reshape(T, -1, 2, half)
        br, bi = R[:, :, 1] * cs - I[:, :, 1] * sn, R[:, :, 1] * sn + I[:, :, 1] * cs
        re = np.concatenate([R[:, :, 0] + br, R[:, :, 0] - br], -1).reshape(T, NFFT)
        im = np.concatenate([I[:, :, 0] + bi, I[:, :, 0] - bi], -1).reshape(T, NFFT)
    P = (re * re + im * im)[:, :NBIN]
    mel = np.zeros((T, d["n_mels"]), dtype=f)
    Mw = d["mel"].numpy()
    for k in range(NBIN):
        mel += P[:, k:k + 1] * Mw[None, :, k]
    return torch.from_numpy(np.log(np.maximum(mel, f(FLOOR))).astype(f))


def run_fbank(ops, d, to=None):
    ops, to = _call(ops, to)
    T, nm = d["T"], d["n_mels"]
    out = to(nan(T + GUARD, nm))
    ops.fbank(to(d["wave"]), d["n"], d["scale"], d["win"], d["shift"], to(d["window"]), to(d["mel"]), nm, d["preemph"], out)
    (out,) = _back(out)
    assert untouched(out[T:]), "fbank: rows past the last frame were written"
    return {"out": out[:T]}


def fb_sharp_rms(got, ref):
    """(rms error over the elements with E <= FB_SHARP, their share)"""
    want, E = ref.tol["out"]
    keep = E <= FB_SHARP
    if not bool(keep.any()):
        return 0.0, 0.0
    return float((got.to(F64) - want)[keep].pow(2).mean().sqrt()), float(keep.double().mean())


# ================================================================================================ lfr_cmvn
LfrCase = collections.namedtuple("LfrCase", "m n D cmvn")
LFR_CASES = [LfrCase(m, n, D, cm) for m, n in ((7, 6), (1, 1), (4, 3), (7, 1)) for D in (80, 8) for cm in (1, 0)]
LFR_T = tuple(range(1, 14)) + (100,)


def lfr_inputs(c, T):
    g = gen(c.m, c.n, c.D, T, 3)
    fb = nan(T + 2, c.D)                                         # two NaN rows behind frame T - 1
    fb[:T] = torch.randn(T, c.D, generator=g) * 5 + 10
    W = c.m * c.D
    return dict(fb=fb, T=T, D=c.D, m=c.m, n=c.n, Tl=cdiv(T, c.n), means=torch.randn(W, generator=g) if c.cmvn else None,
                scales=torch.rand(W, generator=g) + 0.5 if c.cmvn else None)


def lfr_reference(d):
    """the padded-sequence definition: (m - 1) // 2 copies of frame 0 in front, copies of the last frame behind"""
    T, m, n = d["T"], d["m"], d["n"]
    fb = d["fb"][:T].numpy()
    seq = np.concatenate([np.repeat(fb[:1], (m - 1) // 2, 0), fb, np.repeat(fb[-1:], m + n, 0)], 0)
    out = np.stack([seq[i * n:i * n + m].reshape(-1) for i in range(d["Tl"])]).astype(np.float32)
    if d["means"] is not None:
        out = (out + d["means"].numpy()[None, :]) * d["scales"].numpy()[None, :]
    return Ref({}, {"out": torch.from_numpy(out.astype(np.float32))})


def run_lfr(ops, d, to=None):
    ops, to = _call(ops, to)
    Tl = d["Tl"]
    out = to(nan(Tl + GUARD, d["m"] * d["D"]))
    ops.lfr_cmvn(to(d["fb"]), d["T"], d["D"], d["m"], d["n"], None if d["means"] is None else to(d["means"]),
                 None if d["scales"] is None else to(d["scales"]), out)
    (out,) = _back(out)
    assert untouched(out[Tl:]), "lfr_cmvn: rows past ceil(T / lfr_n) were written"
    return {"out": out[:Tl]}


# ================================================================================================ PSD: buffers
HEAD = 4                                                         # psd_on_device: the body view starts at row 4, bstride = T + 4


def body_buffer(B, T, ld, rows, lens, pad=2.0):
    """[HEAD + B (T + HEAD), ld] fp32: NaN everywhere, `rows` [B, T, V] on the live frames, `pad` in their columns [V, ld).  Row
    (b, t) of the view buf[HEAD:] is b (T + HEAD) + t: the last one is the allocation's last row."""
    V = rows.shape[-1]
    bs = T + HEAD
    buf = nan(B * bs, ld)
    for b in range(B):
        L = int(lens[b])
        buf[HEAD + b * bs:HEAD + b * bs + L, :V] = rows[b, :L]
        buf[HEAD + b * bs:HEAD + b * bs + L, V:] = pad
    return buf


# ================================================================================================ psd_frame_stats
StatCase = collections.namedtuple("StatCase", "V blank")
STAT_CASES = [StatCase(V, bl) for V in (1, 255, 256, 257, 1000, 25055) for bl in ("first", "last")]


def tie_profiles(V):
    """(name, columns that hold the row's maximum); `None`: the whole row equal / zero"""
    out = [("none", ())]
    for a, b in ((5, 5 + 256), (63, 64), (255, 256), (0, V - 1), (70, 70 + 512), (300, 300 + 256 * 3)):
        if b < V and a != b:
            out.append((f"{a}={b}", (a, b)))
    return out + [("equal", None), ("zero", None)]


def stat_inputs(c):
    V = c.V
    prof = tie_profiles(V)
    T, B = len(prof), 3
    ld = cdiv(V + 1, 64) * 64
    g = gen(V, 9)
    rows = torch.rand(B, T, V, generator=g) * 0.5
    for b in range(B):
        for t, (name, cols) in enumerate(prof):
            if name == "equal":
                rows[b, t] = 0.375
            elif name == "zero":
                rows[b, t] = 0.0
            else:
                for col in cols:
                    rows[b, t, col] = 0.75
    lens = torch.tensor([0, 1, T], dtype=I32)
    return dict(post=body_buffer(B, T, ld, rows, lens), rows=rows, lens=lens, B=B, T=T, V=V, ld=ld, blank=0 if c.blank == "first" else V - 1,
                profiles=prof)


def stat_reference(d):
    B, T, bl = d["B"], d["T"], d["blank"]
    live = torch.arange(T)[None] < d["lens"][:, None]
    fid = torch.where(live, first_argmax(d["rows"].to(F64).reshape(B * T, -1)).view(B, T), torch.full((B, T), -1))
    fb = torch.where(live, d["rows"][..., bl], torch.zeros(B, T))
    return Ref({}, {"fid": fid.reshape(-1).to(I32), "fblank": fb.reshape(-1)})


def run_stats(ops, d, to=None):
    ops, to = _call(ops, to)
    B, T = d["B"], d["T"]
    n = B * T
    fid, fb = to(ints(n + GUARD)), to(nan(n + GUARD))
    ops.psd_frame_stats(to(d["post"])[HEAD:], to(d["lens"]), fid[:n], fb[:n], B, T, T + HEAD, d["V"], d["blank"])
    fid, fb = _back(fid, fb)
    assert untouched(fid[n:]) and untouched(fb[n:]), "psd_frame_stats: wrote past B x T frames"
    return {"fid": fid[:n], "fblank": fb[:n]}


# ================================================================================================ psd_plan
PLAN_CASES = ["random769", "random257", "one", "t255", "t256", "t504", "t513", "cross", "long", "blanks", "lanes", "garbage", "identity",
              "threshold"]
THR = float(np.float32(0.9))                                     # the fp32 value the library receives for 0.90


def _runs(g, L, lo=1, hi=6, p_blank=0.3, p_drop=0.3):
    """ids and blank probabilities of L frames: runs of 1..hi equal non-blank ids, single blanks between some; a run's frames are
    all low (kept) or all high (dropped), so no mean comes near the threshold"""
    ids, bp = [], []
    prev = -1
    while len(ids) < L:
        if float(torch.rand(1, generator=g)) < p_blank:
            k, i = 1, 0
        else:
            k = int(torch.randint(lo, hi + 1, (1,), generator=g))
            i = int(torch.randint(1, 20, (1,), generator=g))
            while i == prev:
                i = i % 19 + 1
        drop = float(torch.rand(1, generator=g)) < p_drop
        v = torch.rand(k, generator=g) * (0.06 if drop else 0.8) + (0.93 if drop else 0.0)
        ids += [i] * k
        bp += v.tolist()
        prev = i
    return torch.tensor(ids[:L], dtype=I32), torch.tensor(bp[:L], dtype=F32)


def plan_inputs(name):
    g = gen(len(name), sum(map(ord, name)))
    blank, thr, exact = 0, THR, False
    shapes = {"random769": (769, (769, 513, 504, 257, 0)), "random257": (257, (257, 256, 255, 1, 0)), "one": (1, (1,)), "t255": (255, (255, 0)),
              "t256": (256, (256, 255)), "t504": (504, (504, 300)), "t513": (513, (513, 512)), "identity": (769, (769, 513, 504, 257, 0)),
              "garbage": (257, (257, 100, 0))}
    T, lens = shapes.get(name, (769, (769, 600)))
    B = len(lens)
    fid, fbl = ints(B, T), nan(B, T)
    for b, L in enumerate(lens):
        ids, bp = _runs(g, L)
        if name == "cross" and L:                                # runs across 255|256 and 511|512, the first frame of a chunk continuing
            ids[250:262], bp[250:262] = 21 + b, 0.25
            ids[505:520], bp[505:520] = 23 + b, 0.5 if b == 0 else 0.97
            ids[249], ids[262], ids[504], ids[520] = 1, 2, 3, 4
        if name == "long" and L:                                 # 300 equal ids: longer than a chunk; then a second one that is dropped
            ids[100:400], bp[100:400] = 21, torch.rand(300, generator=g) * 0.5
            ids[99], ids[400] = 1, 2
            if b == 1:
                ids[256:556], bp[256:556] = 22, 0.96             # starts on a chunk's first frame
                ids[99:256], ids[556] = 21, 2
        if name == "blanks" and L:                               # every frame blank: its own segment, kept and dropped in turn
            ids[:] = 0
            bp[:] = torch.where(torch.arange(L) % 3 == 1, 0.95, 0.4) + torch.rand(L, generator=g) * 0.04
        if name == "lanes" and L:                                # every frame its own segment; lanes 63 and 64 kept, a wave and a chunk empty
            ids[:] = (torch.arange(L) % 17 + 1).to(I32)
            keep = torch.rand(L, generator=g) < 0.6
            keep[63], keep[64], keep[255], keep[512], keep[513] = True, True, True, True, b == 0
            keep[128:192] = False
            keep[256:512] = False
            bp[:] = torch.where(keep, 0.3, 0.95) + torch.rand(L, generator=g) * 0.04
        fid[b, :L], fbl[b, :L] = ids, bp
        if L:
            fid[b, L:] = int(torch.randint(0, 20, (1,), generator=g)) if name == "garbage" else ids[L - 1]   # behind lens[b]
    if name == "identity":                                       # the do_psd = false call
        blank, thr = -2, 2.0
    if name == "threshold":                                      # a mean that EQUALS the threshold is dropped, one ulp below it is kept
        T, lens, exact = 8, (8,), True
        t9 = np.float32(0.9)
        below = np.nextafter(t9, np.float32(0))
        fid = torch.tensor([[5, 5, 6, 6, 0, 0, 7, 8]], dtype=I32)
        fbl = torch.tensor([[t9, t9, below, below, t9, below, t9, below]], dtype=F32)
        B = 1
    return dict(fid=fid, fblank=fbl, lens=torch.tensor(lens, dtype=I32), B=B, T=T, blank=blank, thr=thr, exact=exact, name=name)


def _segments(ids, L, blank):
    """[(start, length)] of one utterance: runs of equal non-blank ids; blanks (blank < 0: all frames) stay single"""
    out, s = [], 0
    for t in range(1, L + 1):
        if t == L or blank < 0 or ids[s] == blank or ids[t] != ids[s]:
            out.append((s, t - s))
            s = t
    return out


def plan_reference(d):
    B, T = d["B"], d["T"]
    ss, sl, nl = ints(B * T + GUARD), ints(B * T + GUARD), ints(B + GUARD)
    thr = np.float32(d["thr"])
    for b in range(B):
        L = int(d["lens"][b])
        ids, bp = d["fid"][b].tolist(), d["fblank"][b].numpy()
        n = 0
        for s, ln in _segments(ids, L, d["blank"]):
            acc = np.float32(0)
            for t in range(s, s + ln):
                acc = np.float32(acc + bp[t])
            mean = acc if ln == 1 else np.float32(acc / np.float32(ln))
            if mean < thr:
                ss[b * T + n], sl[b * T + n] = s, ln
                n += 1
        nl[b] = n
    return Ref({}, {"seg_start": ss, "seg_len": sl, "new_lens": nl})


def plan_margins(d):
    """float64 side check: (smallest |mean - thr| / fp32 rounding of that mean, number of means equal to thr)"""
    worst, equal = math.inf, 0
    thr = float(np.float32(d["thr"]))
    for b in range(d["B"]):
        L = int(d["lens"][b])
        bp = d["fblank"][b].to(F64)
        for s, ln in _segments(d["fid"][b].tolist(), L, d["blank"]):
            mean = float(bp[s:s + ln].sum()) / ln
            if mean == thr:
                equal += 1
                continue
            worst = min(worst, abs(mean - thr) / ((ln + 1) * e * max(mean, thr)))
    return worst, equal


def run_plan(ops, d, to=None):
    """the whole buffers, guard elements included: everything at and past new_lens[b] keeps -7"""
    ops, to = _call(ops, to)
    B, T = d["B"], d["T"]
    ss, sl, nl = to(ints(B * T + GUARD)), to(ints(B * T + GUARD)), to(ints(B + GUARD))
    ops.psd_plan(to(d["fid"].reshape(-1)), to(d["fblank"].reshape(-1)), to(d["lens"]), ss[:B * T], sl[:B * T], nl[:B], B, T, d["blank"], d["thr"])
    ss, sl, nl = _back(ss, sl, nl)
    return {"seg_start": ss, "seg_len": sl, "new_lens": nl}


# ================================================================================================ psd_gather
GatherCase = collections.namedtuple("GatherCase", "plan V tout")   # tout: "below", "equal", "above" max(new_lens)
GATHER_W = {50: (64, 64), 203: (256, 256), 257: (320, 320), 560: (560, 576)}     # V -> (ldp, ldo); 560: the raw-feature source


def _gather_cases():
    out = [GatherCase("hand", V, t) for V in GATHER_W for t in ("below", "equal", "above")]
    out += [GatherCase(p, V, t) for p, V, t in (("random769", 50, "equal"), ("long", 203, "below"), ("cross", 257, "above"),
                                                ("lanes", 560, "below"), ("random257", 560, "equal"), ("identity", 50, "below"))]
    return out


GATHER_CASES = _gather_cases()


def gather_inputs(c):
    if c.plan == "hand":                                         # segments of 300, 1, 2, 7 frames; an utterance with none; one frame
        T, lens = 320, (320, 40, 1)
        segs = [[(0, 1), (1, 300), (301, 2), (310, 7)], [], [(0, 1)]]
        B = len(lens)
        ss, sl = ints(B * T), ints(B * T)
        for b, sg in enumerate(segs):
            for j, (s, n) in enumerate(sg):
                ss[b * T + j], sl[b * T + j] = s, n
        nl = torch.tensor([len(s) for s in segs], dtype=I32)
        lens = torch.tensor(lens, dtype=I32)
    else:
        p = plan_inputs(c.plan)
        r = plan_reference(p)
        B, T, lens = p["B"], p["T"], p["lens"]
        ss, sl, nl = r.exact["seg_start"][:B * T], r.exact["seg_len"][:B * T], r.exact["new_lens"][:B]
    ldp, ldo = GATHER_W[c.V]
    g = gen(c.V, len(c.plan), 13)
    rows = torch.randn(B, T, c.V, generator=g) * 3 if c.V == 560 else torch.rand(B, T, c.V, generator=g)
    mx = int(nl.max())
    Tout = {"below": max(mx - 2, 1), "equal": mx, "above": mx + 3}[c.tout]
    return dict(src=body_buffer(B, T, ldp, rows, lens), rows=rows, B=B, T=T, V=c.V, ldp=ldp, ldo=ldo, Tout=Tout, seg_start=ss, seg_len=sl,
                new_lens=nl)


def gather_reference(d):
    B, T, V, Tout, ldo = d["B"], d["T"], d["V"], d["Tout"], d["ldo"]
    out, E = torch.zeros(B * Tout, ldo, dtype=F64), torch.zeros(B * Tout, ldo, dtype=F64)
    x = d["rows"].to(F64)
    for b in range(B):
        for j in range(min(int(d["new_lens"][b]), Tout)):
            s, n = int(d["seg_start"][b * T + j]), int(d["seg_len"][b * T + j])
            seg = x[b, s:s + n]
            o = seg.sum(0) / n
            out[b * Tout + j, :V] = o
            if n > 1:
                E[b * Tout + j, :V] = (n - 1) * e * seg.abs().sum(0) / n + e * o.abs()
    return Ref({"out": (out, E)}, {})


def run_gather(ops, d, to=None):
    ops, to = _call(ops, to)
    n = d["B"] * d["Tout"]
    out = to(nan(n + GUARD, d["ldo"]))
    ops.psd_gather(to(d["src"])[HEAD:], to(d["seg_start"]), to(d["seg_len"]), to(d["new_lens"]), out[:n], d["B"], d["T"], d["T"] + HEAD,
                   d["Tout"], d["V"])
    (out,) = _back(out)
    assert untouched(out[n:]), "psd_gather: rows past B x Tout were written"
    return {"out": out[:n]}


# ------------------------------------------------------------------------------------------------ the chain
CHAIN_B, CHAIN_T, CHAIN_V, CHAIN_LD, CHAIN_LENS = 3, 504, 64, 128, (504, 300, 257)


def chain_inputs():
    """a peaked fp32 posterior [B, T, V]: runs of a dominant id, blank frames with a high or a low blank probability"""
    g = gen(504, 64, 17)
    B, T, V = CHAIN_B, CHAIN_T, CHAIN_V
    x = torch.randn(B, T, V, generator=g, dtype=F64)
    for b in range(B):
        ids, bp = _runs(g, T, p_drop=0.5)
        peak = torch.where((ids == 0) & (bp < 0.9), 5.0, 8.0).to(F64)   # a blank frame at about 0.6 is kept, at about 0.97 dropped
        x[b, torch.arange(T), ids.long()] += peak
    post = torch.softmax(x, -1).to(F32)
    lens = torch.tensor(CHAIN_LENS, dtype=I32)
    return dict(post3=post, post=body_buffer(B, T, CHAIN_LD, post, lens), lens=lens, B=B, T=T, V=V, ld=CHAIN_LD, blank=0, thr=THR)


def chain_plan_inputs(d):
    """the frame statistics of the chain's posterior, as plan inputs"""
    B, T = d["B"], d["T"]
    live = torch.arange(T)[None] < d["lens"][:, None]
    fid = torch.where(live, first_argmax(d["post3"].to(F64).reshape(B * T, -1)).view(B, T), torch.full((B, T), -1)).to(I32)
    return dict(fid=fid, fblank=torch.where(live, d["post3"][..., 0], torch.zeros(B, T)), lens=d["lens"], B=B, T=T, blank=0, thr=d["thr"],
                exact=False, name="chain")


def chain_reference(d):
    """oracle/tasu_oracle.py's psd() on the same posterior in float64: Ref of the rows [B * Tout, ld] (E = len e mean for a run of
    len > 1 non-negative rows, the operand's bits for a single frame), new_lens, the plan's seg_len [B, T]"""
    from oracle import tasu_oracle as O
    B, T, V = d["B"], d["T"], d["V"]
    p64 = d["post3"].to(F64)
    rows, nl = O.psd(p64, d["lens"].long(), p64, blank_id=0, blank_threshold=d["thr"])
    plan = plan_reference(chain_plan_inputs(d))
    sl = plan.exact["seg_len"][:B * T].view(B, T)
    assert torch.equal(plan.exact["new_lens"][:B].long(), nl), "the oracle's psd() and the sequential scan disagree on the lengths"
    Tout = int(nl.max())
    out, E = torch.zeros(B, Tout, d["ld"], dtype=F64), torch.zeros(B, Tout, d["ld"], dtype=F64)
    out[..., :V] = rows
    n = sl[:, :Tout].clamp_min(0).to(F64)[..., None]
    E[..., :V] = torch.where(n > 1, n * e * rows, torch.zeros_like(rows))
    return Ref({"out": (out.view(B * Tout, -1), E.view(B * Tout, -1))}, {"new_lens": nl.to(I32), "seg_len": sl.contiguous()}), Tout


def run_chain(ops, d, to=None):
    ops, to = _call(ops, to)
    B, T, V = d["B"], d["T"], d["V"]
    n = B * T
    post = to(d["post"])[HEAD:]
    lens = to(d["lens"])
    fid, fb = to(ints(n + GUARD)), to(nan(n + GUARD))
    ss, sl, nl = to(ints(n + GUARD)), to(ints(n + GUARD)), to(ints(B + GUARD))
    ops.psd_frame_stats(post, lens, fid[:n], fb[:n], B, T, T + HEAD, V, d["blank"])
    ops.psd_plan(fid[:n], fb[:n], lens, ss[:n], sl[:n], nl[:B], B, T, d["blank"], d["thr"])
    (nlh,) = _back(nl)
    Tout = int(nlh[:B].max())
    out = to(nan(B * Tout + GUARD, d["ld"]))
    ops.psd_gather(post, ss[:n], sl[:n], nl[:B], out[:B * Tout], B, T, T + HEAD, Tout, V)
    fid, fb, ss, sl, out = _back(fid, fb, ss, sl, out)
    assert untouched(out[B * Tout:]) and untouched(nlh[B:]) and untouched(ss[n:]) and untouched(sl[n:]) and untouched(fid[n:]) and untouched(fb[n:])
    return {"new_lens": nlh[:B], "seg_len": sl[:n].view(B, T), "out": out[:B * Tout]}, Tout


# ================================================================================================ posterior_build
PostCase = collections.namedtuple("PostCase", "R V ld alpha")
POST_CASES = [PostCase(R, V, ld, a) for R in (1, 40) for V, ld in ((203, 256), (256, 256), (25055, 25088)) for a in ("none", "zero", "random")]


def post_inputs(c):
    g = gen(c.R, c.V, 19)
    ids = torch.randint(0, c.V, (c.R,), generator=g).to(I32)
    if c.R > 1:
        ids[0], ids[1], ids[2], ids[5::7] = 0, c.V - 1, -1, -1
    else:
        ids[0] = c.V - 1
    alpha = None if c.alpha == "none" else (torch.zeros(c.R) if c.alpha == "zero" else torch.rand(c.R, generator=g) * 0.3)
    return dict(ids=ids, alpha=alpha, R=c.R, V=c.V, ld=c.ld)


def post_reference(d):
    R, V, ld = d["R"], d["V"], d["ld"]
    a = (d["alpha"] if d["alpha"] is not None else torch.zeros(R)).to(F64)
    ok = d["ids"] >= 0
    base = torch.where(ok, a / V, torch.zeros(R, dtype=F64))
    out, E = torch.zeros(R, ld, dtype=F64), torch.zeros(R, ld, dtype=F64)
    out[:, :V], E[:, :V] = base[:, None], (e * base)[:, None]
    r = torch.nonzero(ok)[:, 0]
    peak = (1 - a) + base
    out[r, d["ids"][r].long()] = peak[r]
    E[r, d["ids"][r].long()] = torch.where(a[r] == 0, torch.zeros(len(r), dtype=F64), 2 * e * peak[r])
    return Ref({"out": (out, E)}, {})


def run_post(ops, d, to=None):
    ops, to = _call(ops, to)
    R = d["R"]
    out = to(nan(R + GUARD, d["ld"]))
    ops.posterior_build(to(d["ids"]), None if d["alpha"] is None else to(d["alpha"]), out, R, d["V"])
    (out,) = _back(out)
    assert untouched(out[R:]), "posterior_build: rows past R were written"
    return {"out": out[:R]}


# ================================================================================================ embed_merge, merge_bwd
MergeCase = collections.namedtuple("MergeCase", "M D kinds")
MERGE_M, MERGE_D = (1, 3, 4, 5, 61), (4, 252, 256, 260, 1536)
MERGE_CASES = [MergeCase(M, D, "mixed") for M in MERGE_M for D in MERGE_D] + [MergeCase(M, D, "none") for M, D in ((5, 260), (61, 256))]
MERGE_VT, MERGE_R = 7, 9


def merge_inputs(c):
    g = gen(c.M, c.D, 23)
    M, D = c.M, c.D
    kind = (torch.arange(M) + int(torch.randint(0, 3, (1,), generator=g))) % 3 if c.kinds == "mixed" else torch.zeros(M, dtype=torch.long)
    idx = torch.where(kind == 1, torch.randint(0, MERGE_VT, (M,), generator=g), torch.randint(0, MERGE_R, (M,), generator=g))
    idx = torch.where(kind == 0, torch.zeros_like(idx), idx)
    return dict(table=torch.randn(MERGE_VT, D, generator=g), proj=torch.randn(MERGE_R, D, generator=g).to(BF), kind=kind.to(I32), idx=idx.to(I32), M=M, D=D)


def merge_reference(d):
    x = torch.zeros(d["M"], d["D"])
    for m in range(d["M"]):
        k, i = int(d["kind"][m]), int(d["idx"][m])
        if k == 1:
            x[m] = d["table"][i]
        elif k == 2:
            x[m] = d["proj"][i].float()
    return Ref({}, {"x": x})


def run_merge(ops, d, to=None):
    ops, to = _call(ops, to)
    M, D = d["M"], d["D"]
    x = to(nan(M + GUARD, D))
    ops.embed_merge(to(d["table"]), to(d["proj"]), to(d["kind"]), to(d["idx"]), x, M, D)
    (x,) = _back(x)
    assert untouched(x[M:]), "embed_merge: rows past M were written"
    return {"x": x[:M]}


def rne_bf16(x):
    """fp32 -> bf16, round to nearest, ties to even, in integer arithmetic on the bits (no NaN among the inputs)"""
    b = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = (b + 0x7FFF + ((b >> 16) & 1)) >> 16
    r = r & 0xFFFF
    return torch.where(r >= 0x8000, r - 0x10000, r).to(torch.int16).view(BF)


def bwd_special_values():
    """fp32 values on and one ulp either side of bf16 ties (towards both an even and an odd neighbour), the largest finite value,
    subnormals, zeros"""
    pats = []
    for hi in (0x3F80, 0x3F81, 0xC07F, 0x0080, 0x7F7F, 0x4000):  # even and odd bf16 mantissas, either sign, the smallest normal
        for lo in (0x7FFF, 0x8000, 0x8001, 0x0001, 0xFFFF):
            pats.append((hi << 16) | lo)
    pats += [0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x80008001, 0x80000000, 0x00000000]
    t = torch.tensor([p - (1 << 32) if p >= (1 << 31) else p for p in pats], dtype=torch.int64).to(torch.int32)
    return t.view(F32)


def bwd_inputs(c):
    g = gen(c.M, c.D, 29)
    n, D, Mx = c.M, c.D, 6
    dx = torch.randn(Mx, D, generator=g)
    sp = bwd_special_values()
    flat = dx.view(-1)                                           # row 0 (D = 4: all rows) starts with them ...
    flat[:min(len(sp), flat.numel())] = sp[:flat.numel()]
    if D >= 2 * len(sp):
        dx[0, D - len(sp):] = sp                                 # ... and ends with them: the row's last vectors
    rows = torch.randint(0, Mx, (n,), generator=g).to(I32)
    rows[0] = 0 if c.kinds == "mixed" else -1
    if c.kinds == "none":
        rows[:] = -1
    elif n > 1:
        rows[1::3] = -1
    return dict(dx=dx, rows=rows, n=n, D=D)


def bwd_reference(d):
    out = torch.zeros(d["n"], d["D"], dtype=BF)
    for r in range(d["n"]):
        m = int(d["rows"][r])
        if m >= 0:
            out[r] = rne_bf16(d["dx"][m])
    return Ref({}, {"dproj": out})


def run_bwd(ops, d, to=None):
    ops, to = _call(ops, to)
    n, D = d["n"], d["D"]
    o = to(nan(n + GUARD, D, dtype=BF))
    ops.merge_bwd(to(d["dx"]), to(d["rows"]), o, n, D)
    (o,) = _back(o)
    assert untouched(o[n:]), "merge_bwd: rows past n were written"
    return {"dproj": o[:n]}
