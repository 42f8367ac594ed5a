"""TEST HELPER (not a test, never shipped): generate(do_sample=True, num_beams > 1) restated -- the Gumbel keys' integer RNG in numpy
uint64, the row distribution and the keys in float64, and the bound the row kernels tasu_beam_sample_rows / tasu_f32_beam_sample_rows
(csrc/sample.hip) are held to.  Nothing is shared with the kernels or with tests/beam_sample_ops.py.

THE RNG.  For output row m, column v, generated position t:  z = mix64((seed ^ t * GOLD) + (m * V + v) * ODD) modulo 2^64 (mix64 the
splitmix64 finaliser of tests/sample_ref64.py),  u = ((z >> 41) + 1/2) * 2^-23: 23 bits and a half, exact in fp32, 2^-24 <= u <= 1 - 2^-24.

THE DISTRIBUTION (HF _beam_search with do_sample), per row on the fp32 logits x:
  lp = (x - max) - log sum exp(x - max);  lp' = lp < 0 ? lp * p : lp / p on the distinct history tokens;  banned columns -inf;
  s = lp' / T;  top-k keeps s >= the max(top_k, 2)-th largest s (ties kept, the pool's id cut as at one beam);  top-p: w = exp(s - max s),
  entries in descending (s, then ascending id) order, S_r = sum_{q >= r} w_q; the first r >= 2 with S_r <= (1 - top_p) S_0 and
  everything behind it go.  Nothing is renormalised.
THE DRAW.  a = s + run (the row's running score), key = a + G, G = -log(-log(u)); the row's K best by (key descending, id ascending).
Over an utterance's rows that is sampling without replacement in proportion to softmax(a) in Plackett-Luce order: the maximum of
a_i + G_i falls on i with probability exp(a_i) / sum exp(a), and the rest is the same draw on what remains.

THE BOUND.  e = 2^-24 (tests/row_ref64.py: an fp32 +, *, /: e relative; expf / logf and the hardware exp2 / log2 behind __expf /
__logf: 1 ulp = 2 e; __expf's argument product adds e |d| relative, __logf's product with ln 2 another e).
  * the sum Z^ of exp(x_i - max): a term carries e (|d_i| + 2) relative, the tree (a thread's chunks one by one, 6 shuffle levels, at
    most 15 wave totals, one addition) `depth(V, vec)` additions of e each:  zrel = e (sum_i w_i (|d_i| + 2) / Z + depth).
  * log Z^: zrel + 3 e |log Z|.  Common to the row:  E = zrel + 3 e |log Z| (+ e |max + log Z| for bf16 logits, whose kernel forms
    x - (max + log Z); tasu_logprob_topk's forms, treated as tests/decode_ref64.py treats them).
  * lp^_v: E + e |d_v| + e |lp_v|;  the penalty and the division by T one e each:  ds_v = (p_v / T) (E + e |d_v| + e |lp_v|) + 2 e |s_v|.
    E is common to a row, so two columns outside the history with different x never swap and equal x give equal s^ bit for bit: the
    top-k threshold is EXACT among them; a history column against the others is decided when they differ by more than ds + ds'
    (else the row is `ambiguous`: the test grids keep rows far from that).
  * top-p: as tests/sample_ref64.py, with the weights' argument error 2 max ds on top:  pmargin = 2 rel + 2 e, rel = e (dmax + 2 + 22)
    + 2 max ds.  A rank within pmargin of the cut may go either way (`alternatives`).
  * G^ = -logf(-logf(u)): the inner logf 2 e relative, which the outer turns into 2 e absolute, the outer 2 e |G|:  dG = 2 e (1 + |G|).
  * a^ = fl(s^ + run): ds_v + e |a|.   key^ = fl(a^ + G^):  dk_v = ds_v + e |a_v| + dG_v + e |key_v|.
Two candidates whose keys differ by less than dk + dk' may come out in either order, and the last of them may replace the first one
left out: `Row.check` accepts exactly that, and `Row.ambiguous` says whether a row has such a class (or an open filter decision)."""
import numpy as np

from row_ref64 import e
from sample_ref64 import GOLD, ODD, POOL, pool_cut

NONE = 0x7fffffff
_U64 = np.uint64


def mix64v(z):
    """splitmix64's finaliser on a uint64 array (numpy wraps modulo 2^64)."""
    z = (z ^ (z >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> _U64(27))) * _U64(0x94D049BB133111EB)
    return z ^ (z >> _U64(31))


def key_bits(seed, t, c):
    """The 23-bit integers (z >> 41) of the counters c (an integer array, 64-bit)."""
    k = _U64(int(seed) & ((1 << 64) - 1)) ^ _U64((int(t) * GOLD) & ((1 << 64) - 1))
    with np.errstate(over="ignore"):
        z = mix64v(k + np.asarray(c, dtype=np.int64).astype(_U64) * _U64(ODD))
    return (z >> _U64(41)).astype(np.int64)


def key_uniforms(seed, t, c):
    """float32 u of the counters c: (bits + 1/2) * 2^-23, exact."""
    return ((key_bits(seed, t, c).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)).astype(np.float32)


def gumbel32(seed, t, c):
    """G = -log(-log(u)) in float32 numpy (the fixture draw's and the CPU double's; the kernel's logf may differ in the last bit)."""
    u = key_uniforms(seed, t, c)
    return (-np.log(-np.log(u))).astype(np.float32)


def draw_flat(a, seed, t, K):
    """The draw on HF's accumulated scores a [B, nb * V] float32 (-inf: filtered): per utterance the K flat indices with the largest
    float32 keys a + G, in the order (key descending, flat index = (beam, token) ascending).  What stands in torch.multinomial's place."""
    a = np.asarray(a, dtype=np.float32)
    B, N = a.shape
    out = np.zeros((B, K), dtype=np.int64)
    for b in range(B):
        fin = np.flatnonzero(a[b] > -np.inf)
        assert len(fin) >= K, (len(fin), K)
        key = (a[b, fin] + gumbel32(seed, t, b * N + fin)).astype(np.float32)
        out[b] = fin[np.lexsort((fin, -key.astype(np.float64)))[:K]]
    return out


def depth(V, vec):
    """Additions on the longest chain of the kernel's row sum: a thread's columns, 6 shuffle levels, 15 wave totals, one more."""
    chunks = -(-V // vec)
    return -(-chunks // 1024) * vec + 22


class Row:
    """One row's float64 reference.  x: [V] fp32-representable logits; hist: the row's generated tokens (or None); banned: column ids
    (negative: none); run: the row's running score (fp32); m: the output row (the RNG's counter); fast: bf16 logits (the kernel's
    x - (max + log Z) form)."""

    def __init__(self, x, hist, banned, penalty, temperature, top_k, top_p, run, seed, t, m, K, fast, pool=POOL):
        x = np.asarray(x, dtype=np.float64)
        V = len(x)
        self.K, self.V = K, V
        p, T = float(np.float32(penalty)), float(np.float32(temperature))
        mx = x.max()
        d = x - mx
        w = np.exp(d)
        Z = w.sum()
        logZ = np.log(Z)
        zrel = e * (float((w * (np.abs(d) + 2)).sum() / Z) + depth(V, 8 if fast else 4))
        E = zrel + 3 * e * abs(logZ) + (e * abs(mx + logZ) if fast else 0.0)
        lp = d - logZ
        in_hist = np.zeros(V, dtype=bool)
        if hist is not None and p != 1.0:
            h = np.unique(np.asarray(hist, dtype=np.int64))
            in_hist[h[(h >= 0) & (h < V)]] = True
        pv = np.where(in_hist, p, 1.0)
        lpp = np.where(in_hist, np.where(lp < 0, lp * p, lp / p), lp)
        for b in banned:
            if 0 <= b < V:
                lpp[b] = -np.inf
        s = lpp / T
        with np.errstate(invalid="ignore"):
            ds = pv / T * (E + e * np.abs(d) + e * np.abs(lp)) + 2 * e * np.abs(s)
        ds[~np.isfinite(s)] = 0.0
        self.s, self.ds = s, ds
        # ---- top-k at max(top_k, 2): exact among the columns outside the history; a history column near the threshold opens it
        k = max(int(top_k), 2)
        self.desc = pool_cut(s, k, pool)
        self.ambiguous = False
        sel = np.flatnonzero(s > -np.inf)
        if len(self.desc) < len(sel):
            kth = s[self.desc].min()
            others = np.setdiff1d(sel, self.desc)
            nxt = others[np.argmax(s[others])]
            at = self.desc[s[self.desc] == kth]
            if (in_hist[at].any() or in_hist[nxt]) and kth - s[nxt] <= ds[at].max() + ds[nxt]:
                self.ambiguous = True
        sd = s[self.desc]
        self.dmax = float(np.abs(sd - sd[0]).max())
        rel = e * (self.dmax + 2 + 22) + 2 * float(ds[self.desc].max())
        wd = np.exp(sd - sd[0])
        n = len(sd)
        self.alternatives = [n]
        top_p32 = float(np.float32(top_p))
        if top_p32 < 1.0:
            S = np.cumsum(wd[::-1])[::-1]
            thr = 1.0 - top_p32
            ratio = S / S[0]
            rank = np.arange(n)
            gone = np.flatnonzero((ratio <= thr) & (rank >= 2))
            near = (np.abs(ratio - thr) < 2 * rel + 2 * e) & (rank >= 2)
            clear = gone[~near[gone]]
            g0 = int(clear[0]) if len(clear) else n
            self.cut = int(gone[0]) if len(gone) else n
            self.alternatives = sorted({g0} | {int(r) for r in np.flatnonzero(near) if r < g0})
        else:
            self.cut = n
        self.ambiguous = self.ambiguous or len(self.alternatives) > 1
        # ---- keys of everything that may survive
        ids = self.desc[:max(self.alternatives)]
        u = key_uniforms(seed, t, int(m) * V + ids.astype(np.int64)).astype(np.float64)
        G = -np.log(-np.log(u))
        a = s[ids] + float(run)
        key = a + G
        dk = ds[ids] + e * np.abs(a) + 2 * e * (1 + np.abs(G)) + e * np.abs(key)
        self.ids, self.a, self.key, self.dk, self.da = ids, a, key, dk, ds[ids] + e * np.abs(a)
        self.pos = {int(v): i for i, v in enumerate(ids)}
        n_sure = min(self.alternatives)
        order = np.lexsort((ids[:self.cut], -key[:self.cut]))
        self.want = ids[:self.cut][order][:K]                         # the reference's own outcome
        top = order[:K + 1]
        for i in range(len(top) - 1):
            if key[top[i]] - key[top[i + 1]] <= dk[top[i]] + dk[top[i + 1]]:
                self.ambiguous = True
        if n_sure < len(ids) and n_sure < K + 1:
            self.ambiguous = True

    def check(self, out_key, out_val, out_idx):
        """None when the kernel's K slots are a legal outcome, else a description."""
        out_key, out_val, out_idx = (np.asarray(t) for t in (out_key, out_val, out_idx))
        K = self.K
        real = out_idx != NONE
        n = int(real.sum())
        if not real[:n].all():
            return "fillers in front of candidates"
        if not (np.isneginf(out_key[n:]).all() and np.isneginf(out_val[n:]).all()):
            return "a filler slot is not (-inf, -inf, 0x7fffffff)"
        if not any(n == min(K, alt) for alt in self.alternatives):
            return f"{n} candidates, the survivors are {self.alternatives}"
        toks = [int(v) for v in out_idx[:n]]
        if len(set(toks)) != n:
            return "a token twice"
        for i, v in enumerate(toks):
            if v not in self.pos:
                return f"slot {i}: token {v} is not a survivor"
            q = self.pos[v]
            if not abs(float(out_val[i]) - self.a[q]) <= self.da[q]:
                return f"slot {i}: a = {float(out_val[i])!r} vs {self.a[q]!r}, bound {self.da[q]:.3g}"
            if not abs(float(out_key[i]) - self.key[q]) <= self.dk[q]:
                return f"slot {i}: key = {float(out_key[i])!r} vs {self.key[q]!r}, bound {self.dk[q]:.3g}"
            if i and not (out_key[i - 1] > out_key[i] or (out_key[i - 1] == out_key[i] and toks[i - 1] < v)):
                return f"slots {i - 1}, {i} are not in (key descending, id ascending) order"
        # nothing clearly better was left out: a survivor under every admissible cut that is not in the output
        if n:
            q_out = np.array([self.pos[v] for v in toks])
            worst = int(q_out[np.argmin(self.key[q_out])])
            for q in range(min(self.alternatives)):
                if int(self.ids[q]) not in toks and n == K and self.key[q] - self.key[worst] > self.dk[q] + self.dk[worst]:
                    return f"token {int(self.ids[q])} (key {self.key[q]!r}) is left out, token {int(self.ids[worst])} (key {self.key[worst]!r}) is in"
        if not self.ambiguous and toks != [int(v) for v in self.want]:
            return f"tokens {toks}, the reference's {self.want.tolist()}"
        return None


# ------------------------------------------------------------------------------------------ the row kernels' test cases
import collections  # noqa: E402

KernelCase = collections.namedtuple("KernelCase", "V M nb K first hist T top_k top_p seed t")
# V = 1000 and 151936, M in {2, 10, 64}, K in {4, 10, 32} (the kernel takes K and the beam count separately; the decode loop passes
# K = 2 nb), `first` on and off, with and without history (and ban); top_k = 1 is the max(top_k, 2) path.  Every (M, K) pair at
# V = 1000, where a reference row is cheap; the diagonal and three corners at V = 151936.  The seeds: the first from 41 on with which
# the reference alone keeps the share of ambiguous rows of every case under AMBIGUOUS_CAP for both logit types
# (tests/test_generate_beam_sample_cpu.py checks it).
KERNEL_CASES = [KernelCase(1000, 2, 2, 4, False, False, 1.0, 50, 1.0, 41, 0), KernelCase(1000, 2, 1, 10, False, True, 0.7, 50, 0.9, 41, 1),
                KernelCase(1000, 2, 2, 32, True, True, 1.5, 50, 1.0, 41, 2), KernelCase(1000, 10, 2, 4, True, False, 1.0, 8, 0.5, 41, 4),
                KernelCase(1000, 10, 5, 10, True, True, 0.7, 8, 0.9, 41, 3), KernelCase(1000, 10, 5, 32, False, False, 1.5, 50, 0.9, 41, 5),
                KernelCase(1000, 64, 2, 4, False, True, 0.7, 2, 1.0, 41, 6), KernelCase(1000, 64, 4, 10, True, False, 1.0, 50, 0.5, 41, 8),
                KernelCase(1000, 64, 16, 32, False, True, 1.5, 50, 0.5, 41, 199), KernelCase(151936, 2, 2, 4, True, False, 1.0, 1, 0.9, 41, 1),
                KernelCase(151936, 10, 5, 10, False, True, 0.7, 50, 1.0, 41, 7), KernelCase(151936, 64, 16, 32, True, False, 1.0, 50, 0.9, 41, 2),
                KernelCase(151936, 64, 2, 4, False, True, 1.0, 2, 0.5, 41, 11), KernelCase(151936, 2, 1, 32, False, True, 1.5, 50, 1.0, 41, 9),
                KernelCase(151936, 10, 2, 32, True, False, 0.7, 50, 0.9, 41, 10)]
AMBIGUOUS_CAP = 0.10
KERNEL_PENALTY = 1.3
KERNEL_SEED = -6148914691236517206                                 # the call's 64-bit seed in every case


def kernel_inputs(c):
    """Logits on a 1/8 grid (exact in bf16 and fp32; the filters are decided far above the bound): a body of N(0, 2^2) clipped to
    [-12, 6] and 64 head columns per row in [8, 16).  -> dict(x [R, V] float64 with R = M / nb logits rows when ``first`` else M,
    hist [M, 64] / hist_len [M] (lengths 0, 1, 37 by row: the row's best column; its eight best, repeats and background columns),
    banned (row 0's best column), run [M] float32 running scores in (-20, 0])."""
    g = np.random.default_rng(1000 * c.seed + c.V % 997 + c.M)
    R = c.M // c.nb if c.first else c.M
    x = np.clip(np.round(g.normal(size=(R, c.V)) * 16) / 8, -12, 6)
    for r in range(R):
        x[r, g.permutation(c.V)[:64]] = 8 + g.integers(0, 64, 64) / 8
    hist = g.integers(0, c.V, (c.M, 64)).astype(np.int32)
    hl = np.zeros(c.M, dtype=np.int32)
    for m in range(c.M):
        best = np.argsort(-x[m // c.nb if c.first else m], kind="stable")[:8].tolist()
        if m % 3 == 1:
            hist[m, 0], hl[m] = best[0], 1
        elif m % 3 == 2:
            h = (best + best[:3] + g.integers(0, c.V, 26).tolist())[:37]
            hist[m, :37], hl[m] = h, 37
    run = (-g.random(c.M) * 20).astype(np.float32)
    return dict(x=x, hist=hist, hist_len=hl, banned=int(np.argmax(x[0])), run=run)


_ROWS = {}


def kernel_rows(c, fast):
    """The case's M row references (computed once per session and shared)."""
    if (c, fast) not in _ROWS:
        d = kernel_inputs(c)
        _ROWS[c, fast] = [Row(d["x"][m // c.nb if c.first else m], d["hist"][m, :d["hist_len"][m]] if c.hist else None,
                              [d["banned"]] if c.hist else [], KERNEL_PENALTY if c.hist else 1.0, c.T, c.top_k, c.top_p, d["run"][m],
                              KERNEL_SEED, c.t, m, c.K, fast) for m in range(c.M)]
    return _ROWS[c, fast]
