"""TEST HELPER (not a test, never shipped): generate(do_sample=True, num_beams=1) restated -- the counter-based uniforms in integer
numpy, the scores s in numpy float32 (the operations are IEEE: the kernel's bits), filter and draw in float64, and the bound the
sampler kernels (csrc/sample.hip) are held to.  Nothing is shared with the kernels or with tests/sample_ops.py.

THE RNG.  u(seed, t, r) = float(mix64((seed ^ t * GOLD) + r * ODD) >> 40) * 2^-24, everything modulo 2^64, mix64 the splitmix64
finaliser (the dropout masks' of csrc/lora.hip).

THE DISTRIBUTION (HF's order: repetition penalty, EOS ban, temperature, top-k, top-p), per row on the fp32 logits x:
  x' = x < 0 ? x * p : x / p on the distinct history tokens;  banned columns -inf;  s = x' / T (fp32, -0 -> +0);
  top-k keeps s >= the k-th largest s (ties kept; more than `pool` survivors: the ones above the threshold and the first ties by id);
  top-p: w = exp(s - max), entries in descending (s, then ascending id) order, S_r = sum_{q >= r} w_q; the first r >= 1 with
  S_r <= (1 - top_p) S_0 and everything behind it go.
THE DRAW.  Survivors in ascending id order, C_i = sum_{j <= i} w_j, Z = C_last: the smallest i with C_i > u Z.

THE BOUND.  e = 2^-24 is fp32's unit roundoff (tests/row_ref64.py, whose constants these are: an fp32 +, *, /: e relative; expf, the
correctly reduced library function: 1 ulp = 2 e, its rounded argument d = s - max turning e |d| absolute into as much relative).
  * s is reproduced exactly (one fp32 product or quotient, one fp32 quotient), so the top-k survivors are EXACT: no margin class.
  * a kernel weight w^_j = w_j (1 + th_j), |th_j| <= e (|d_j| + 2) <= e (dmax + 2), dmax the largest |d| among the survivors.
  * every sum of the kernel is a fixed tree: 6 shuffle levels in a wave, at most 15 wave totals added one by one, one addition of the
    two: DEPTH = 22 additions on the longest chain, so C^_i = C_i (1 + g), |g| <= e (dmax + 2 + DEPTH) =: rel, to first order.
  * the pick: C^_{i-1} <= fl(u Z^) < C^_i with fl(u Z^) = u Z (1 + g') (1 + e').  So
        C_{i-1} - delta <= u Z <= C_i + delta,   delta = Z (2 rel + 2 e)        (the C's and u Z are all <= Z)
  * top-p compares S^_r <= fl((1 - top_p) S^_0), both sums carrying rel, the product and the fp32 (1 - top_p) an e each: a row whose
    |S_r / S_0 - (1 - top_p)| is below  pmargin = 2 rel + 2 e  for some r >= 1 may be cut at r or behind it (`alternatives`).
  * the log-probability (s - max) - logf(Z^): rel + 2 e |log Z| (logf, 1 ulp) + e |d| + e |lp| (the two subtractions).
`pool_cut` is the documented departure from HF (which keeps every tie) and is exact too."""
import numpy as np

from row_ref64 import e

M64 = (1 << 64) - 1
GOLD, ODD = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03
DEPTH = 22
POOL = 1024


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def uniforms(seed, t, M):
    """float32 [M]: the uniforms of generated position t (python integers, modulo 2^64)."""
    key = (int(seed) & M64) ^ ((int(t) * GOLD) & M64)
    return np.array([(mix64((key + r * ODD) & M64) >> 40) * 2.0 ** -24 for r in range(M)], dtype=np.float32)


def scores32(x, hist, banned, penalty, temperature):
    """s [R, V] float32 with the kernel's bits.  x: [R, V] array of fp32-representable logits; hist: per row a list of generated
    tokens (or None); banned: list of column ids (negative: none)."""
    s = np.array(x, dtype=np.float32)
    p, T = np.float32(penalty), np.float32(temperature)
    if hist is not None and float(penalty) != 1.0:
        for r, h in enumerate(hist):
            h = np.unique(np.asarray(h, dtype=np.int64))
            h = h[(h >= 0) & (h < s.shape[1])]
            v = s[r, h]
            s[r, h] = np.where(v < 0, v * p, v / p)
    for b in banned:
        if 0 <= b < s.shape[1]:
            s[:, b] = -np.inf
    s = s / T
    s[s == 0] = 0.0
    return s


def pool_cut(s, top_k, pool=POOL):
    """Step 4 on one row of scores: ids of the survivors, descending (s, then ascending id)."""
    sel = np.flatnonzero(s > -np.inf)
    k = min(int(top_k), len(sel))
    kth = np.partition(s[sel], len(sel) - k)[len(sel) - k]        # the k-th largest
    sel = sel[s[sel] >= kth]
    order = sel[np.lexsort((sel, -s[sel].astype(np.float64)))]
    return order[:pool]


class Row:
    """One row's float64 reference: ids (descending order) after top-k, weights, the top-p cut and its ambiguity, the bound's terms."""

    def __init__(self, s, top_k, top_p, pool=POOL):
        self.desc = pool_cut(s, top_k, pool)
        sd = s[self.desc].astype(np.float64)
        self.smax = sd[0]
        self.dmax = float(np.abs(sd - sd[0]).max())
        self.rel = e * (self.dmax + 2 + DEPTH)
        w = np.exp(sd - sd[0])
        self.w_desc, self.s_desc = w, sd
        n = len(sd)
        self.cut, self.alternatives = n, [n]
        top_p32 = float(np.float32(top_p))
        if top_p32 < 1.0:
            S = np.cumsum(w[::-1])[::-1]
            thr = 1.0 - top_p32
            ratio = S / S[0]
            gone = np.flatnonzero((ratio <= thr) & (np.arange(n) >= 1))
            self.cut = int(gone[0]) if len(gone) else n
            pmargin = 2 * self.rel + 2 * e
            near = (np.abs(ratio - thr) < pmargin) & (np.arange(n) >= 1)
            # a near rank may decide either way; the others decide as here: the cut is the first rank that is clearly gone, or a
            # near rank in front of it
            clear = gone[~near[gone]]
            g0 = int(clear[0]) if len(clear) else n
            self.alternatives = sorted({g0} | {int(r) for r in np.flatnonzero(near) if r < g0})
        self.ambiguous = len(self.alternatives) > 1

    def check(self, token, u, logprob=None):
        """None when (token, logprob) is a legal outcome for uniform u under one of the admissible cuts, else a description."""
        why = []
        for cut in self.alternatives:
            ids, w, sd = self.desc[:cut], self.w_desc[:cut], self.s_desc[:cut]
            o = np.argsort(ids)
            ids, w, sd = ids[o], w[o], sd[o]
            C = np.cumsum(w)
            Z = C[-1]
            hit = np.flatnonzero(ids == token)
            if len(hit) == 0:
                why.append(f"cut {cut}: token {token} is not a survivor")
                continue
            i = int(hit[0])
            delta = Z * (2 * self.rel + 2 * e)
            lo, hi = (C[i - 1] if i else 0.0) - delta, C[i] + delta
            uz = float(u) * Z
            if not lo <= uz <= hi:
                why.append(f"cut {cut}: u Z = {uz!r} outside [{lo!r}, {hi!r}] of token {token} (delta {delta:.3g})")
                continue
            if logprob is not None:
                lp = (sd[i] - self.smax) - np.log(Z)
                bound = self.rel + 2 * e * abs(np.log(Z)) + e * abs(sd[i] - self.smax) + e * abs(lp)
                if not abs(float(logprob) - lp) <= bound:
                    why.append(f"cut {cut}: log-prob {float(logprob)!r} vs {lp!r}, bound {bound:.3g}")
                    continue
            return None
        return "; ".join(why)

    def survivors(self):
        return np.sort(self.desc[:self.cut])

    def draw(self, u):
        """The reference's own token for uniform u."""
        ids = self.desc[:self.cut]
        o = np.argsort(ids)
        C = np.cumsum(self.w_desc[:self.cut][o])
        i = np.flatnonzero(C > float(u) * C[-1])
        return int(ids[o][i[0] if len(i) else -1])


def inverse_cdf(probs, u):
    """The draw on a row of probabilities (zeros for filtered tokens), the form the fixture generator puts in torch.multinomial's
    place: float64 prefix sums in token-id order, the smallest i with C_i > u Z."""
    p = np.asarray(probs, dtype=np.float64)
    C = np.cumsum(p)
    i = np.flatnonzero((C > float(u) * C[-1]) & (p > 0))
    return int(i[0]) if len(i) else int(np.flatnonzero(p > 0)[-1])
