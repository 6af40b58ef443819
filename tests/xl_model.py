"""A plain restatement of what csrc/ks_k_apply_xl.h promises (its header comment), in NumPy and Python only — no library of this
project is loaded here.  tests/xl_case.py uses it to prove, independently of the kernel, that a hand-built input contains the edge
it is named after, and to predict the path a UNIFORM run takes (every update of a chain carries the same increment: the result and
the classification of the chunks do not depend on the integration order).

The chain of one voxel: 21 class sums p_c <- fl(p_c + x_c,i) (f32, in order) and the weight w <- min(max_weight, fl(w + uw_i)).
The documented shortcut: a chunk of 256 updates collapses into integer sums (fl(p + x) = -(M + R) u inside one binade) if, for
every one of the 22 chains,
  * the chain stays strictly inside the binade it starts the chunk in,
  * that binade is one of the eight counted from the binade the RUN started in,
  * no increment of the chunk is a rounding tie there (|x| / u has the fractional part exactly 0.5),
  * no class increment is positive (no weight increment negative),
  * every increment is below 2^22 spacings (of the binade the run starts in: the finest of the eight),
  * the weight is at max_weight already, or ends the chunk below it.
Any other chunk is replayed update by update; a run with more than n_chunks / 8 + 8 replays is handed back to the serial kernel
with its record untouched (the replay that exceeds the budget is counted, the ones after it never happen)."""
import math

import numpy as np

F = np.float32
NUM_LABELS = 21
CHAINS = NUM_LABELS + 1        # chain 21: the weight
CHUNK = 256
BINADES = 8
LONG_RUN = 1024                # runs of MORE than this many updates are listed
EPS = F(1e-6)                  # Voxblox's kFloatEpsilon
PRIOR_INIT = F(-0.60205999132)


def bits(x):
    return int(np.asarray(x, F).reshape(1).view(np.uint32)[0])


def from_bits(b):
    return np.array([b], np.uint32).view(F)[0]


def exponent(x):
    """Biased exponent field."""
    return (bits(x) >> 23) & 0xFF


def mantissa(x):
    """The integer M of a normal |x| = M * 2^(e - 150), 2^23 <= M < 2^24."""
    return (bits(x) & 0x7FFFFF) | 0x800000


def spacing_exp(e_biased):
    """log2 of the spacing of the binade with that biased exponent."""
    return e_biased - 150


def units(x, e_biased):
    """|x| in spacings of that binade, exactly (a double holds a 24-bit significand times a power of two)."""
    return math.ldexp(abs(float(x)), -spacing_exp(e_biased))


def is_tie(x, e_biased):
    t = units(x, e_biased)
    return t - math.floor(t) == 0.5


def trailing_zeros(x):
    m = mantissa(x)
    return (m & -m).bit_length() - 1


def tie_binade(x):
    """The biased exponent of the one binade in which the f32 increment x (normal, non-zero) is a tie: with exponent e and tz
    trailing zero mantissa bits, x = m 2^(e - 23) and x / u = m 2^(e - E) has its lowest set bit at 2^-1 iff E = e + 1 + tz."""
    e = exponent(x)
    assert 1 <= e <= 254 and float(x) != 0.0
    E = e + 1 + trailing_zeros(x)
    assert is_tie(x, E) and not is_tie(x, E - 1) and not is_tie(x, E + 1)
    return E


# ---- the chains, update by update ---------------------------------------------------------------------------------------------
def serial_chain(p0, increments):
    """f32 additions in order.  p0: scalar or (k,), increments: (n,) or (k, n).  Returns the value after every update: (..., n + 1)
    with the start in front."""
    inc = np.asarray(increments, F)
    p = np.asarray(p0, F).copy()
    out = np.empty(p.shape + (inc.shape[-1] + 1,), F)
    out[..., 0] = p
    for i in range(inc.shape[-1]):
        p = (p + inc[..., i]).astype(F)
        out[..., i + 1] = p
    return out


def serial_weight(w0, uws, max_weight):
    """The reference's rule: w = min(max_w, w + uw) (a sum below kFloatEpsilon leaves the voxel alone)."""
    w, mw = F(w0), F(max_weight)
    out = np.empty(len(uws) + 1, F)
    out[0] = w
    for i, uw in enumerate(np.asarray(uws, F)):
        nw = F(w + uw)
        if not nw < EPS:
            w = min(mw, nw)
        out[i + 1] = w
    return out


def integer_sum(p0, increments):
    """The shortcut's formula for one chain inside one binade: sign * (M + sum of R_i) * u, R_i = |x_i| / u rounded to the nearest
    integer (ties to even: Python's round on an exact double)."""
    e = exponent(p0)
    total = mantissa(p0) + sum(round(units(x, e)) for x in np.asarray(increments, F))
    assert total < 1 << 24
    v = F(math.ldexp(float(total), spacing_exp(e)))
    return -v if float(p0) < 0 else v


# ---- the classification of a run ------------------------------------------------------------------------------------------------
class Run:
    """What classify() found: per chunk `ok` and the reasons of the others, the replays, the budget, the end state."""

    def __init__(self):
        self.n = self.n_chunks = self.replays_needed = self.budget = 0
        self.ok, self.reasons, self.binade_index, self.tie_chunks, self.ambiguous = [], [], [], [], []
        self.end = None

    @property
    def handed_back(self):
        return self.replays_needed > self.budget

    @property
    def replayed(self):
        """What the walk counts: every replay, the one that exceeds the budget included."""
        return min(self.replays_needed, self.budget + 1)

    @property
    def binades_spanned(self):
        """Binades a chain is in over the run, the starting one included, the most of any chain."""
        return self._span

    def summary(self):
        return dict(n=self.n, chunks=self.n_chunks, replays_needed=self.replays_needed, budget=self.budget, handed_back=self.handed_back,
                    binades_spanned=self.binades_spanned, tie_chunks=len(self.tie_chunks),
                    reasons=sorted({r for rs in self.reasons for r in rs}))


def classify(p0, increments, max_weight, active=None):
    """p0: the 22 start values (21 class sums, the weight).  increments: (22, n) per-update increments (row 21: the update weights).
    active: (n,) bool, False where an update carries no semantic update at all (its class increments are skipped).  Says for
    every chunk of 256 updates whether the documented rule can carry it."""
    p0 = np.asarray(p0, F)
    inc = np.asarray(increments, F)
    assert p0.shape == (CHAINS,) and inc.shape[0] == CHAINS
    n = inc.shape[1]
    act = np.ones(n, bool) if active is None else np.asarray(active, bool)
    mw = F(max_weight)
    cls = serial_chain(p0[:NUM_LABELS], np.where(act[None, :], inc[:NUM_LABELS], F(0)))
    wts = serial_weight(p0[NUM_LABELS], inc[NUM_LABELS], mw)
    states = np.concatenate([cls, wts[None, :]], axis=0)          # (22, n + 1)
    e0 = [exponent(v) for v in p0]
    R = Run()
    R.n, R.n_chunks = n, (n + CHUNK - 1) // CHUNK
    R.budget = R.n_chunks // 8 + 8
    R.end = states[:, -1].copy()
    span = 1
    for b in range(R.n_chunks):
        lo, hi = b * CHUNK, min(n, (b + 1) * CHUNK)
        why, k_of, tied, amb = set(), [], False, False
        for c in range(CHAINS):
            is_w = c == NUM_LABELS
            start = states[c, lo]
            if is_w and start == mw:
                k_of.append(exponent(start) - e0[c])
                continue                                              # at the clamp it stays: every update weight is >= 0 (checked below)
            e = exponent(start)
            k_of.append(e - e0[c])
            xs = inc[c, lo:hi] if is_w else inc[c, lo:hi][act[lo:hi]]
            if not is_w and (float(start) >= 0 or not 1 <= e <= 253 or not np.isfinite(start)):
                why.add("state")
            if any(exponent(v) != e for v in states[c, lo + 1:hi + 1]):
                why.add("leaves_binade")
            elif mantissa(states[c, hi]) == 0xFFFFFF:
                amb = True                                            # the last value of the binade: "strictly inside" could be read either way
            if not 0 <= e - e0[c] < BINADES:
                why.add("beyond_eight_binades")
            if any(is_tie(x, e) for x in xs):
                why.add("tie")
                tied = True
            if (not is_w and (xs > 0).any()) or (is_w and (xs < 0).any()):
                why.add("sign")
            if any(units(x, e0[c]) >= 1 << 22 for x in xs) or not np.isfinite(xs).all():
                why.add("increment_too_large")
            if is_w:
                unclamped = start
                for x in xs:
                    unclamped = F(unclamped + x)
                if not unclamped < mw:
                    why.add("weight_meets_clamp")
        if (inc[NUM_LABELS, lo:hi] < 0).any():
            why.add("sign")                                           # (also where the weight sits at the clamp)
        R.ok.append(not why)
        R.reasons.append(sorted(why))
        R.binade_index.append(k_of)
        R.ambiguous.append(amb)
        if tied:
            R.tie_chunks.append(b)
    for c in range(CHAINS):
        es = {exponent(v) for v in states[c]}
        span = max(span, max(es) - min(es) + 1)
    R._span = span
    R.replays_needed = sum(not ok for ok in R.ok)
    R.states = states
    return R


# ---- the state a run starts from (k_xl_measure's rule) --------------------------------------------------------------------------
def accepts(rec, color_mode, truncation, max_weight):
    """rec: dict(distance, weight, priors[21]).  All of: not colour-blend mode; distance == truncation; kEps <= w <= max_weight <
    1e30; every class sum negative, normal, biased exponent <= 253."""
    w, mw = F(rec["weight"]), F(max_weight)
    if int(color_mode) == 0:
        return False
    if not F(rec["distance"]) == F(truncation):
        return False
    if not (w >= EPS and w <= mw and mw < F(1e30)):
        return False
    for p in np.asarray(rec["priors"], F):
        b = bits(p)
        if not (b >> 31 == 1 and 1 <= ((b >> 23) & 0xFF) <= 253):
            return False
    return True


def saturating(sdf, truncation):
    """An update with a positive weight leaves a distance that sits at +truncation there iff its own clamped distance is the
    truncation: sdf >= truncation (a weighted mean of the two).  The cases stay far from the boundary on purpose: anything
    between truncation and twice that is refused here instead of judged."""
    assert not (float(truncation) <= float(sdf) < 2 * float(truncation)), sdf
    return float(sdf) >= 2 * float(truncation)


def predict(rec, increments, sdfs, color_mode, truncation, max_weight, active=None):
    """The path of ONE run of a uniform case, as deltas of (walked, serial, chunks, replayed), and the classification (or None)."""
    n = np.asarray(increments).shape[1]
    zero = dict(walked=0, serial=0, chunks=0, replayed=0)
    if n <= LONG_RUN:
        return zero, None                                            # not listed
    if not accepts(rec, color_mode, truncation, max_weight):
        return dict(zero, serial=1), None                            # refused at measure
    if not all(saturating(s, truncation) for s in sdfs):
        return dict(zero, serial=1), None                            # some update moves the distance off the clamp: no walk
    p0 = np.concatenate([np.asarray(rec["priors"], F), [F(rec["weight"])]])
    R = classify(p0, increments, max_weight, active)
    assert not any(R.ambiguous), "a chunk ends on the last value of its binade: choose another input"
    if R.handed_back:
        return dict(walked=0, serial=1, chunks=R.n_chunks, replayed=R.replayed), R
    return dict(walked=1, serial=0, chunks=R.n_chunks, replayed=R.replayed), R


# ---- search helpers ------------------------------------------------------------------------------------------------------------
def search_probability(log_non_match, tie_in_binade, lo=0.55, hi=0.95, limit=200000):
    """The first f32 probability p in [lo, hi) whose log(1 - p) — as `log_non_match(p)` computes it: the caller passes the
    oracle's, NumPy's logarithm only proposes candidates — is a tie exactly in the binade with biased exponent `tie_in_binade`.
    Returns (p, x = log(1 - p))."""
    p = F(lo)
    for _ in range(limit):
        if not p < F(hi):
            break
        guess = np.log(F(1) - p, dtype=F)
        if float(guess) != 0.0 and exponent(guess) + 1 + trailing_zeros(guess) == tie_in_binade:
            x = F(log_non_match(p))
            if tie_binade(x) == tie_in_binade:
                return p, x
        p = np.nextafter(p, F(1))
    raise AssertionError("no probability found")


def binade_of_magnitude(v):
    """Biased exponent of the binade that holds |v|."""
    return exponent(F(abs(v)))
