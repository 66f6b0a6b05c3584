"""-m "not gpu": the signed-digit recoding of the MSMs (csrc/msm_impl.hpp for_each_digit and digit_step_c<17 / 20>) restated in
Python, and the generator of the scalars that drive it to its edges -- the top bucket (digit +2^(c-1), the last bin and sub-bucket of
the two-level sort), the first negative digit (raw 2^(c-1) + 1, which carries), carries that run through every window, and the largest
digit a canonical scalar reaches in the top window (a carry-only or one-bit window at c = 2 and c = 11).  Random scalars hit each of
these with probability about 2^-c per window; tests/test_gpu_edges.py feeds this set to zk_msm_g1 / zk_msm_g2 and to a proof.

The self-check below asserts that the generated set really reaches every case for every window size the library accepts, so a
generator that drifts fails here instead of silently testing nothing; and that the set catches plausible slips of the recoding."""
import numpy as np
import pytest

from zksnark_rs_amd import R_MODULUS as R

WINDOW_SIZES = range(2, 23)          # msm_impl.hpp: window_bits in [2, 22]


def windows(c):
    return 254 // c + 1


def recode(k, c, nwin=None, neg_test=None, carry_on_zero=True, word_bits=False):
    """for_each_digit restated: window w takes bits [c w, c w + c) plus the carry of window w - 1 (raw); raw > 2^(c-1) becomes the
    negative digit raw - 2^c and carries 1.  Returns (raw, digit) per window and the carry left after the last window.
    The keyword arguments are the slips the mutation check below plants (the default is the library's recoding)."""
    mask, half = (1 << c) - 1, 1 << (c - 1)
    carry, out = 0, []
    for w in range(windows(c) if nwin is None else nwin):
        if word_bits:                       # bits read from one 32-bit word only (no funnel shift across words)
            bit = c * w
            bits = ((k >> (bit & ~31)) & 0xFFFFFFFF) >> (bit & 31) & mask
        else:
            bits = (k >> (c * w)) & mask
        raw = bits + carry
        neg = raw > half if neg_test is None else neg_test(raw, half)
        mag = (1 << c) - raw if neg else raw
        carry = int(neg) if carry_on_zero or mag else 0
        out.append((raw, -mag if neg else mag))
    return out, carry


def rebuild(digits, c):
    return sum(d << (c * w) for w, (_, d) in enumerate(digits))


def _ones(c, j):
    """windows 0 .. j all ones (each carries out); 0 for j < 0"""
    return (1 << (c * (j + 1))) - 1 if j >= 0 else 0


def _chain(c, j):
    """the smallest value that carries out of window j: digit 2^(c-1) + 1 in window 0, 2^(c-1) (+ the carry) in windows 1 .. j"""
    half = 1 << (c - 1)
    return sum(half << (c * i) for i in range(j + 1)) + 1 if j >= 0 else None


def min_scalar_with_raw(c, w, v):
    """the smallest scalar whose window w sees raw = v: bits v and no carry, or bits v - 1 and the smallest carry out of window w - 1"""
    mask = (1 << c) - 1
    cands = []
    if v <= mask:
        cands.append(v << (c * w))
    if 1 <= v <= mask + 1 and w >= 1:
        cands.append(((v - 1) << (c * w)) + _chain(c, w - 1))
    return min(cands) if cands else None


def reachable_windows(c, v):
    """windows in which some canonical scalar (< r) has raw = v"""
    return {w for w in range(windows(c)) if (m := min_scalar_with_raw(c, w, v)) is not None and m < R}


def top_raw_max(c):
    """the largest raw a canonical scalar reaches in the top window: r's top bits, plus 1 if the rest of r leaves room for a carry"""
    wt = windows(c) - 1
    top = (R - 1) >> (c * wt)
    return top + 1 if _chain(c, wt - 1) < R - (top << (c * wt)) else top


def recoding_cases(c):
    """canonical scalars that together give, for window size c:
      (a) digit +2^(c-1) in every window that can hold it;   (b) raw 2^(c-1) + 1 (negative digit, carry) in every window;
      (c) carries from window 0 through every window up to the top;   (d) the largest top-window raw a canonical scalar reaches;
      (e) 0, 1, 2, r - 1, r - 2, r - 2^k, 2^k, (r - 1) / 2."""
    half, wt = 1 << (c - 1), windows(c) - 1
    ks = []

    def add(k):
        if k is not None and 0 <= k < R and k not in ks:
            ks.append(k)
            return True
        return False

    for w in range(wt + 1):
        # (a) bits 2^(c-1), or bits 2^(c-1) - 1 under a carry out of the all-ones windows below
        if not add(half << (c * w)) and w:
            add(((half - 1) << (c * w)) + _ones(c, w - 1)) or add(((half - 1) << (c * w)) + _chain(c, w - 1))
        # (b) bits 2^(c-1) + 1, or 2^(c-1) under a carry
        if not add((half + 1) << (c * w)) and w:
            add((half << (c * w)) + _ones(c, w - 1)) or add((half << (c * w)) + _chain(c, w - 1))
    # (b) raw 2^(c-1) + 1 in every window at once, as far up as a canonical scalar goes
    for j in range(wt, -1, -1):
        if add(_chain(c, j)):
            break
    # (c) all-ones low windows of every length (each window carries into the next), with the window above them at 0, 2^(c-1) - 1 and
    # 2^(c-1) (raw 2^(c-1) and 2^(c-1) + 1 there); and the smallest chain into the top window where all-ones does not fit below r
    for j in range(wt):
        for above in (0, half - 1, half):
            add(_ones(c, j) + (above << (c * (j + 1))))
    add(_chain(c, wt - 1))
    # (d) the top window at its largest raw: r's top bits and a carry from below where r leaves room for one
    top = (R - 1) >> (c * wt)
    for low in (_ones(c, wt - 1), _chain(c, wt - 1), 0):
        add((top << (c * wt)) + low)
    add(((top - 1) << (c * wt)) + _ones(c, wt - 1) if top else None)
    # (e)
    for k in (0, 1, 2, R - 1, R - 2, (R - 1) // 2) + tuple(1 << e for e in (1, 31, 32, 63, 64, 127, 128, 200, 252, 253)) \
            + tuple(R - (1 << e) for e in (0, 1, 32, 64, 128, 200, 252)):
        add(k)
    return ks


def coverage(c, ks):
    """what the set reaches: windows with digit +2^(c-1), windows with raw 2^(c-1) + 1, scalars whose carry runs from window 0 into the
    top window, scalars at the top window's largest raw"""
    half, wt, tmax = 1 << (c - 1), windows(c) - 1, top_raw_max(c)
    a, b, chain, top = set(), set(), 0, 0
    for k in ks:
        digits, _ = recode(k, c)
        a |= {w for w, (raw, d) in enumerate(digits) if d == half}
        b |= {w for w, (raw, d) in enumerate(digits) if raw == half + 1}
        chain += all(d < 0 or raw == 1 << c for raw, d in digits[:wt])   # every window below the top carried
        top += digits[wt][0] == tmax
    return a, b, chain, top


def _check(k, c, digits, carry):
    half = 1 << (c - 1)
    return carry == 0 and rebuild(digits, c) == k and all(-half <= d <= half for _, d in digits) and digits[-1][1] >= 0


def test_recoding_rebuilds_every_scalar():
    """for every c in 2..22: the digits rebuild the scalar, lie in [-2^(c-1), 2^(c-1)] (bucket |digit| - 1 < 2^(c-1)), the top digit
    is never negative and no carry is left after the last window -- on the edge set and on 10^4 random canonical scalars"""
    rng = np.random.default_rng(254)
    rand = [int.from_bytes(rng.bytes(32), "little") % R for _ in range(10000)]
    for c in WINDOW_SIZES:
        tmax = top_raw_max(c)
        for k in recoding_cases(c) + rand:
            digits, carry = recode(k, c)
            assert _check(k, c, digits, carry), (c, k)
            assert digits[-1][0] <= tmax, (c, k)          # nothing canonical goes past the computed top


def test_recoding_cases_cover_every_edge(capsys):
    """the generator reaches (a)-(d) for every window size: (a) and (b) in exactly the windows where a canonical scalar can have them
    (computed from r, not listed), (c) and (d) at least once"""
    rows = []
    for c in WINDOW_SIZES:
        ks = recoding_cases(c)
        assert all(0 <= k < R for k in ks) and len(set(ks)) == len(ks)
        a, b, chain, top = coverage(c, ks)
        want_a, want_b = reachable_windows(c, 1 << (c - 1)), reachable_windows(c, (1 << (c - 1)) + 1)
        rows.append("c=%2d windows=%3d  (a) %3d/%3d  (b) %3d/%3d  (c) %3d  (d) %d at raw %d  scalars %d"
                    % (c, windows(c), len(a), len(want_a), len(b), len(want_b), chain, top, top_raw_max(c), len(ks)))
        assert a == want_a and b == want_b, rows[-1]
        assert len(a) and len(b) and chain and top, rows[-1]
        # every window below the top can hold both; the top window holds neither (r < 2^254)
        assert want_a == want_b == set(range(windows(c) - 1)), rows[-1]
    with capsys.disabled():
        print("\n" + "\n".join(rows))


def test_top_window_examples():
    """the windows the issue names: at c = 2 the top window has no scalar bits (a carry is its only digit), at c = 11 it has one"""
    assert 2 * (windows(2) - 1) == 254 and top_raw_max(2) == 1
    assert 11 * (windows(11) - 1) == 253 and top_raw_max(11) == 2
    for c in (2, 11):
        assert any(recode(k, c)[0][-1][0] == top_raw_max(c) for k in recoding_cases(c))


MUTANTS = {
    "sign test one late (raw > 2^(c-1) + 1)": dict(neg_test=lambda raw, half: raw > half + 1),
    "top window dropped": dict(nwin="short"),
    "no carry when the magnitude is 0 (raw = 2^c)": dict(carry_on_zero=False),
    "bits from one 32-bit word only": dict(word_bits=True),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_edge_set_catches_recoding_slips(name):
    """each slip of the recoding is caught by the edge set alone at every c where it changes anything (the word-boundary slip only
    where a window straddles two 32-bit words: c does not divide 32)"""
    kw = dict(MUTANTS[name])
    for c in WINDOW_SIZES:
        if kw.get("word_bits") and 32 % c == 0:
            continue
        if kw.get("nwin") == "short" or name.startswith("top"):
            kw["nwin"] = windows(c) - 1
        caught = [k for k in recoding_cases(c) if not _check(k, c, *recode(k, c, **kw))]
        assert caught, (name, c)
