"""-m "not gpu": the model of zk_powers_check (tests/powers_check_model.py) on its own -- a transcript of a known (alpha, beta, x)
passes, a contribution to it passes and is the transcript of the products, and every alteration sets exactly the bits the relations
say it must.  Python integers only."""
import pytest

import zksnark_rs_amd as zk
from zksnark_rs_amd import SplitMix64

import powers_check_model as pm

R = zk.R_MODULUS
SHAPES = [(2, 2), (3, 2), (5, 3), (9, 4), (12, 12), (40, 7)]


def drawn(seed):
    rng = SplitMix64(seed)
    return rng.fr(), rng.fr(), rng.fr(), rng.fr()


@pytest.mark.parametrize("n1,n2", SHAPES)
def test_a_transcript_of_known_scalars_passes(n1, n2):
    alpha, beta, x, c = drawn(71000 + n1)
    t = pm.exponents(alpha, beta, x, n1, n2)
    assert pm.check(t, c) == 0
    assert pm.check(t, 1) == 0 and pm.check(t, R - 1) == 0
    assert pm.check(pm.exponents(1, 1, 1, n1, n2), c) == 0              # zk_powers_initial


@pytest.mark.parametrize("n1,n2", SHAPES)
def test_a_contribution_is_the_transcript_of_the_products(n1, n2):
    alpha, beta, x, c = drawn(72000 + n1)
    s, a, b, _ = drawn(72500 + n1)
    t = pm.exponents(alpha, beta, x, n1, n2)
    u, _ = pm.contributed(t, s, a, b)
    assert u == pm.exponents(alpha * a % R, beta * b % R, x * s % R, n1, n2)
    assert pm.check(u, c) == 0
    assert pm.check_contribution(t, u, pm.record_points(t), pm.record_points(u), True, c) == 0
    assert pm.check_contribution(u, t, pm.record_points(t), pm.record_points(u), True, c) == pm.BIT["RECORD"]
    assert pm.check_contribution(t, u, pm.record_points(t), pm.record_points(u), False, c) == pm.BIT["KNOWLEDGE"]


@pytest.mark.parametrize("n1,n2", SHAPES)
def test_every_alteration_sets_exactly_its_bits(n1, n2):
    alpha, beta, x, c = drawn(73000 + n1)
    t = pm.exponents(alpha, beta, x, n1, n2)
    alts = pm.alterations(t)
    assert len(alts) >= 12
    for name, bad, bits in alts:
        assert pm.check(bad, c) == bits, (name, n1, n2)
    seen = 0
    for _, _, bits in alts:
        seen |= bits
    assert seen == sum(pm.BIT[k] for k in ("GENERATORS", "POWERS_G1", "POWERS_G2", "ALPHA", "BETA", "BETA_TWINS"))


def test_degenerate_transcripts_are_flagged_and_otherwise_consistent():
    alpha, beta, x, c = drawn(74000)
    D = pm.BIT["DEGENERATE"]
    assert pm.check(pm.exponents(alpha, beta, 0, 9, 4), c) == D           # x = 0: tau[k] = infinity for k >= 1, every relation holds
    assert pm.check(pm.exponents(0, beta, x, 9, 4), c) == D
    assert pm.check(pm.exponents(alpha, 0, x, 9, 4), c) == D
    t0 = pm.exponents(alpha, beta, 0, 9, 4)
    u, _ = pm.contributed(t0, 5, 6, 7)
    assert u["tau_g1"][1:] == [0] * 8 and pm.check(u, c) == D             # infinities pass through a contribution
