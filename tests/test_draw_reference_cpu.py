"""Without a GPU: the float64 contract of tests/_draw_reference.py (its docstring derives delta) holds for oracle/draw.py on every
family and parameter set tests/test_gpu_draw_kernel.py launches, the share of ambiguous draws stays under its cap, and the contract
bites: eight float32 draws with one change each leave it."""
import numpy as np
import pytest

import _draw_reference as dr
from oracle import draw as odraw

SEED, STREAM = 0x5EED0123456789, 3


def _ids(n, P=2, base=1000):
    return base + np.arange(n) // P, np.arange(n) % P


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10, through this module's own generator, and agreement with the oracle's."""
    w = dr.philox4x32_10([np.array([0]), np.array([0]), np.array([0]), np.array([0])], (0, 0))
    assert [int(x[0]) for x in w] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = np.array([0xffffffff])
    w = dr.philox4x32_10([f, f, f, f], (0xffffffff, 0xffffffff))
    assert [int(x[0]) for x in w] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    w = dr.philox4x32_10([np.array([0x243f6a88]), np.array([0x85a308d3]), np.array([0x13198a2e]), np.array([0x03707344])],
                         (0xa4093822, 0x299f31d0))
    assert [int(x[0]) for x in w] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    rng = np.random.default_rng(0)
    c = [rng.integers(0, 2**32, 500) for _ in range(4)]
    mine = dr.philox4x32_10(c, (123456789, 987654321))
    theirs = odraw.philox4x32_10(c[0], c[1], c[2], c[3], 123456789, 987654321)
    assert all((a == b).all() for a, b in zip(mine, theirs))


def test_polynomial_error():
    """Step 4 of the derivation: pg_exp's polynomial against 2^f in exact arithmetic."""
    f = np.linspace(0.0, 1.0, 2**20 + 1)
    p = np.full_like(f, float(odraw.EXP2_COEF[6]))
    for c in odraw.EXP2_COEF[5::-1]:
        p = p * f + float(c)
    worst = np.abs(p / np.exp2(f) - 1).max() / dr.V24
    print("polynomial: %.3f x 2^-24" % worst)
    assert worst <= 0.3


def test_delta_is_the_stated_figure_and_covers_the_derivation():
    for k in range(1, 33):
        assert dr.delta(k) == (2 * k + 16) * 2.0 ** -24
        assert ((k - 1) * (1 + 2.23 / np.e) + 1 + 3.15) * 2.0 ** -24 < dr.delta(k)


def test_unmutated_restatement_is_the_oracle():
    for nv in (1, 5, 32):
        valid = dr.valid_list(nv, 33, "shuffled")
        rows = dr.stacked_rows(nv, valid, 33, seed=1)
        rid, slot = _ids(len(rows))
        for top_k, sample, temp in ((0, False, None), (3, False, 0.7), (3, True, 7.5)):
            a = (rows, valid, top_k, sample, temp, rid, 4, slot, STREAM, SEED)
            assert (dr.draw32(*a) == odraw.draw_rows(*a)).all()


@pytest.mark.parametrize("nv", dr.N_VALID)
def test_oracle_meets_the_contract_on_the_lane_cases(nv):
    n_draws = 0
    for V, order, top_k, temp in dr.lane_cases(nv):
        valid = dr.valid_list(nv, V, order)
        rows = dr.stacked_rows(nv, valid, V, seed=1)
        rid, slot = _ids(len(rows))
        for it, sample in ((0, True), (1, False)):
            a = (rows, valid, top_k, sample, temp, rid, 10 + it, slot, STREAM, SEED)
            wrong, _ = dr.contract(dr.exact_draw(*a), odraw.draw_rows(*a))
            assert len(wrong) == 0, (V, order, top_k, temp, sample, wrong)
            n_draws += len(rows)
    print("n_valid %d: %d draws" % (nv, n_draws))


@pytest.mark.parametrize("family", dr.FAMILIES)
def test_ambiguous_share_is_under_the_cap(family):
    """20 000 draws of one repeated row per case: no unambiguous draw off the reference, ambiguous share <= 1e-3."""
    for nv, V, top_k, temp in dr.SHARE_CASES:
        valid, row = dr.share_rows(family, nv, V)
        rows = np.repeat(row, dr.SHARE_DRAWS, axis=0)
        rid, slot = _ids(dr.SHARE_DRAWS, P=5)
        a = (rows, valid, top_k, False, temp, rid, 10, slot, STREAM, SEED)
        ex = dr.exact_draw(*a)
        wrong, share = dr.contract(ex, odraw.draw_rows(*a))
        differ = int((odraw.draw_rows(*a) != ex.pick).sum())
        print("%s n_valid %d V %d top_k %d temperature %s: k %d, ambiguous share %.2e (2 delta (k-1) = %.2e), %d draws off the exact pick"
              % (family, nv, V, top_k, temp, ex.k, share, 2 * dr.delta(ex.k) * (ex.k - 1), differ))
        assert len(wrong) == 0
        assert share <= dr.SHARE_CAP


def _mutation_cases():
    """Listed cases: lane cases of n_valid 20 and 32 at V = 33 (all families stacked), enough for every mutation."""
    for nv in (20, 32):
        for V, order, top_k, temp in dr.lane_cases(nv):
            if V != 33 or order != "shuffled":
                continue
            valid = dr.valid_list(nv, V, order)
            rows = np.repeat(dr.stacked_rows(nv, valid, V, seed=1), 8, axis=0)
            rid, slot = _ids(len(rows), P=3)
            for it, sample in ((0, True), (1, False)):
                yield (rows, valid, top_k, sample, temp, rid, 10 + it, slot, STREAM, SEED)


def _share_cases_at_32():
    """Listed cases again: the share-cap case with all 32 lanes live, every family, 20 000 draws each."""
    nv, V, top_k, temp = dr.SHARE_CASES[0]
    for family in dr.FAMILIES:
        valid, row = dr.share_rows(family, nv, V)
        rid, slot = _ids(dr.SHARE_DRAWS, P=5)
        yield (np.repeat(row, dr.SHARE_DRAWS, axis=0), valid, top_k, False, temp, rid, 10, slot, STREAM, SEED)


@pytest.mark.parametrize("mutation", dr.MUTATIONS)
def test_the_contract_bites(mutation):
    off_contract = off_oracle = n = 0
    for a in _mutation_cases():
        got = dr.draw32(*a, mutate=mutation)
        off_contract += len(dr.contract(dr.exact_draw(*a), got)[0]) > 0
        off_oracle += bool((got != odraw.draw_rows(*a)).any())
        n += 1
    print("%s: leaves the float64 contract on %d of %d cases, bit-equality with the oracle on %d" % (mutation, off_contract, n, off_oracle))
    assert off_contract > 0


def test_a_change_of_rounding_alone_stays_inside_the_contract():
    """The same terms summed from the other end: what delta is there to allow (see ROUNDING_ONLY in _draw_reference.py)"""
    for a in _share_cases_at_32():
        got = dr.draw32(*a, mutate=dr.ROUNDING_ONLY)
        assert len(dr.contract(dr.exact_draw(*a), got)[0]) == 0


def test_replay_last_write_wins_and_shadowed_entries_are_not_written():
    tokens = np.full((2, 6), 9, np.int32)
    idx = np.array([[[2 | dr.BIT30, 2, -1], [5, 7, 1 | dr.BIT30]]], np.int32)
    logits = np.zeros((1, 6, 4), np.float32)
    logits[0, np.arange(6), [0, 1, 2, 3, 0, 1]] = 50.0
    r = dr.replay_entry(tokens, logits, 4, 1, idx, np.array([1, 0]), [0, 1, 2, 3], 1, 0, None, 1, 0, 0, 0, 0, 1, mask_idx=8)
    assert r.sampled.tolist() == [[[0, 1, -1], [3, -1, 1]]]
    assert r.masked[0].tolist() == [[9, 8, 9, 9, 9, 8], [9, 9, 8, 9, 9, 9]]
    assert r.tokens.tolist() == [[9, 8, 9, 9, 9, 3], [9, 9, 1, 9, 9, 9]]
