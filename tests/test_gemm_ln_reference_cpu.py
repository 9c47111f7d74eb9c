"""Without a GPU: the conditions tests/_gemm_ln_reference.py states for its input families hold for every case of the GPU table
(tests/test_gpu_gemm_ln_kernels.py), its float64 reference agrees with tests/_row_reference.py's LayerNorm followed by a float64
product, the float32 model of the kernel's stated order is bit-exact on family a and stays inside the bound of family b in both forms
of a r g + b, and five wrong models each leave the bits or the bound on at least one case."""
import numpy as np
import pytest

import _gemm_ln_reference as lr
import _gemm_reference as gr
from _row_reference import layernorm_reference

FMTS = ("bf16", "f16")
NS = sorted({n for _, n in lr.FORCED})


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_the_pools_pass_the_kernels_own_expressions():
    """fl(fl(K m) fl(1 / K)) == m and fl(fl(K a^2) fl(1 / K)) == a^2 in numpy float32, for every K and every value used"""
    assert len(lr.M_POOL) == 32 and len(set(lr.M_POOL)) == 32 and len(lr.A_POW) >= 4 and 100 in lr.R_POOL and 0 in lr.R_POOL
    for K in lr.KS:
        inv_k = np.float32(1.0) / np.float32(K)
        for m in lr.M_POOL + lr.R_POOL:
            assert np.float32(K * m) * inv_k == np.float32(m), (K, m)
        for a in lr.A_POW:
            assert np.float32(K * a * a) * inv_k == np.float32(a * a), (K, a)


@pytest.mark.parametrize("K", lr.KS)
def test_exact_family_conditions(K):
    for N in NS + [n for n, k in lr.ENGINE if k == K]:
        e = lr.exact(N, K)
        assert e.x.shape == (32, K) and len(set(e.m)) == 32
        assert all(e.a[r] != e.a[r + 1] for r in range(31)) and all(e.a[r] != e.a[r + 16] for r in range(16))
        s = (e.x.astype(np.float64) - e.m[:, None]) / e.a[:, None]
        assert (np.abs(s) == 1).all() and (s.sum(1) == 0).all()
        assert lr.pass1_exact(e.x).all() and (np.abs(e.x).max() * 4 * K < 2 ** 24) and (e.x * 4 == np.rint(e.x * 4)).all()
        for v, lim in ((e.gamma, 4), (e.beta, 3)):
            assert (v == np.rint(v)).all() and np.abs(v).max() == lim
            assert all((np.roll(v, p) != v).any() for p in (8, 32, 256) if p < K)
        assert np.abs(e.w).max() == 8 and np.abs(e.h).max() <= 7
        assert e.mag.max() < gr.HEADROOM and 3000 <= np.abs(e.bias).min() and np.abs(e.bias).max() <= 40000
        assert np.abs(e.ref).max() < 65504
        changed = [float((gr.round_to(f, e.ref).astype(np.float64) != e.ref).mean()) for f in FMTS]
        assert min(changed) >= 0.25, changed
        # the float64 LayerNorm of these rows is the integer operand, up to float64 rounding
        assert np.abs(lr.layernorm64(e.x, e.gamma, e.beta, 0.0) - e.h).max() < 1e-12


@pytest.mark.parametrize("K", lr.KS)
def test_exact_gelu_family_conditions(K):
    for N in NS + [n for n, k in lr.ENGINE if k == K]:
        g = lr.exact_gelu(N, K)
        assert set(np.unique(g.gamma)) <= {-1.0, 0.0, 1.0} and not g.beta.any() and set(np.unique(g.w)) <= {-1.0, 0.0, 1.0}
        assert (g.z * 8 == np.rint(g.z * 8)).all() and np.abs(g.z).max() < 2 ** 10
    g = lr.exact_gelu(96, K)
    share, var = float((np.abs(g.z) <= 4).mean()), float(g.z.var())
    print("K %d: var z %.2f, |z| <= 4: %.3f" % (K, var, share))
    assert share >= 0.5 and 1.0 < var < 8.0


@pytest.mark.parametrize("K,eps", [(K, lr.eps_of(K)) for K in lr.KS] + [(K, 1e-12) for _, K in lr.ENGINE[:1]])
def test_realistic_family_conditions(K, eps):
    rows = lr.realistic_rows(K, eps)
    x64 = rows.x.astype(np.float64)
    assert lr.pass1_exact(rows.x).all()                                 # the mean-cancellation term is 0 by construction ...
    generic = (rows.x * np.float32(1.0 + 2.0 ** -20)).astype(np.float32)
    assert not lr.pass1_exact(generic).any()                            # ... and charged in full to rows that do not qualify
    _, d0 = lr.ln_delta(rows.x, rows.gamma, rows.beta, rows.eps)
    _, d1 = lr.ln_delta(generic, rows.gamma, rows.beta, rows.eps)
    assert d1[0].mean() > 50 * d0[0].mean()                             # row 0: |mean| / sigma = 100
    ratio = np.abs(x64.mean(1)) / x64.std(1)
    assert ratio.max() > 90 and ratio.min() < 0.01 and np.abs(ratio[0] - 100) < 10
    assert len(set(rows.sigma)) >= 4 and rows.sigma.max() / rows.sigma.min() >= 8
    assert np.abs(rows.gamma - 1).max() <= 0.1001 and 0.0 < rows.beta.mean() < 0.2
    share = lr.flip_shares(rows)
    print("K %d eps %g seed %d: largest flip share %.4f" % (K, rows.eps, rows.seed, share))
    assert share <= lr.MAX_FLIP_SHARE
    for N in NS:
        w, _ = lr.weights(N, K)
        assert all((gr.round_to(f, w) == w).all() for f in FMTS) and 0.02 < w.std() < 0.04


@pytest.mark.parametrize("K", lr.KS)
def test_reference_agrees_with_the_row_reference(K):
    rows, (w, bias) = lr.realistic_rows(K, lr.eps_of(K)), lr.weights(48, K)
    for fmt in FMTS:
        r = lr.reference(rows.x, rows.gamma, rows.beta, rows.eps, w, bias, fmt, False)
        h = layernorm_reference(rows.x, rows.gamma, rows.beta, rows.eps)
        assert np.abs(r.h - h).max() < 1e-12
        z = lr.round16(fmt, h) @ w.astype(np.float64).T + bias.astype(np.float64)
        assert (lr.round16(fmt, h) == r.h16).all() and np.abs(r.ref - z).max() <= 1e-12
        assert (lr.round16(fmt, r.h16) == r.h16).all() and np.abs(r.h16 - r.h).max() <= lr.U16[fmt] * np.abs(r.h).max()
        over = r.bound / (lr.U16[fmt] * np.abs(r.ref) + 1e-300)
        print("K %d %s: bound / the output's half ulp: median %.2f" % (K, fmt, np.median(over)))
        assert (over > 1).all()


def _model_cases(K):
    """(M, nb, N) of the table, thinned for the CPU: every M at one forced width, every forced width at M = 32"""
    return [(M, 1, 48) for M in lr.MS] + [(32, nb, N) for nb, N in lr.FORCED]


@pytest.mark.parametrize("K", lr.KS)
def test_model_is_exact_on_family_a_and_inside_the_bound_of_family_b(K):
    rows = lr.realistic_rows(K, lr.eps_of(K))
    worst = 0.0
    for M, nb, N in _model_cases(K):
        Mi = lr.padded(M)
        e, g, (w, bias) = lr.exact(N, K), lr.exact_gelu(N, K), lr.weights(N, K)
        xb = rows.x[:Mi].copy()
        xb[M:] = 0
        for fmt in FMTS:
            for contract in (False, True):
                out = lr.model(e.x[:Mi], e.gamma, e.beta, 0.0, e.w, e.bias, fmt, False, contract, nb=nb)
                assert (_bits(out) == _bits(gr.round_to(fmt, e.ref[:Mi]))).all(), (M, N, fmt, contract)
                out = lr.model(g.x[:Mi], g.gamma, g.beta, 0.0, g.w, g.bias, fmt, True, contract, nb=nb)
                assert (np.abs(out - g.ref[:Mi]) <= gr.gelu_bound(g._replace(z=g.z[:Mi], ref=g.ref[:Mi]), 4, fmt)).all()
                for gelu in (False, True):
                    r = lr.reference(xb[:M], rows.gamma, rows.beta, rows.eps, w, bias, fmt, gelu)
                    out = lr.model(xb, rows.gamma, rows.beta, rows.eps, w, bias, fmt, gelu, contract, nb=nb)
                    frac = float((np.abs(out[:M] - r.ref) / r.bound).max())
                    worst = max(worst, frac)
                    assert frac <= 1.0 and np.isfinite(out).all(), (M, N, fmt, contract, gelu, frac)
    print("K %d: the model's largest fraction of bound b %.3f" % (K, worst))


def test_every_wrong_model_leaves_the_bits_or_the_bound():
    caught = {name: [] for name in lr.WRONG}
    for K in lr.KS:
        rows = lr.realistic_rows(K, lr.eps_of(K))
        for nb, N in ((1, 48), (2, 64)):
            e, (w, bias) = lr.exact(N, K), lr.weights(N, K)
            for fmt in FMTS:
                r = lr.reference(rows.x, rows.gamma, rows.beta, rows.eps, w, bias, fmt, False)
                for name in lr.WRONG:
                    out = lr.model(e.x, e.gamma, e.beta, 0.0, e.w, e.bias, fmt, wrong=name, nb=nb)
                    bits = int((_bits(out) != _bits(gr.round_to(fmt, e.ref))).sum())
                    out = lr.model(rows.x, rows.gamma, rows.beta, rows.eps, w, bias, fmt, wrong=name, nb=nb)
                    frac = float(np.nanmax(np.abs(out - r.ref) / r.bound)) if np.isfinite(out).any() else np.inf
                    caught[name].append((K, nb, fmt, bits, frac, not np.isfinite(out).all()))
    for name, seen in caught.items():
        by_bits = sum(1 for s in seen if s[3] > 0)
        by_bound = sum(1 for s in seen if s[4] > 1.0 or s[5])
        print("%-52s family a bits: %d of %d cases; family b bound: %d of %d (largest fraction %.1f)" % (
            name, by_bits, len(seen), by_bound, len(seen), max(s[4] for s in seen)))
        applies = [s for s in seen if s[1] == 2] if name == lr.WRONG[4] else seen
        if name == lr.WRONG[0]:
            # family a is exact for a one-pass formula too wherever the sums of squares still fit 24 bits; family b notices it on
            # the rows of |mean| / sigma = 100 and 64 at K = 256 and 512 (beyond, term 3 of the bound grows past its effect)
            assert by_bound > 0 and by_bits + by_bound >= 4, name
            continue
        assert all(s[3] > 0 for s in applies), name                    # the exact family notices it in every case it applies to
        if name != lr.WRONG[4]:
            assert by_bound > 0, name
    # block 0's bias in block 1 changes nothing where there is one block per workgroup
    assert all(s[3] == 0 and s[4] <= 1.0 for s in caught[lr.WRONG[4]] if s[1] == 1)


def test_the_table_reaches_all_forty_instantiations():
    reached = {(lr.padded(M) // 16, gelu, K // 256, nb) for M in lr.MS for K in lr.KS for gelu in (0, 1) for nb, _ in lr.FORCED}
    assert len(reached) == 40
    assert all(N % (16 * nb) == 0 for nb, N in lr.FORCED)
    assert [lr.expected_nb(N, 256) for N, _ in lr.ENGINE] == [1, 2] and lr.expected_nb(5120, 320) == 1
