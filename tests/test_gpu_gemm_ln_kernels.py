"""Kernel-level parity of the single-chain GEMM with the folded LayerNorm (gemm_ln_skinny_kernel) on the MI355X, launched alone through
pg_dbg_gemm_ln in both 16-bit operand flavours, against the references of tests/_gemm_ln_reference.py --

  * family a: bit for bit against the int64 result rounded to the flavour, all Mi rows; its GELU sub-family per element under the
    documented epilogue error on exact pre-activations;
  * family b: every element within the derived bound (float64 LayerNorm, operand rounded once, float64 product), rows with
    |mean| / sigma up to 100;
  * family c: the live rows' bits do not depend on what the padding rows hold, and nothing is written outside out[Mi][N];
  * invariants that hold by construction, bit for bit: nb = 1 against nb = 2, an M = 32 call against the M = 16 call on its first 16
    rows, an N = 64 call against the N = 32 call on its first 32 features.

Every launch's recorded plan text must be `ln+skinny8w <N / (16 nb)>t`; the last test holds the set of (MT, EPI, NKS, NB) instances
launched over the file to all 40.  PGIBBS_GEMM_LN_FRACTIONS=<file> appends the largest fraction of each bound per epilogue and flavour
(the table in DESIGN.md)."""
import ctypes
import os

import numpy as np
import pytest

import _gemm_ln_reference as lr
import _gemm_reference as gr
from protein_gibbs_sampler_amd import _lib

pytestmark = pytest.mark.gpu
PREC = {"bf16": _lib.PG_PREC_BF16, "f16": _lib.PG_PREC_F16}
FLAVOURS = ("bf16", "f16")
REACHED = {fmt: set() for fmt in FLAVOURS}
GUARD = 16                                                               # rows of the caller's pattern behind out[Mi][N]


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _pattern(rows, N):
    """small integers, exact in bf16 and in fp16, that differ along both axes"""
    return ((np.arange(rows * N).reshape(rows, N) * 7) % 251 - 125).astype(np.float32)


def _run(fmt, x, x_pad, gamma, beta, eps, w, bias, gelu, nb):
    """-> out[Mi][N]; asserts the plan text, the untouched guard rows and records the instance"""
    (M, K), N = x.shape, w.shape[0]
    Mi = lr.padded(M)
    assert x_pad is None or x_pad.shape == (Mi - M, K)
    x, x_pad = np.ascontiguousarray(x), None if x_pad is None or Mi == M else np.ascontiguousarray(x_pad)
    out = np.full((Mi + GUARD, N), np.nan, np.float32)
    out[Mi:] = _pattern(GUARD, N)
    plan = ctypes.create_string_buffer(256)
    _lib.check(_lib.lib().pg_dbg_gemm_ln(0, PREC[fmt], _lib.ptr(x), None if x_pad is None else _lib.ptr(x_pad), _lib.ptr(gamma),
                                         _lib.ptr(beta), eps, _lib.ptr(w), _lib.ptr(bias), _lib.ptr(out), Mi + GUARD, M, N, K, int(gelu),
                                         nb, plan, 256))
    ran = plan.value.decode()
    used = nb or lr.expected_nb(N, _n_cu())
    assert ran == "ln+skinny8w %dt" % (N // (16 * used)), (ran, N, nb)
    assert (_bits(out[Mi:]) == _bits(_pattern(GUARD, N))).all(), "rows behind out[Mi][N] were written"
    REACHED[fmt].add((Mi // 16, int(gelu), K // 256, used))
    return out[:Mi]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_bits(out, want, what):
    bad = _bits(out) != _bits(want)
    if bad.any():
        r, c = np.argwhere(bad)[0]
        raise AssertionError("%s: %d of %d outputs differ, rows %d..%d, first at [%d, %d]: %r, expected %r" % (
            what, bad.sum(), bad.size, np.argwhere(bad)[:, 0].min(), np.argwhere(bad)[:, 0].max(), r, c, out[r, c], want[r, c]))


def _note(key, frac):
    path = os.environ.get("PGIBBS_GEMM_LN_FRACTIONS")
    if path:
        with open(path, "a") as f:
            f.write("%s\t%.4f\n" % (" ".join(map(str, key)), frac))


def _check_bound(out, ref, bound, key, what):
    assert np.isfinite(out).all(), what
    err = np.abs(out.astype(np.float64) - ref)
    frac = float((err / np.maximum(bound, 1e-300)).max())
    print("%s: worst |err| / bound %.3f (max |err| %.3e)" % (what, frac, err.max()))
    _note(key, frac)
    if frac > 1.0:
        r, c = np.unravel_index(np.argmax(err / bound), err.shape)
        raise AssertionError("%s: %d of %d outputs leave the bound, worst %.2f x at [%d, %d]: %r, reference %r" % (
            what, (err > bound).sum(), err.size, frac, r, c, out[r, c], ref[r, c]))


def _family_a(fmt, M, N, K, gelu, nb):
    Mi = lr.padded(M)
    what = "family a %s M %d N %d K %d gelu %d nb %d" % (fmt, M, N, K, gelu, nb)
    if gelu:
        g = lr.exact_gelu(N, K)
        out = _run(fmt, g.x[:M], g.x[M:Mi], g.gamma, g.beta, 0.0, g.w, g.bias, True, nb)
        _check_bound(out, g.ref[:Mi], gr.gelu_bound(g._replace(z=g.z[:Mi], ref=g.ref[:Mi]), 4, fmt), ("a gelu_poly2", fmt), what)
    else:
        e = lr.exact(N, K)
        out = _run(fmt, e.x[:M], e.x[M:Mi], e.gamma, e.beta, 0.0, e.w, e.bias, False, nb)
        _assert_bits(out, gr.round_to(fmt, e.ref[:Mi]), what)


def _family_b(fmt, M, N, K, gelu, nb, eps=None):
    rows, (w, bias) = lr.realistic_rows(K, lr.eps_of(K) if eps is None else eps), lr.weights(N, K)
    r = lr.reference(rows.x[:M], rows.gamma, rows.beta, rows.eps, w, bias, fmt, gelu)
    assert (r.flip != 0).mean() <= lr.MAX_FLIP_SHARE
    out = _run(fmt, rows.x[:M], None, rows.gamma, rows.beta, rows.eps, w, bias, gelu, nb)
    assert np.isfinite(out).all()                                       # zero padding rows: LayerNorm gives beta
    _check_bound(out[:M], r.ref, r.bound, ("b gelu" if gelu else "b plain", fmt),
                 "family b %s M %d N %d K %d gelu %d nb %d" % (fmt, M, N, K, gelu, nb))


@pytest.mark.parametrize("K", lr.KS)
@pytest.mark.parametrize("M", lr.MS)
def test_exact_family_bit_for_bit(M, K):
    """assertions 1 and 3, and the GELU half of 2: every forced width, both epilogues, both flavours"""
    for nb, N in lr.FORCED:
        for gelu in (False, True):
            for fmt in FLAVOURS:
                _family_a(fmt, M, N, K, gelu, nb)


@pytest.mark.parametrize("K", lr.KS)
@pytest.mark.parametrize("M", lr.MS)
def test_realistic_family_within_its_bound(M, K):
    """assertions 2 and 3"""
    for nb, N in lr.FORCED:
        for gelu in (False, True):
            for fmt in FLAVOURS:
                _family_b(fmt, M, N, K, gelu, nb)


@pytest.mark.parametrize("shape", lr.ENGINE, ids=lambda s: "%dx%d" % s)
def test_engine_widths_with_the_launchers_choice(shape):
    """nb = 0: the plan text must be what the launcher's rule gives for this device's CU count (_run asserts it)"""
    N, K = shape
    for M in (15, 32):
        for gelu in (False, True):
            for fmt in FLAVOURS:
                _family_a(fmt, M, N, K, gelu, 0)
                _family_b(fmt, M, N, K, gelu, 0, eps=1e-12)


@pytest.mark.parametrize("K", (256, 1280))
def test_invariants_bit_for_bit(K):
    rows = lr.realistic_rows(K, lr.eps_of(K))
    (w, bias), args = lr.weights(64, K), (rows.gamma, rows.beta, rows.eps)
    for fmt in FLAVOURS:
        for gelu in (False, True):
            one = _run(fmt, rows.x, None, *args, w, bias, gelu, 1)
            _assert_bits(_run(fmt, rows.x, None, *args, w, bias, gelu, 2), one, "nb 2 against nb 1, %s gelu %d" % (fmt, gelu))
            for nb in (1, 2):
                _assert_bits(_run(fmt, rows.x[:16], None, *args, w, bias, gelu, nb), one[:16], "M 16 against M 32, %s nb %d" % (fmt, nb))
                _assert_bits(_run(fmt, rows.x, None, *args, w[:32], bias[:32], gelu, nb), one[:, :32], "N 32 against N 64, %s nb %d" % (fmt, nb))


@pytest.mark.parametrize("K", (512, 1280))
@pytest.mark.parametrize("M", (1, 15, 17, 31))
def test_live_rows_do_not_depend_on_the_padding_rows(M, K):
    """family c; _run checks the rows behind out[Mi][N] on every launch"""
    rows, Mi = lr.realistic_rows(K, lr.eps_of(K)), lr.padded(M)
    rng = np.random.default_rng([K, M])
    pads = {"zeros": np.zeros((Mi - M, K), np.float32),
            "near 1e30": (1e30 * (1 + rng.random((Mi - M, K))) * rng.choice([-1, 1], (Mi - M, K))).astype(np.float32),
            "NaN": np.full((Mi - M, K), np.nan, np.float32)}
    for nb, N in ((1, 48), (2, 64)):
        w, bias = lr.weights(N, K)
        for fmt in FLAVOURS:
            for gelu in (False, True):
                want = _run(fmt, rows.x[:M], None, rows.gamma, rows.beta, rows.eps, w, bias, gelu, nb)[:M]
                for name, pad in pads.items():
                    got = _run(fmt, rows.x[:M], pad, rows.gamma, rows.beta, rows.eps, w, bias, gelu, nb)[:M]
                    _assert_bits(got, want, "padding rows of %s, %s M %d N %d gelu %d" % (name, fmt, M, N, gelu))


def test_every_instantiation_was_launched():
    """the 40 instances per flavour: m-tiles 1, 2 x plain, GELU x 1 ... 5 k-steps per wave x 1, 2 feature blocks"""
    every = {(mt, e, nks, nb) for mt in (1, 2) for e in (0, 1) for nks in (1, 2, 3, 4, 5) for nb in (1, 2)}
    for fmt in FLAVOURS:
        assert REACHED[fmt] == every, (fmt, sorted(every - REACHED[fmt]))
