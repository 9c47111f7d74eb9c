"""Kernel-level parity of the GEMM kernels on the MI355X: every tile kernel forced by variant through pg_dbg_gemm_v, in both 16-bit
operand flavours, against the references of tests/_gemm_reference.py --

  * bit for bit against the int64 result on small-integer operands (fp32 outputs, the residual read-modify-write, split-K with and
    without scratch) and against its round-to-nearest-even conversion (16-bit outputs): any dropped, doubled or misplaced k, row,
    column, tile, split, bias or residual differs by at least 1;
  * per element under the documented epilogue error for the two GELU forms on exact pre-activations;
  * the strict mode's plain and fused three-product kernels bit for bit against the three-product definition in int64.

Every launch's recorded plan text must name the kernel the case is meant to run, with its tile count where that does not depend on the
CU count, and equal pg_dbg_gemm_plan's answer for the device's own CU count.  PGIBBS_GEMM_FRACTIONS=<file> appends the largest
fraction of the GELU bound per epilogue and flavour (the table in DESIGN.md)."""
import ctypes
import functools
import os

import numpy as np
import pytest

import _gemm_reference as gr
from protein_gibbs_sampler_amd import _lib

pytestmark = pytest.mark.gpu
PREC = {"bf16": _lib.PG_PREC_BF16, "f16": _lib.PG_PREC_F16, "f32": _lib.PG_PREC_FP32}
FLAVOURS = ("bf16", "f16")
FRACTIONS = {}


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _plan(M, N, K, epi, variant, have_ws, m_live):
    buf = ctypes.create_string_buffer(256)
    _lib.check(_lib.lib().pg_dbg_gemm_plan(M, N, K, gr.EPI_INTERNAL[epi], variant, have_ws, m_live, _n_cu(), buf, 256))
    return buf.value.decode()


def _run(fmt, x, w, bias, res, epi, variant=-1, have_ws=-1):
    (M, K), N = x.shape, w.shape[0]
    out = np.full((M, N), np.nan, np.float32) if res is None else res.copy()
    plan = ctypes.create_string_buffer(256)
    _lib.check(_lib.lib().pg_dbg_gemm_v(0, PREC[fmt], _lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(out), M, N, K, epi, variant, have_ws,
                                        M, plan, 256))
    return out, plan.value.decode()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_bits(out, want, what):
    bad = _bits(out) != _bits(want)
    if bad.any():
        r, c = np.argwhere(bad)[0]
        raise AssertionError("%s: %d of %d outputs differ, rows %d..%d, first at [%d, %d]: %r, expected %r" % (
            what, bad.sum(), bad.size, np.argwhere(bad)[:, 0].min(), np.argwhere(bad)[:, 0].max(), r, c, out[r, c], want[r, c]))


@functools.lru_cache(maxsize=4)
def _exact(M, N, K, residual, out16):
    return gr.integers(M, N, K, seed=1, residual=residual, out16=out16)


@functools.lru_cache(maxsize=2)
def _gelu(M, N, K):
    return gr.gelu_inputs(M, N, K, seed=3)


def _note(key, frac):
    FRACTIONS[key] = max(FRACTIONS.get(key, 0.0), frac)
    path = os.environ.get("PGIBBS_GEMM_FRACTIONS")
    if path:
        with open(path, "a") as f:
            f.write("%s\t%.4f\n" % (" ".join(map(str, key)), frac))


def _check_gelu(out, g, epi, kind, key):
    assert np.isfinite(out).all(), key
    err, bound = np.abs(out.astype(np.float64) - g.ref), gr.gelu_bound(g, epi, kind)
    frac = float((err / np.maximum(bound, 1e-300)).max())
    print("%s: worst |err| / bound %.3f (max |err| %.3e)" % (" ".join(map(str, key)), frac, err.max()))
    _note(key, frac)
    assert (err <= bound).all(), (key, frac)


def _check_plan(c, epi, ran, have_ws):
    want = gr.expected_plan(c._replace(epis=(epi,)))
    assert ran.startswith(want), (ran, want)
    if not c.strict:
        assert ran == _plan(gr.launched_rows(c.M), c.N, c.K, epi, c.variant, have_ws, c.M), ran


NON_STRICT = [c for c in gr.CASES if not c.strict]
STRICT = [c for c in gr.CASES if c.strict]
_id = lambda c: "%s-v%d-ws%d-%dx%dx%d" % (c.kernel, c.variant, c.have_ws, c.M, c.N, c.K)


@pytest.mark.parametrize("case", NON_STRICT, ids=_id)
def test_tile_kernel(case):
    c = case
    for epi in c.epis:
        have_ws = int(epi == 2) if c.have_ws < 0 else c.have_ws      # what -1 means to the entry, for the plan function
        for fmt in FLAVOURS:
            what = "%s epi %d %s" % (_id(c), epi, fmt)
            if epi in (1, 4):
                g = _gelu(c.M, c.N, c.K)
                out, ran = _run(fmt, g.x, g.w, g.bias, None, epi, c.variant, c.have_ws)
                _check_plan(c, epi, ran, have_ws)
                _check_gelu(out, g, epi, "f32" if epi == 1 else fmt, ("gelu_erf" if epi == 1 else "gelu_poly2", fmt))
                continue
            e = _exact(c.M, c.N, c.K, epi == 2, epi == 3)
            out, ran = _run(fmt, e.x, e.w, e.bias, e.res, epi, c.variant, c.have_ws)
            _check_plan(c, epi, ran, have_ws)
            _assert_bits(out, gr.round_to(fmt, e.ref) if epi == 3 else e.ref.astype(np.float32), what)


@pytest.mark.parametrize("epi", [3, 2])
def test_production_grid_of_big_tiles_and_tail_tiles(epi):
    """the 16-wave kernel (16-bit output) and the 8-wave kernel (residual) with a panel of 64 x 64 tail tiles in the same grid"""
    M, N, K = gr.PRODUCTION_TAIL
    want = _plan(M, N, K, epi, 2, int(epi == 2), M)
    if "tail64" not in want:
        pytest.skip("%d CUs: the plan of %d x %d has no tail tiles (%s)" % (_n_cu(), M, N, want))
    assert want.startswith("w16-256x256" if epi == 3 else "pp256x256"), want
    e = _exact(M, N, K, epi == 2, epi == 3)
    for fmt in FLAVOURS:
        out, ran = _run(fmt, e.x, e.w, e.bias, e.res, epi, 2)
        assert ran == want, (ran, want)
        _assert_bits(out, gr.round_to(fmt, e.ref) if epi == 3 else e.ref.astype(np.float32), "production %s epi %d" % (fmt, epi))


@pytest.mark.parametrize("case", STRICT, ids=_id)
def test_strict_kernel(case):
    c = case
    for epi in c.epis:
        if epi == 5:
            g = _gelu(c.M, c.N, c.K)
            out, ran = _run("f32", g.x, g.w, g.bias, None, 5)
            _check_plan(c, epi, ran, 0)
            _check_gelu(out, g, 5, "pair", ("gelu_poly2", "strict"))
            continue
        e = gr.strict_integers(c.M, c.N, c.K, seed=2, residual=epi == 2)
        out, ran = _run("f32", e.x, e.w, e.bias, e.res, epi)
        _check_plan(c, epi, ran, 0)
        _assert_bits(out, e.ref.astype(np.float32), "%s epi %d" % (_id(c), epi))


@pytest.mark.parametrize("shape", gr.BIG_STRICT, ids=lambda s: "%dx%dx%d" % s)
def test_strict_fused_kernel_on_256_row_tiles(shape):
    """the smallest shapes that give the fused three-product kernel a full round of 256 x 256 tiles, without and with a panel of tail
    tiles behind it (256 CUs: 256 tiles; 256 tiles + 64 tail tiles); plain, residual and the fused fc1 epilogue"""
    M, N, K = shape
    n_cu = _n_cu()
    for epi in (0, 2, 5):
        if epi == 5:
            g = _gelu(M, N, K)
            out, ran = _run("f32", g.x, g.w, g.bias, None, 5)
            _check_gelu(out, g, 5, "pair", ("gelu_poly2", "strict"))
        else:
            e = gr.strict_integers(M, N, K, seed=2, residual=epi == 2)
            out, ran = _run("f32", e.x, e.w, e.bias, e.res, epi)
            _assert_bits(out, e.ref.astype(np.float32), "strict fused %s epi %d" % (shape, epi))
        assert ran.startswith("gemm_split3_w16"), ran
        if n_cu == 256:
            assert ran == ("gemm_split3_w16 256t" if M == 16384 else "gemm_split3_w16 256t + tail64 64t"), ran


def test_have_ws_is_ignored_by_the_other_epilogues():
    """scratch on offer to a plain and a 16-bit epilogue at a depth that would split: the plan does not split, the result is exact"""
    M, N, K = 32, 128, 2048
    for epi in (0, 3):
        e = _exact(M, N, K, False, epi == 3)
        out, ran = _run("bf16", e.x, e.w, e.bias, None, epi, 2, 1)
        assert ran == "skinny8w 8t", ran
        _assert_bits(out, gr.round_to("bf16", e.ref) if epi == 3 else e.ref.astype(np.float32), "epi %d" % epi)


def test_pg_dbg_gemm_is_the_new_entry_with_defaults():
    e = _exact(129, 128, 2048, True, False)
    a, ran = _run("bf16", e.x, e.w, e.bias, e.res, 2)
    b = e.res.copy()
    _lib.check(_lib.lib().pg_dbg_gemm(0, PREC["bf16"], _lib.ptr(e.x), _lib.ptr(e.w), _lib.ptr(e.bias), _lib.ptr(b), 129, 128, 2048, 2))
    assert ran == "tile64x64 6t x2k" and (_bits(a) == _bits(b)).all()
    _assert_bits(a, e.ref.astype(np.float32), "pg_dbg_gemm")
