"""Without a GPU: the conditions tests/_gemm_reference.py states for its input families hold for every case of the GPU table
(tests/test_gpu_gemm_kernels.py), a float32 restatement of the kernels' arithmetic reproduces the references bit for bit in a
shuffled k order, four wrong models of a kernel each differ from the reference wherever they apply, and the dispatch (256 CUs)
puts every case on the kernel it is meant to run."""
import ctypes

import numpy as np
import pytest

import _gemm_reference as gr
from protein_gibbs_sampler_amd import _lib

SHAPES = sorted({(c.M, c.N, c.K) for c in gr.CASES if not c.strict})
STRICT_SHAPES = sorted({(c.M, c.N, c.K) for c in gr.CASES if c.strict and 5 not in c.epis})
GELU_SHAPES = sorted({(c.M, c.N, c.K) for c in gr.CASES if set(c.epis) & {1, 4, 5}})
IDS = lambda s: "%dx%dx%d" % s


def _changed(fmt, ref):
    return float((gr.round_to(fmt, ref).astype(np.float64) != ref).mean())


@pytest.mark.parametrize("shape", SHAPES + [gr.PRODUCTION_TAIL], ids=IDS)
def test_integer_family_conditions(shape):
    for residual in (False, True):
        e = gr.integers(*shape, seed=1, residual=residual)
        assert e.mag.max() < gr.HEADROOM and np.abs(e.x).max() <= 8 and np.abs(e.w).max() <= 8
        assert np.abs(e.bias).max() <= 2 ** 20 and (e.res is None or np.abs(e.res).max() <= 2 ** 20)
        assert (e.ref.astype(np.float32).astype(np.int64) == e.ref).all()
    e = gr.integers(*shape, seed=1, out16=True)
    assert e.mag.max() < gr.HEADROOM and np.abs(e.ref).max() < 65504
    shares = {fmt: _changed(fmt, e.ref) for fmt in ("bf16", "f16")}
    u = e.ref.astype(np.float32).view(np.uint32)
    ties = {"bf16": float(((u & 0xFFFF) == 0x8000).mean()), "f16": float(((u & 0x1FFF) == 0x1000).mean())}      # halfway cases
    print("rounded away: %s; ties: %s" % (shares, ties))
    assert min(shares.values()) >= 0.25
    assert e.ref.size < 4096 or min(ties.values()) > 0.005


@pytest.mark.parametrize("shape", STRICT_SHAPES + list(gr.BIG_STRICT[:1]), ids=IDS)
def test_strict_family_conditions(shape):
    e = gr.strict_integers(*shape, seed=2, residual=True)
    assert e.mag.max() < gr.HEADROOM
    (xh, xl), (wh, wl) = gr.split_pair(e.x), gr.split_pair(e.w)
    assert set(np.unique(np.abs(xl))) == {0.0, 1.0} and set(np.unique(np.abs(xh[np.abs(e.x) > 8]))) == {256.0, 384.0}
    assert set(np.unique(np.abs(wl))) == {0.0, 1.0}
    share = gr.shared_nine_bit(e)
    print("pairs of rows that share the k of a 9-bit value: %.3f" % share)
    assert 0 < share < 0.5
    true = gr._matmul_exact(e.x, e.w) + e.bias.astype(np.int64) + e.res.astype(np.int64)
    dropped = gr._matmul_exact(xl, wl)
    assert (true - dropped == e.ref).all() and (dropped != 0).any()


@pytest.mark.parametrize("shape", GELU_SHAPES, ids=IDS)
def test_gelu_family_conditions(shape):
    g = gr.gelu_inputs(*shape, seed=3)
    z32 = (g.x @ g.w.T + g.bias).astype(np.float32)
    assert (z32.astype(np.float64) == g.z).all() and (g.z * 8 == np.rint(g.z * 8)).all()      # exact: integers + eighths
    share, var = float((np.abs(g.z) <= 4).mean()), float(g.z.var())
    print("var z %.2f, |z| <= 4: %.3f" % (var, share))
    assert share >= 0.5 and 2.0 < var < 8.0


def _splits(c):
    return gr.splitk_splits(c.K) if c.have_ws == 1 and 2 in c.epis else 1


def _tail_row0(c):
    return gr.launched_rows(c.M) // 192 * 192 if c.kernel == "pp192x256" and c.M % 192 else None


RESTATE = [c for c in gr.CASES if not c.strict and (c.kernel in ("pp192x256", "pp256x256", "skinny4w") or c.have_ws == 1) and c.M <= 768]


@pytest.mark.parametrize("case", RESTATE, ids=lambda c: "%s-v%d-%dx%dx%d" % (c.kernel, c.variant, c.M, c.N, c.K))
def test_float32_restatement_and_wrong_models(case):
    c = case
    residual = 2 in c.epis
    e = gr.integers(c.M, c.N, c.K, seed=1, residual=residual)
    got = gr.restate_f32(e.x, e.w, e.bias, e.res, _splits(c), np.random.default_rng(c.K))
    assert (got.view(np.uint32) == e.ref.astype(np.float32).view(np.uint32)).all()
    applied = 0
    for name, wrong in gr.wrong_models(e, _splits(c), _tail_row0(c)).items():
        if wrong is None:
            continue
        applied += 1
        assert (wrong != e.ref).any(), name
    assert applied >= 2 + (_splits(c) > 1) + (_tail_row0(c) is not None and residual)


@pytest.mark.parametrize("shape", STRICT_SHAPES, ids=IDS)
def test_strict_restatement_and_wrong_models(shape):
    e = gr.strict_integers(*shape, seed=2, residual=True)
    (xh, xl), (wh, wl) = gr.split_pair(e.x), gr.split_pair(e.w)
    products = [(xl, wh), (xh, wl), (xh, wh)]
    got = gr.restate_f32(e.x, e.w, e.bias, e.res, 1, np.random.default_rng(5), products)
    assert (got.view(np.uint32) == e.ref.astype(np.float32).view(np.uint32)).all()
    for name, wrong in gr.wrong_models(e, 1, None, products).items():
        assert wrong is None or (wrong != e.ref).any(), name
    # the lo block of x taken from the hi block (xl := xh in the first product), and from the next 32-column group
    assert (gr._matmul_exact(xh, wh) * 2 + gr._matmul_exact(xh, wl) + e.bias.astype(np.int64) + e.res.astype(np.int64) != e.ref).any()
    shifted = np.roll(xl, 32, axis=1)
    assert (gr._matmul_exact(shifted, wh) + gr._matmul_exact(xh, wl) + gr._matmul_exact(xh, wh) + e.bias.astype(np.int64)
            + e.res.astype(np.int64) != e.ref).any()


def _plan(M, N, K, epi, variant, have_ws, n_cu=256):
    buf = ctypes.create_string_buffer(256)
    _lib.check(_lib.lib().pg_dbg_gemm_plan(M, N, K, gr.EPI_INTERNAL[epi], variant, have_ws, M, n_cu, buf, 256))
    return buf.value.decode()


def test_every_case_is_planned_onto_its_kernel():
    """on 256 CUs; the GPU test repeats this with the text the launch recorded on the device it runs on"""
    for c in gr.CASES:
        if c.strict and 5 in c.epis:
            continue                                    # launch_gemm_split3_w16 has no plan function
        for epi in c.epis:
            rows, K = ((c.M + 255) // 256 * 256, 3 * c.K) if c.strict else (gr.launched_rows(c.M), c.K)
            have_ws = int(epi == 2) if c.have_ws < 0 else c.have_ws
            got = _plan(rows, c.N, K, epi, 2 if c.strict else c.variant, 0 if c.strict else have_ws)
            want = gr.expected_plan(c._replace(epis=(epi,)))
            assert got == want, (c, epi, got, want)
    M, N, K = gr.PRODUCTION_TAIL
    assert _plan(M, N, K, 3, 2, 0) == "w16-256x256 256t + tail64 256t"
    assert _plan(M, N, K, 2, 2, 1) == "pp256x256 256t + tail64 256t"


def test_the_table_covers_every_kernel_label():
    labels = {c.kernel for c in gr.CASES}
    assert labels == {"skinny4w", "skinny8w", "tile64x64", "tile128x128", "tile256x256-lockstep", "pp256x256", "pp192x256", "w16-256x256",
                      "gemm_split3_w16"}
    split = {(c.kernel, gr.splitk_splits(c.K)) for c in gr.CASES if c.have_ws == 1}
    assert split == {(k, s) for k in ("skinny8w", "tile64x64", "tile128x128") for s in (2, 3, 4)}
