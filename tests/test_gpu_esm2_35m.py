"""ESM-2 35M (esm2_t12_35M_UR50D: 20 heads of 24, d_model 480; models.ESM2_35M) on the HIP engine.  The model runs embedded: every
head in a slot of 32, rows of 640 features whose last 160 are structural zeros (include/pgibbs.h pg_engine_create_embedded), on the
GEMM, attention and rotary kernels of the 150M shape.  The one kernel family that had to learn something is the row kernels, which
normalise over the live features and write zeros behind them: here each of them in its live-width form against the existing entry on
rows of d = d_live, bit for bit; the refusals that stay; and the engine forward against the numpy reference at the NATURAL shape
(heads of 24) and a HuggingFace fixture, under the bounds the 150M row holds for the same kernels at the same run shape (the shared
bodies of tests/_esm2_gpu_common.py).  The full size, precision="auto" and the sampler are the esm2_35m rows of
tests/test_gpu_esm2_sizes.py."""
import ctypes

import numpy as np
import pytest

import _esm2_gpu_common as common
import _row_reference as rr
import test_gpu_row_kernels as rk
from _esm2_sizes import PRECISIONS, SIZES
from _ln_host import PLAIN, SPLIT_DUP, SPLIT_NODUP
from protein_gibbs_sampler_amd import _lib, models, weights

pytestmark = pytest.mark.gpu

F32 = np.float32
_p = rk._p


# ---- the row kernels in their live-width form ------------------------------------------------------------------------------------------
# (M, d, d_live): 35M's own row (two chunks per lane of which the second is 7/8 full -> 120 live chunks, 40 pad chunks); one chunk
# that is 3/4 live; the 10-chunk instantiation with a pad shorter than a wave
LIVE_CASES = [(5, 640, 480), (3, 128, 96), (9, 2560, 2400)]


def _padded(a, d, fill=np.nan):
    """a[..., d_live] -> [..., d] with `fill` behind the live features: what a kernel must not read (NaN) or must pass through"""
    out = np.full(a.shape[:-1] + (d,), fill, dtype=a.dtype)
    out[..., :a.shape[-1]] = a
    return out


def _check_live_rows(h, want, M, d, dl, form, case):
    """h[rows][d or 3 d] from a live-width entry, want[rows][dl or 3 dl] from the existing entry on rows of dl features"""
    if form == PLAIN:
        assert np.array_equal(h[:M, :dl], want[:M]), case
        assert (h[:M, dl:] == 0).all(), case
    else:
        assert np.array_equal(h[:M, :3 * dl], want[:M]), case                      # whole groups of 32 columns: dl is a multiple of 32
        pad = h[:M, 3 * dl:].reshape(M, (d - dl) // 32, 3, 32)
        assert (pad[:, :, :2] == 0).all(), case                                     # [lo | hi] of every pad group
        assert (pad[:, :, 2] == (rk.FILL if form == SPLIT_NODUP else 0)).all(), case
    assert (h[M:] == rk.FILL).all(), case


def _ln_rows_live(x, g, b, dl, form, prec, extra=3):
    M, d = x.shape
    h = np.full((M + extra, d * (3 if form else 1)), rk.FILL, dtype=np.uint16)
    k = ctypes.c_int(-1)
    _lib.check(_lib.lib().pg_embedded_layernorm_rows(0, prec, _p(x), _p(g), _p(b), _p(h), h.shape[0], M, d, rk.EPS, form, 0, 0, ctypes.byref(k), dl))
    return h, rk.KERNEL[k.value]


@pytest.mark.parametrize("M, d, dl", LIVE_CASES)
def test_live_layernorm_rows_are_the_rows_of_the_live_width(M, d, dl):
    xl = rk._rows(M, dl, M * 7 + dl)
    gl, bl = rk._affine(dl, dl)
    x, g, b = _padded(xl, d), _padded(gl, d), _padded(bl, d)                        # NaN behind the live features: never read
    for name, prec, form in rk.FORMS:
        want, _ = rk.ln_rows(xl, gl, bl, form, prec)
        h, kernel = _ln_rows_live(x, g, b, dl, form, prec)
        assert kernel == "plain"
        _check_live_rows(h, want, M, d, dl, form, (name, M, d, dl))
    # d_live == d: the existing entry, bit for bit
    xf = rk._rows(M, d, M + d)
    gf, bf = rk._affine(d, d + 1)
    for name, prec, form in rk.FORMS:
        assert np.array_equal(_ln_rows_live(xf, gf, bf, d, form, prec)[0], rk.ln_rows(xf, gf, bf, form, prec)[0]), name


@pytest.mark.parametrize("M, d, dl", [(4, 64, 48), (6, 640, 496)])
def test_live_split_rows_with_a_half_live_group(M, d, dl):
    """A head count that is no multiple of 4 (2 heads of 24 in rows of 64) ends the live features in the middle of a group of 32
    columns of the strict mode's rows: chunks 0 .. 3 of that group hold values, chunks 4 .. 7 zeros.  The existing split entry takes
    whole groups only, so the rows are built on the host: the fp32 LayerNorm of the same kernel arithmetic (pg_dbg_layernorm at
    d = d_live), zeros behind it, through store_rows_host -- the layout's independent restatement."""
    from _ln_host import store_rows_host
    xl = rk._rows(M, dl, M + dl)
    gl, bl = rk._affine(dl, dl + 1)
    y = np.full_like(xl, np.nan)
    _lib.check(_lib.lib().pg_dbg_layernorm(0, _p(xl), _p(gl), _p(bl), _p(y), M, dl, rk.EPS))
    x, g, b = _padded(xl, d), _padded(gl, d), _padded(bl, d)
    for name, prec, form in rk.FORMS:
        h, kernel = _ln_rows_live(x, g, b, dl, form, prec)
        want = store_rows_host(_padded(y, d, 0.0), form, prec == rk.F16, rk.FILL)
        assert kernel == "plain" and np.array_equal(h[:M], want) and (h[M:] == rk.FILL).all(), (name, M, d, dl)
        if form == PLAIN:
            assert np.array_equal(h[:M, :dl], rk.ln_rows(xl, gl, bl, form, prec)[0][:M])


def test_live_layernorm_never_takes_the_stride_kernel_and_has_no_column_major_form():
    """8448 rows of 1280 features are the stride kernel's; with a live width the plain kernel runs"""
    M, d, dl = 8448, 1280, 1248
    xl = rk._rows(M, dl, 5)
    gl, bl = rk._affine(dl, 6)
    want, kernel = rk.ln_rows(xl, gl, bl, PLAIN, rk.BF16, extra=1)
    h, kernel_live = _ln_rows_live(_padded(xl, d), _padded(gl, d), _padded(bl, d), dl, PLAIN, rk.BF16, extra=1)
    assert kernel_live == "plain"
    _check_live_rows(h, want, M, d, dl, PLAIN, "stride")
    assert _ln_rows_live(rk._rows(M, d, 7), *rk._affine(d, 8), d, PLAIN, rk.BF16, extra=1)[1] == "stride"      # d_live == d: as ever
    L = _lib.lib()
    x, g = np.zeros((24, 768), F32), np.zeros(768, F32)
    hh = np.full((24, 768), rk.FILL, dtype=np.uint16)
    assert L.pg_embedded_layernorm_rows(0, rk.BF16, _p(x), _p(g), _p(g), _p(hh), 24, 24, 768, rk.EPS, PLAIN, 3, 8, None, 736) == _lib.PG_ERR_INVALID
    assert b"column-major" in L.pg_last_error() and (hh == rk.FILL).all()
    for bad in (0, 6, 772, -4):
        assert L.pg_embedded_layernorm_rows(0, rk.BF16, _p(x), _p(g), _p(g), _p(hh), 24, 24, 768, rk.EPS, PLAIN, 0, 0, None, bad) == _lib.PG_ERR_INVALID


def _gather_ln_live(x, idx, row_map, P, width, g, b, n_sel, split, prec, dl, extra=2):
    d = x.shape[1]
    h = np.full((n_sel + extra, d * (3 if split else 1)), rk.FILL, dtype=np.uint16)
    _lib.check(_lib.lib().pg_embedded_gather_ln(0, prec, _p(x), x.shape[0], _p(idx), _p(row_map), 0 if row_map is None else len(row_map), P,
                                                width, _p(g), _p(b), _p(h), h.shape[0], n_sel, d, rk.EPS, int(split), dl))
    return h


@pytest.mark.parametrize("M, d, dl", LIVE_CASES)
def test_live_gather_layernorm(M, d, dl):
    width, P, n_seq = 9, 2, 6
    n_sel = n_seq * P + 1 - 2                                                       # 11 rows: the last workgroup is 3/4 full
    xl = rk._rows(n_seq * width, dl, M + dl)
    gl, bl = rk._affine(dl, dl + 3)
    x, g, b = _padded(xl, d), _padded(gl, d), _padded(bl, d)
    rng = np.random.default_rng(d)
    idx = rng.integers(0, width, n_sel).astype(np.int32)
    idx[1], idx[4], idx[6], idx[7] = -1, width + 1, 3 | rk.SHADOW, (width - 1) | rk.SHADOW      # a zero row, one past the width, shadowed
    row_map = rng.permutation(n_seq).astype(np.int32)
    for split, prec in ((0, rk.BF16), (1, rk.BF16), (0, rk.F16)):
        form = SPLIT_DUP if split else PLAIN
        for im, rm in ((idx, None), (idx, row_map), (None, None)):
            want = rk.gather_ln(xl, im, rm, P, width, gl, bl, n_sel, split, prec)
            h = _gather_ln_live(x, im, rm, P, width, g, b, n_sel, split, prec, dl)
            _check_live_rows(h, want, n_sel, d, dl, form, (d, split, prec, rm is not None))
            if im is not None:
                assert (h[1] == 0).all() and (h[4] == 0).all()                      # idx < 0, idx >= width: a row of zeros, every block
        xf = rk._rows(n_seq * width, d, 1)
        gf, bf = rk._affine(d, 2)
        assert np.array_equal(_gather_ln_live(xf, idx, row_map, P, width, gf, bf, n_sel, split, prec, d),
                              rk.gather_ln(xf, idx, row_map, P, width, gf, bf, n_sel, split, prec))


def _lm_tail_live(g, e, bias, gb, dl):
    n, vocab = g.shape[0], e.shape[0]
    out = np.full((n, vocab), np.nan, dtype=F32)
    k = ctypes.c_int(-1)
    _lib.check(_lib.lib().pg_embedded_lm_tail(0, _p(g), _p(gb[0]) if gb else None, _p(gb[1]) if gb else None, _p(e), _p(bias), _p(out), n,
                                              g.shape[1], vocab, rk.EPS, ctypes.byref(k), dl))
    return out, k.value


@pytest.mark.parametrize("M, d, dl", LIVE_CASES)
def test_live_lm_tail_on_both_kernels(M, d, dl):
    """1 and 300 rows: the workgroup-per-row kernel; 1025 rows: the row-per-wave kernel (the switch is at 1024 rows)"""
    for n in (1, 300, 1025):
        gl, el, bias, gbl = rk._tail_input(n, dl, 33)
        g, e, gb = _padded(gl, d), _padded(el, d), (_padded(gbl[0], d), _padded(gbl[1], d))
        for with_ln in (1, 0):
            want, small = rk.lm_tail(gl, el, bias, gbl if with_ln else None)
            got, small_live = _lm_tail_live(g, e, bias, gb if with_ln else None, dl)
            assert small == small_live == (1 if n <= 1024 else 0)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n, d, dl, with_ln)
        gf, ef, bias, gbf = rk._tail_input(n, d, 33)
        assert np.array_equal(_lm_tail_live(gf, ef, bias, gbf, d)[0].view(np.uint32), rk.lm_tail(gf, ef, bias, gbf)[0].view(np.uint32))


def _embed_live(tok, e, gb2, dropout, prec, dl):
    n_seq, T = tok.shape
    d = e.shape[1]
    x = np.full((n_seq * T, d), np.nan, dtype=F32)
    h2 = np.full((n_seq * T, d), rk.FILL, dtype=np.uint16)
    _lib.check(_lib.lib().pg_embedded_embed_rows(0, prec, _p(tok), n_seq, T, _p(e), e.shape[0], d, None, 0, None, 0, None, None, _p(gb2[0]),
                                            _p(gb2[1]), rr.PAD, rr.MASK, int(dropout), rk.EPS, 1.0, _p(x), _p(h2), dl))
    return x, h2


@pytest.mark.parametrize("M, d, dl", LIVE_CASES)
def test_live_embedding_and_its_fused_first_layernorm(M, d, dl):
    has_pos, ln_before, dropout, scaled, rows_per_msa = rk.EMBED_MODELS["esm2"]
    rng = np.random.default_rng(d)
    el = (rng.standard_normal((rk.V, dl), dtype=F32) * F32(0.3)).astype(F32)
    el[:, 0] += np.arange(rk.V, dtype=F32)
    e = _padded(el, d, 0.0)                                                         # the table's pad columns are zeros, as the engine's
    gb2l = rk._affine(dl, dl + 6)
    gb2 = (_padded(gb2l[0], d), _padded(gb2l[1], d))
    for i, (n_seq, T) in enumerate([(1, 1), (3, 27), (2, 65)]):
        for j, pattern in enumerate(rr.PATTERNS):
            tok = rr.make_tokens(pattern, n_seq, T, seed=T * 10 + j)
            prec = (rk.BF16, rk.F16)[(i + j) % 2]
            xw, hw = rk.embed(tok, el, None, None, 0, None, gb2l, dropout, 1.0, prec)
            x, h2 = _embed_live(tok, e, gb2, dropout, prec, dl)
            case = (d, dl, n_seq, T, pattern)
            assert np.array_equal(x[:, :dl].view(np.uint32), xw.view(np.uint32)) and (x[:, dl:] == 0).all(), case
            assert np.array_equal(h2[:, :dl], hw) and (h2[:, dl:] == 0).all(), case
    ef = (rng.standard_normal((rk.V, d), dtype=F32) * F32(0.3)).astype(F32)
    gbf = rk._affine(d, 9)
    tok = rr.make_tokens(rr.PATTERNS[0], 3, 27, seed=4)
    a, b = _embed_live(tok, ef, gbf, dropout, rk.BF16, d), rk.embed(tok, ef, None, None, 0, None, gbf, dropout, 1.0, rk.BF16)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])
    gb = rk._affine(d, 5)                                                           # emb_layer_norm_before has no live-width form
    x = np.zeros((tok.size, d), F32)
    h2 = np.zeros((tok.size, d), np.uint16)
    rc = _lib.lib().pg_embedded_embed_rows(0, rk.BF16, _p(tok), 3, 27, _p(ef), rk.V, d, None, 0, None, 0, _p(gb[0]), _p(gb[1]), _p(gbf[0]), _p(gbf[1]),
                                      rr.PAD, rr.MASK, 1, rk.EPS, 1.0, _p(x), _p(h2), dl)
    assert rc == _lib.PG_ERR_INVALID and b"emb_layer_norm_before" in _lib.lib().pg_last_error()


# ---- refusals that stay ---------------------------------------------------------------------------------------------------------------
def test_pg_engine_create_still_names_the_built_widths_and_the_embedded_entry_is_esm2s():
    cfg = dict(weights.ESM2_T12_CONFIG)
    c = _lib.ModelConfig(**{k: cfg[k] for k, _ in _lib.ModelConfig._fields_})
    h = ctypes.c_void_p()
    L = _lib.lib()
    assert L.pg_engine_create(ctypes.byref(c), None, 0, 0, _lib.PG_PREC_BF16, ctypes.byref(h)) == _lib.PG_ERR_INVALID       # 480 / 20
    c.d_model, c.n_heads = 384, 16                                                                                          # heads of 24, a GEMM width
    assert L.pg_engine_create(ctypes.byref(c), None, 0, 0, _lib.PG_PREC_BF16, ctypes.byref(h)) == _lib.PG_ERR_INVALID
    assert b"head dim must be 64 (every architecture) or 32, 128, 16 (ESM-2 only)" in L.pg_last_error()
    c.d_model, c.n_heads, c.arch = 480, 20, _lib.PG_ARCH_ESM1B
    assert L.pg_engine_create_embedded(ctypes.byref(c), 32, None, 0, 0, _lib.PG_PREC_BF16, ctypes.byref(h)) == _lib.PG_ERR_INVALID
    assert b"PG_ARCH_ESM2 only" in L.pg_last_error()
    # a tensor of the wrong size is the loader's error, named
    cfg2, sd, _ = common.case("esm2_35m", d=96, d_ffn=256)
    sd = dict(sd)
    sd["layers.0.fc1.weight"] = sd["layers.0.fc1.weight"][:, :95].copy()
    with pytest.raises(Exception, match=r"layers\.0\.fc1\.weight.*expected 24576"):
        common.model(models.ESM2_35M, cfg2, sd, "bf16").model.to("cuda:0")


# ---- forward: the shared bodies (tests/_esm2_gpu_common.py) at this size ---------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SIZES["esm2_35m"]["forward"]["shapes"]))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_esm2_35m_forward_against_the_reference(precision, shape):
    common.check_forward("esm2_35m", shape, precision)


def test_esm2_35m_forward_against_huggingface_logits():
    common.check_huggingface_logits("hd24")
