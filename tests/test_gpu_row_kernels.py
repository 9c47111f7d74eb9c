"""The memory-bound row kernels of csrc/elementwise.hip on the MI355X, each through its own debug entry (include/pgibbs.h):
embed_ln_kernel, the plain / stride / column-major LayerNorm operand kernels, gather_ln_bf16_kernel, gather_rows_kernel and the two
LM-head tail kernels.

Bit-exact expectations come first: operand rows against the host loop of tests/_ln_host.py (ln_inplace and store_row_bf16 restated
operation for operation), one kernel against another where the code says "same bits", byte equality for the gathers.  Values that
only a sum order separates from the exact result are compared with float64 numpy (tests/_row_reference.py, itself checked against
the oracle in tests/test_row_kernels_cpu.py) under bounds derived from the number of float32 roundings.

Inputs are seeded, asymmetric and distinct per row.  PGIBBS_* switches are read once per process: the A/B runs are child processes."""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import _row_reference as rr
from _ln_host import PLAIN, SPLIT_DUP, SPLIT_NODUP, _ln_inplace_host, rows_not_from_host_loop, store_rows_host
from protein_gibbs_sampler_amd import _lib

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F32 = np.float32
BF16, F16 = _lib.PG_PREC_BF16, _lib.PG_PREC_F16
FILL = 0xA5C3                                   # what every output buffer holds before a launch: bf16 -2.6e-16, never a result
EPS = 1e-5
U = 2.0 ** -24                                  # unit roundoff of float32
KERNEL = {0: "plain", 1: "stride", 2: "colmajor"}
FORMS = [("bf16", BF16, PLAIN), ("fp16", F16, PLAIN), ("split", BF16, SPLIT_DUP), ("split-nodup", BF16, SPLIT_NODUP)]


def _p(a):
    return _lib.ptr(a) if a is not None else None


def _rows(n, d, seed, spread=3.0, shift=1.0):
    """n distinct rows: a mean and a last column that differ from row to row, so a shifted or swapped row cannot pass"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, d), dtype=F32) * F32(spread) + F32(shift)).astype(F32)
    x[:, 0] += np.arange(n, dtype=F32) * F32(0.01)
    x[:, -1] += F32(40.0)                        # the last chunk's last lane matters to the mean and the variance
    return x


def _affine(d, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(d, dtype=F32), rng.standard_normal(d, dtype=F32)


def ln_rows(x, g, b, form=PLAIN, prec=BF16, extra=3, R=0, C=0, M=None):
    """pg_dbg_layernorm_rows on x: (bits [M + extra][d or 3 d], the kernel the launcher chose); the buffer starts as FILL"""
    M = x.shape[0] if M is None else M
    d = x.shape[1]
    h = np.full((M + extra, d * (3 if form else 1)), FILL, dtype=np.uint16)
    k = ctypes.c_int(-1)
    _lib.check(_lib.lib().pg_dbg_layernorm_rows(0, prec, _p(x), _p(g), _p(b), _p(h), h.shape[0], M, d, EPS, form, R, C, ctypes.byref(k)))
    return h, KERNEL[k.value]


def _third_blocks(h, d):
    return h.reshape(h.shape[0], d // 32, 3, 32)[:, :, 2]


def _check_against_host_loop(h, x, g, b, form, prec, y0=None):
    """rows < M: store(ln_host(x)) with the root at 0 or +-1 ulp; rows >= M and, without the duplicate block, every third block: FILL"""
    M, d = x.shape
    assert (h[M:] == FILL).all(), "rows past M were written"
    if form == SPLIT_NODUP:
        assert (_third_blocks(h[:M], d) == FILL).all(), "the duplicate block was written"
    got = h[:M]
    if y0 is not None:                           # the correctly rounded root, computed once per input for all forms
        miss = np.flatnonzero((got != store_rows_host(y0, form, prec == F16, FILL)).any(axis=1))
        bad = miss[rows_not_from_host_loop(got[miss], x[miss], g, b, EPS, form, prec == F16, FILL)] if miss.size else miss
    else:
        bad = rows_not_from_host_loop(got, x, g, b, EPS, form, prec == F16, FILL)
    assert bad.size == 0, ("rows that differ from the host loop", bad[:10], bad.size)


# ---- LayerNorm operand rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [128, 640, 768, 1280, 2048, 2304, 2560])
@pytest.mark.parametrize("M", [1, 3, 37, 4099])
def test_operand_rows_equal_the_host_loop(M, d):
    x = _rows(M, d, M * 7 + d)
    g, b = _affine(d, d)
    y0 = _ln_inplace_host(x, g, b, EPS)
    for name, prec, form in FORMS:
        h, kernel = ln_rows(x, g, b, form, prec)
        assert kernel == "plain", (name, kernel)
        _check_against_host_loop(h, x, g, b, form, prec, y0)


# (M, the kernel of the default run): the stride kernel takes more than 8 and at most 32 workgroups per CU of the plain grid, 4 rows
# each -- on the MI355X's 256 CUs 8193 .. 32768 rows; 8192 and 32772 are the first row counts outside on either side
STRIDE_CASES = [(8192, "plain"), (8193, "stride"), (8448, "stride"), (16512, "stride"), (32768, "stride"), (32772, "plain")]
STRIDE_FORMS = [PLAIN, SPLIT_DUP, SPLIT_NODUP]


def _stride_input(d):
    return _rows(32772, d, 1000 + d), _affine(d, 2000 + d)


def _sample_rows(M):
    return np.unique(np.concatenate([np.arange(8), np.arange(M - 8, M), np.arange(0, M, 509)]))


def _stride_child(path):
    out = {}
    for d in (1280, 768):
        x_all, (g, b) = _stride_input(d)
        for M, _ in STRIDE_CASES:
            x = np.ascontiguousarray(x_all[:M])
            for form in STRIDE_FORMS:
                h, kernel = ln_rows(x, g, b, form, BF16, extra=1)
                key = "%d_%d_%d" % (d, M, form)
                out[key + "_kernel"] = np.array(kernel)
                out[key + "_digest"] = np.array(hashlib.blake2b(h.tobytes(), digest_size=16).hexdigest())
                out[key + "_rows"] = h[_sample_rows(M)].copy()
                out[key + "_past"] = h[M].copy()
    np.savez(path, **out)


def _run_child(fn, path, **switches):
    env = dict(os.environ)
    for k, v in switches.items():
        env.pop(k, None)
        if v is not None:
            env[k] = v
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_row_kernels as t; t.%s(%r)" % (ROOT, HERE, fn, path)
    p = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    return np.load(path)


def test_stride_kernel_gives_the_bits_of_the_plain_kernel(tmp_path):
    """layernorm_bf16_stride_kernel<1280 | 768> against layernorm_bf16_kernel on the same rows (PGIBBS_LN_STRIDE=0): every byte of
    the output equal, for all three forms, and the entry says which kernel ran -- a dispatch that stopped taking the stride kernel
    would otherwise compare the plain kernel with itself."""
    on = _run_child("_stride_child", str(tmp_path / "on.npz"), PGIBBS_LN_STRIDE=None)
    off = _run_child("_stride_child", str(tmp_path / "off.npz"), PGIBBS_LN_STRIDE="0")
    for d in (1280, 768):
        x_all, (g, b) = _stride_input(d)
        for M, kernel in STRIDE_CASES:
            rows = _sample_rows(M)
            x = np.ascontiguousarray(x_all[rows])
            y0 = _ln_inplace_host(x, g, b, EPS)
            for form in STRIDE_FORMS:
                key = "%d_%d_%d" % (d, M, form)
                assert str(on[key + "_kernel"]) == kernel and str(off[key + "_kernel"]) == "plain", (key, on[key + "_kernel"], off[key + "_kernel"])
                assert str(on[key + "_digest"]) == str(off[key + "_digest"]), key
                for run in (on, off):
                    h = np.concatenate([run[key + "_rows"], run[key + "_past"][None]])
                    _check_against_host_loop(h, x, g, b, form, BF16, y0)


@pytest.mark.parametrize("d", [768, 128])
@pytest.mark.parametrize("B,R,C", [(1, 1, 7), (2, 3, 20), (1, 32, 50), (2, 128, 9), (1, 17, 33)])
def test_column_major_rows(B, R, C, d):
    M = B * R * C
    x = _rows(M, d, M + d)
    g, b = _affine(d, d + 1)
    for prec in (BF16, F16):
        plain, k0 = ln_rows(x, g, b, PLAIN, prec)
        cm, k1 = ln_rows(x, g, b, PLAIN, prec, R=R, C=C)
        assert (k0, k1) == ("plain", "colmajor")
        _check_against_host_loop(plain, x, g, b, PLAIN, prec)
        bb, r, c = np.meshgrid(np.arange(B), np.arange(R), np.arange(C), indexing="ij")
        assert np.array_equal(cm[((bb * C + c) * R + r).ravel()], plain[((bb * R + r) * C + c).ravel()])
        assert (cm[M:] == FILL).all()


def test_column_major_refusals():
    """rows that are not whole MSAs, the split forms and the 10-chunk widths: refused, and nothing is written"""
    L = _lib.lib()
    h = np.full((24, 3 * 2304), FILL, dtype=np.uint16)
    for M, d, form, R, C in [(23, 768, PLAIN, 3, 4), (24, 768, SPLIT_DUP, 3, 4), (24, 768, SPLIT_NODUP, 3, 4), (8, 2304, PLAIN, 2, 4)]:
        x, g = np.zeros((M, d), F32), np.zeros(d, F32)
        assert L.pg_dbg_layernorm_rows(0, BF16, _p(x), _p(g), _p(g), _p(h), 24, M, d, EPS, form, R, C, None) == _lib.PG_ERR_INVALID
        assert b"column-major" in L.pg_last_error()
    assert (h == FILL).all()


# ---- the embedding ------------------------------------------------------------------------------------------------------------------
EMBED_SHAPES = [(1, 1), (3, 27), (2, 64), (2, 65), (5, 258), (1, 1022)]
V = 33
# (positions, LayerNorm before, token dropout, sqrt(d) scale, rows_per_msa)
EMBED_MODELS = {"esm1b": (True, True, True, False, 0), "esm1": (True, False, False, True, 0), "esm2": (False, False, True, False, 0),
                "msa1b-1": (True, True, False, False, 1), "msa1b-3": (True, True, False, False, 3), "msa1b-8": (True, True, False, False, 8)}


def embed(tok, e, pos, msa, rows_per_msa, gb, gb2, dropout, scale, prec):
    n_seq, T = tok.shape
    d = e.shape[1]
    x = np.full((n_seq * T, d), np.nan, dtype=F32)
    h2 = np.full((n_seq * T, d), FILL, dtype=np.uint16) if gb2 else None
    _lib.check(_lib.lib().pg_dbg_embed(0, prec, _p(tok), n_seq, T, _p(e), e.shape[0], d, _p(pos), 0 if pos is None else pos.shape[0],
                                       _p(msa), rows_per_msa, _p(gb[0]) if gb else None, _p(gb[1]) if gb else None,
                                       _p(gb2[0]) if gb2 else None, _p(gb2[1]) if gb2 else None, rr.PAD, rr.MASK, int(dropout), EPS,
                                       scale, _p(x), _p(h2)))
    return x, h2


@pytest.mark.parametrize("d", [128, 640, 1280, 2560])
@pytest.mark.parametrize("model", list(EMBED_MODELS))
def test_embedding(model, d):
    has_pos, ln_before, dropout, scaled, rows_per_msa = EMBED_MODELS[model]
    rng = np.random.default_rng(d + len(model))
    e = (rng.standard_normal((V, d), dtype=F32) * F32(0.3)).astype(F32)
    e[:, 0] += np.arange(V, dtype=F32)                                              # a row of its own per token
    pos = (rng.standard_normal((1022 + rr.PAD + 1, d), dtype=F32) * F32(0.2)).astype(F32) if has_pos else None
    if has_pos:
        pos[:, 1] += np.arange(pos.shape[0], dtype=F32) * F32(0.05)                 # ... and per position: one off is seen
    msa = (rng.standard_normal((rows_per_msa, d), dtype=F32) * F32(0.2) + np.arange(rows_per_msa, dtype=F32)[:, None]).astype(F32) if rows_per_msa else None
    gb = _affine(d, d + 5) if ln_before else None
    gb2 = _affine(d, d + 6)
    scale = float(F32(np.sqrt(F32(d)))) if scaled else 1.0
    for i, (n_seq, T) in enumerate(EMBED_SHAPES):
        for j, pattern in enumerate(rr.PATTERNS):
            tok = rr.make_tokens(pattern, n_seq, T, seed=T * 10 + j)
            prec = (BF16, F16)[(i + j) % 2]
            x, h2 = embed(tok, e, pos, msa, rows_per_msa, gb, gb2, dropout, scale, prec)
            want, mag = rr.embed_reference(tok, e, pos, msa, rows_per_msa, gb[0] if gb else None, gb[1] if gb else None,
                                           token_dropout=dropout, eps=EPS, embed_scale=F32(scale))
            want, mag = want.reshape(-1, d), mag.reshape(-1, d)
            pad = (tok == rr.PAD).ravel()
            case = (model, d, n_seq, T, pattern)
            assert (x[pad] == 0).all() and not np.signbit(x[pad]).any(), case
            if ln_before:       # the project's LayerNorm tolerance (test_gpu_kernels.py::test_layernorm)
                assert np.abs(x - want).max() < 2e-5 * max(1.0, np.abs(want).max()), (case, float(np.abs(x - want).max()))
            else:               # at most 7 float32 roundings (3 in the scale, 1 product, 2 adds, 1 for a contraction that may differ)
                worst = np.abs(x - want) - 8 * U * mag
                assert (worst <= 0).all(), (case, float(worst.max()))
            # h2 = the first layer's LayerNorm of the very row written: the operand kernel's bits on x, <pad> rows (x = 0) = beta2
            h, kernel = ln_rows(x, gb2[0], gb2[1], PLAIN, prec, extra=0)
            assert kernel == "plain" and np.array_equal(h2, h), case
            if pad.any():
                assert np.array_equal(h2[pad], np.broadcast_to(store_rows_host(gb2[1][None], PLAIN, prec == F16), h2[pad].shape)), case


# ---- gather + LayerNorm ---------------------------------------------------------------------------------------------------------------
SHADOW = 1 << 30


def gather_ln(x, idx, row_map, P, width, g, b, n_sel, split, prec=BF16, extra=2):
    d = x.shape[1]
    h = np.full((n_sel + extra, d * (3 if split else 1)), FILL, dtype=np.uint16)
    _lib.check(_lib.lib().pg_dbg_gather_ln(0, prec, _p(x), x.shape[0], _p(idx), _p(row_map), 0 if row_map is None else len(row_map), P,
                                           width, _p(g), _p(b), _p(h), h.shape[0], n_sel, d, EPS, int(split)))
    return h


def _index_case(rng, n_sel, P, width, n_seq, maps):
    """idx[n_sel] with every kind of entry (in range, shadowed, negative, past the width, shadowed past the width) and row_map"""
    S = (n_sel + P - 1) // P
    idx = rng.integers(0, width, n_sel).astype(np.int32)
    kind = rng.integers(0, 8, n_sel)
    kind[0] = 0 if n_sel == 1 else kind[0]
    idx[kind == 1] |= SHADOW
    idx[kind == 2] = -1 - rng.integers(0, 5, (kind == 2).sum()).astype(np.int32)
    idx[kind == 3] = width + rng.integers(0, 3, (kind == 3).sum()).astype(np.int32)
    idx[kind == 4] = (width + rng.integers(0, 3, (kind == 4).sum()).astype(np.int32)) | SHADOW
    if n_sel >= 7:
        idx[-1], idx[-2] = (width - 1) | SHADOW, width                          # the edges of the range, whatever was drawn
    row_map = {"none": None, "permutation": rng.permutation(n_seq)[:S].astype(np.int32) if S <= n_seq else None,
               "repeats": rng.integers(0, n_seq, S).astype(np.int32)}[maps]
    return idx, row_map


@pytest.mark.parametrize("d", [640, 1280, 2560])
@pytest.mark.parametrize("P", [1, 2, 5])
def test_gather_layernorm(d, P):
    width = 9                                    # 804 sequences at most: the source stays below the stride kernel's 8193 rows
    g, b = _affine(d, d + P)
    rng = np.random.default_rng(d * 10 + P)
    for n_sel in (1, 2, 7, 801):
        S = (n_sel + P - 1) // P
        n_seq = S + 3
        x = _rows(n_seq * width, d, n_sel + d)
        for split, prec in ((0, BF16), (1, BF16), (0, F16)):
            form = SPLIT_DUP if split else PLAIN
            want_all, kernel = ln_rows(x, g, b, form, prec, extra=0)                # the operand kernel on every source row
            assert kernel == "plain"
            for maps in ("none", "permutation", "repeats"):
                idx, row_map = _index_case(rng, n_sel, P, width, n_seq, maps)
                h = gather_ln(x, idx, row_map, P, width, g, b, n_sel, split, prec)
                case = (d, P, n_sel, split, prec, maps)
                pos = idx & 0x3fffffff
                zero = (idx < 0) | (pos >= width)
                s = np.arange(n_sel) // P
                src = (s if row_map is None else row_map[s]) * width + pos
                assert (h[:n_sel][zero] == 0).all(), case                           # every block of a split row too
                assert np.array_equal(h[:n_sel][~zero], want_all[src[~zero]]), case
                assert (h[n_sel:] == FILL).all(), case
                assert zero.any() or n_sel < 7, case
            # idx == NULL: selected row r is token row r
            h = gather_ln(x, None, None, P, width, g, b, n_sel, split, prec)
            assert np.array_equal(h[:n_sel], want_all[:n_sel]) and (h[n_sel:] == FILL).all(), (d, P, n_sel, split, prec)
    # the operand rows the gather was compared with are themselves the host loop's (all widths and heights: the first test)
    head = np.ascontiguousarray(x[:64])
    _check_against_host_loop(ln_rows(head, g, b, PLAIN, BF16, extra=0)[0], head, g, b, PLAIN, BF16)


# ---- plain row gather ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_bytes", [16, 1040, 2560, 5120, 10240])
@pytest.mark.parametrize("P", [1, 3])
def test_row_gather(row_bytes, P):
    width, n_sel = 19, 203
    S = (n_sel + P - 1) // P
    n_seq = S + 2
    rng = np.random.default_rng(row_bytes + P)
    src = rng.integers(0, 256, (n_seq * width, row_bytes), dtype=np.uint8)
    L = _lib.lib()
    for maps in ("none", "permutation", "repeats"):
        table = np.stack([_index_case(rng, n_sel, P, width, n_seq, "none")[0] for _ in range(4)])
        _, row_map = _index_case(rng, n_sel, P, width, n_seq, maps)
        for n_iters, it in ((0, 0), (4, 0), (4, 1), (4, 3)):
            idx = np.ascontiguousarray(table[it] if n_iters == 0 else table)
            dst = rng.integers(0, 256, (n_sel + 3, row_bytes), dtype=np.uint8)
            before = dst.copy()
            _lib.check(L.pg_dbg_gather_rows(0, _p(src), src.shape[0], _p(dst), dst.shape[0], _p(idx), n_iters, it, _p(row_map),
                                            0 if row_map is None else len(row_map), P, width, n_sel, row_bytes))
            now = table[it]
            pos = now & 0x3fffffff
            pos[(now < 0) | (pos >= width)] = 0                                      # negative and out-of-range: position 0 of the sequence
            s = np.arange(n_sel) // P
            rows = (s if row_map is None else row_map[s]) * width + pos
            case = (row_bytes, P, maps, n_iters, it)
            assert np.array_equal(dst[:n_sel], src[rows]), case
            assert np.array_equal(dst[n_sel:], before[n_sel:]), case
            assert ((now < 0).any() and (now & SHADOW).astype(bool).any()), case


# ---- the LM-head tail ---------------------------------------------------------------------------------------------------------------
TAIL_N = [1, 2, 5, 800, 1024, 1025, 4099]          # the small kernel up to 1024 rows, the row-per-wave kernel beyond
TAIL_V = [1, 4, 5, 33, 64]
TAIL_D = [128, 768, 1280, 2304, 2560]


def _tail_input(n, d, vocab):
    g = _rows(n, d, n * 3 + d, spread=1.0, shift=0.1)
    g[:, -1] -= F32(38.0)
    rng = np.random.default_rng(vocab * 7 + d)
    e = (rng.standard_normal((vocab, d), dtype=F32) * F32(0.3)).astype(F32)
    e[:, 0] += np.arange(vocab, dtype=F32) * F32(0.5)
    bias = rng.standard_normal(vocab, dtype=F32) + np.arange(vocab, dtype=F32)
    return g, e, bias, _affine(d, d + 9)


def lm_tail(g, e, bias, gb):
    n, vocab = g.shape[0], e.shape[0]
    out = np.full((n, vocab), np.nan, dtype=F32)
    k = ctypes.c_int(-1)
    _lib.check(_lib.lib().pg_dbg_lm_tail(0, _p(g), _p(gb[0]) if gb else None, _p(gb[1]) if gb else None, _p(e), _p(bias), _p(out), n,
                                         g.shape[1], vocab, EPS, ctypes.byref(k)))
    return out, k.value


def _tail_child(path):
    out = {}
    for n in TAIL_N:
        for d in TAIL_D:
            for vocab in TAIL_V:
                g, e, bias, gb = _tail_input(n, d, vocab)
                for with_ln in (0, 1):
                    logits, small = lm_tail(g, e, bias, gb if with_ln else None)
                    key = "%d_%d_%d_%d" % (n, d, vocab, with_ln)
                    out[key], out[key + "_small"] = logits, np.array(small)
    np.savez(path, **out)


def test_lm_tail_small_and_large_kernels(tmp_path):
    """lm_tail_small_kernel (default up to 1024 rows) against lm_tail_kernel on the same rows (PGIBBS_LM_TAIL_SMALL=0): the same bits;
    and both against float64.  Per logit a lane adds at most 10 chunk terms of 3 adds each, the butterfly 6 more, the bias 1: with
    the products' own roundings |err| <= 24 u (sum |v_i e_i| + |bias|); with the LayerNorm in front, its tolerance (2e-5 max(1,
    |ln|max) per value, test_layernorm) carried through the dot product on top."""
    on = _run_child("_tail_child", str(tmp_path / "on.npz"), PGIBBS_LM_TAIL_SMALL=None)
    off = _run_child("_tail_child", str(tmp_path / "off.npz"), PGIBBS_LM_TAIL_SMALL="0")
    worst = {0: 0.0, 1: 0.0}
    for n in TAIL_N:
        for d in TAIL_D:
            for vocab in TAIL_V:
                g, e, bias, gb = _tail_input(n, d, vocab)
                for with_ln in (0, 1):
                    key = "%d_%d_%d_%d" % (n, d, vocab, with_ln)
                    a, b = on[key], off[key]
                    assert int(on[key + "_small"]) == (1 if n <= 1024 else 0) and int(off[key + "_small"]) == 0, key
                    assert a.shape == (n, vocab) and np.isfinite(a).all(), key
                    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), key
                    want, mag, vmax, esum = rr.lm_tail_reference(g, e, bias, gb[0] if with_ln else None, gb[1] if with_ln else None, EPS)
                    bound = 24 * U * mag + (2e-5 * max(1.0, vmax) * esum[None, :] if with_ln else 0.0)
                    err = np.abs(a - want)
                    worst[with_ln] = max(worst[with_ln], float((err / bound).max()))
                    assert (err <= bound).all(), (key, float((err / bound).max()))
    print("\n[lm_tail] worst |err| / bound: %.3f without LayerNorm, %.3f with" % (worst[0], worst[1]))
