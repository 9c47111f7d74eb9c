"""Without a GPU: (1) the float64 embedding reference that tests/test_gpu_row_kernels.py trusts (tests/_row_reference.py) reproduces
the oracle's three embeddings on synthetic weights and the shared token patterns; (2) the row-kernel debug entries of
include/pgibbs.h refuse, on the host and before they look for a device, every array the kernel would read out of bounds and every
shape the launchers refuse -- PG_ERR_INVALID and a message."""
import ctypes

import numpy as np
import pytest

import _row_reference as rr
from oracle import esm1_forward, esm_forward, msa_forward
from protein_gibbs_sampler_amd import _lib

F32 = np.float32
SHAPES = [(1, 1), (3, 27), (2, 64), (2, 65), (5, 258)]
U = 2.0 ** -24


def _close_sum(got, want, mag):
    """a sum of at most three float32 terms, each product rounded: the bound the GPU test uses for the forms without LayerNorm"""
    return (np.abs(got - want) <= 8 * U * mag).all()


def _close_ln(got, want):
    return np.abs(got - want).max() <= 2e-5 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("pattern", rr.PATTERNS)
@pytest.mark.parametrize("n_seq,T", SHAPES)
def test_reference_reproduces_the_esm1b_embedding(n_seq, T, pattern):
    cfg = esm_forward.EsmConfig(d_model=128, n_layers=1, n_heads=2, d_ffn=256, max_pos=300)
    w = esm_forward.synthetic_esm_weights(cfg, seed=3, std=0.05, embed_std=0.3, ln_jitter=0.1)
    tok = rr.make_tokens(pattern, n_seq, T, seed=n_seq * 1000 + T)
    want, pad = esm_forward.esm1b_embed(w, cfg, tok)
    got, _ = rr.embed_reference(tok, w["embed_tokens.weight"], w["embed_positions.weight"], gamma=w["emb_layer_norm_before.weight"],
                                beta=w["emb_layer_norm_before.bias"], token_dropout=True)
    assert got.shape == want.shape and _close_ln(want, got)
    assert (got[pad] == 0).all() and (want[pad] == 0).all()


@pytest.mark.parametrize("pattern", rr.PATTERNS)
@pytest.mark.parametrize("n_seq,T", SHAPES)
def test_reference_reproduces_the_esm1_embedding(n_seq, T, pattern):
    cfg = esm1_forward.Esm1Config(d_model=128, n_layers=1, n_heads=2, d_ffn=256, max_pos=300)
    w = esm1_forward.synthetic_esm1_weights(cfg, seed=4, std=0.05, embed_std=0.3, ln_jitter=0.1)
    tok = rr.make_tokens(pattern, n_seq, T, seed=n_seq * 1000 + T, mask=cfg.mask_idx)
    want, pad = esm1_forward.esm1_embed(w, cfg, tok)
    table = esm1_forward.sinusoidal_table(cfg.pad_idx + 1 + T, cfg.d_model, cfg.pad_idx)
    got, mag = rr.embed_reference(tok, w["embed_tokens.weight"], table, mask=cfg.mask_idx, embed_scale=F32(np.sqrt(F32(cfg.d_model))))
    assert got.shape == want.shape and _close_sum(want, got, mag)
    assert (got[pad] == 0).all()


@pytest.mark.parametrize("pattern", rr.PATTERNS)
@pytest.mark.parametrize("B,R,C", [(1, 1, 1), (2, 3, 27), (1, 8, 65), (2, 5, 64)])
def test_reference_reproduces_the_msa_embedding(B, R, C, pattern):
    cfg = msa_forward.MsaConfig(d_model=128, n_layers=1, n_heads=2, d_ffn=256, max_pos=300, max_rows=16)
    w = msa_forward.synthetic_msa_weights(cfg, seed=5, std=0.05, embed_std=0.3, ln_jitter=0.1)
    tok = rr.make_tokens(pattern, B * R, C, seed=R * 1000 + C).reshape(B, R, C)
    want = msa_forward.msa_embed(w, cfg, tok)
    got, _ = rr.embed_reference(tok.reshape(B * R, C), w["embed_tokens.weight"], w["embed_positions.weight"],
                                w["msa_position_embedding"].reshape(-1, cfg.d_model)[:R], R, w["emb_layer_norm_before.weight"],
                                w["emb_layer_norm_before.bias"])
    assert _close_ln(want.reshape(B * R, C, -1), got)


def test_token_patterns_hold_what_their_names_say():
    for n_seq, T in SHAPES + [(1, 1022)]:
        seen = {}
        for pattern in rr.PATTERNS:
            tok = rr.make_tokens(pattern, n_seq, T, seed=1)
            live, masked = tok != rr.PAD, tok == rr.MASK
            assert live.any(1).all() and (masked.sum(1) < live.sum(1)).all(), (pattern, n_seq, T)     # the division stays defined
            seen[pattern] = tok
        if T < 9:
            continue
        assert not (seen["no_pad"] == rr.PAD).any() and not (seen["no_mask"] == rr.MASK).any()
        lens = (seen["right_pad"] != rr.PAD).sum(1)
        assert (lens < T).all() and (n_seq == 1 or len(set(lens)) > 1)
        inner = seen["interior_pad"]
        assert (inner[:, T // 2] == rr.PAD).all() and (inner[:, T // 2 + 1] != rr.PAD).all() and (inner[:, 0] != rr.PAD).all()
        assert (seen["leading_pad"][:, 0] == rr.PAD).all()
        half = seen["half_masked"]
        assert (np.abs(2 * (half == rr.MASK).sum(1) - (half != rr.PAD).sum(1)) <= 1).all()
        near = seen["mask_next_to_pad"]
        assert (near[:, T // 2] == rr.PAD).all() and (near[:, T // 2 - 1] == rr.MASK).all() and (near[:, T // 2 + 1] == rr.MASK).all()


# ---- the debug entries' refusals ----------------------------------------------------------------------------------------------------
BF16, F16 = _lib.PG_PREC_BF16, _lib.PG_PREC_F16


def _refused(rc, *words):
    msg = _lib.lib().pg_last_error().decode()
    assert rc == _lib.PG_ERR_INVALID, (rc, msg)
    assert msg and all(w in msg for w in words), msg


def _embed(tok, V=33, d=128, pos_rows=40, **kw):
    n_seq, T = tok.shape
    e = np.zeros((V, d), F32)
    pos = np.zeros((pos_rows, d), F32)
    x = np.zeros((n_seq * T, d), F32)
    a = dict(precision=BF16, pos=pos)
    a.update(kw)
    return _lib.lib().pg_dbg_embed(0, a["precision"], _lib.ptr(tok), n_seq, T, _lib.ptr(e), V, d,
                                   _lib.ptr(a["pos"]) if a["pos"] is not None else None, pos_rows, None, 0, None, None, None, None,
                                   rr.PAD, rr.MASK, 1, 1e-5, 1.0, _lib.ptr(x), None)


def test_embed_entry_refuses_what_the_kernel_would_read_out_of_bounds():
    tok = rr.make_tokens("right_pad", 2, 20, seed=0)
    bad = tok.copy()
    bad[1, 3] = 33
    _refused(_embed(bad), "token 33", "33 rows")
    bad[1, 3] = -1
    _refused(_embed(bad), "token -1")
    # 20 non-pad tokens end at position row 20 + pad_idx = 21: a table of 21 rows is one short, and only for the sequence that is full
    full = rr.make_tokens("no_pad", 2, 20, seed=0)
    _refused(_embed(full, pos_rows=21), "position row 21", "21 rows")
    _refused(_embed(tok, d=130), "multiple of 4")
    _refused(_embed(tok, d=2564), "2560")
    _refused(_embed(tok, precision=_lib.PG_PREC_FP32), "precision")


def _ln_rows(M, d, form=0, R=0, C=0, precision=BF16, h_rows=None):
    x = np.zeros((M, d), F32)
    g = np.zeros(d, F32)
    h = np.zeros((h_rows if h_rows is not None else M, d * (3 if form else 1)), np.uint16)
    k = ctypes.c_int(-1)
    return _lib.lib().pg_dbg_layernorm_rows(0, precision, _lib.ptr(x), _lib.ptr(g), _lib.ptr(g), _lib.ptr(h), h.shape[0], M, d, 1e-5,
                                            form, R, C, ctypes.byref(k))


def test_layernorm_rows_entry_refusals():
    _refused(_ln_rows(12, 768, form=1, R=3, C=4), "column-major", "plain")
    _refused(_ln_rows(12, 768, form=2, R=3, C=4), "column-major", "plain")
    _refused(_ln_rows(13, 768, R=3, C=4), "whole MSAs")
    _refused(_ln_rows(12, 2304, R=3, C=4), "2048")
    _refused(_ln_rows(4, 2564), "2560")
    _refused(_ln_rows(4, 130), "multiple of 4")
    _refused(_ln_rows(4, 768, form=1, precision=F16), "bf16")
    _refused(_ln_rows(4, 768, h_rows=3), "bad argument")
    _refused(_ln_rows(4, 768, form=3), "bad argument")


def _gather_ln(idx, row_map=None, x_rows=40, P=1, width=10, d=128, split=0, n_sel=None):
    x = np.zeros((x_rows, d), F32)
    g = np.zeros(d, F32)
    n_sel = n_sel if n_sel is not None else len(idx)
    h = np.zeros((n_sel, d * (3 if split else 1)), np.uint16)
    return _lib.lib().pg_dbg_gather_ln(0, BF16, _lib.ptr(x), x_rows, _lib.ptr(idx) if idx is not None else None,
                                       _lib.ptr(row_map) if row_map is not None else None, 0 if row_map is None else len(row_map), P, width,
                                       _lib.ptr(g), _lib.ptr(g), _lib.ptr(h), n_sel, n_sel, d, 1e-5, split)


def _gather_rows(idx, row_map=None, src_rows=40, P=1, width=10, row_bytes=16, n_iters=0, it=0, n_sel=None):
    src = np.zeros((src_rows, row_bytes), np.uint8)
    n_sel = n_sel if n_sel is not None else idx.shape[-1]
    dst = np.zeros((n_sel, row_bytes), np.uint8)
    return _lib.lib().pg_dbg_gather_rows(0, _lib.ptr(src), src_rows, _lib.ptr(dst), n_sel, _lib.ptr(idx), n_iters, it,
                                         _lib.ptr(row_map) if row_map is not None else None, 0 if row_map is None else len(row_map), P, width,
                                         n_sel, row_bytes)


def test_gather_entries_refuse_rows_past_the_source():
    i32 = lambda *v: np.asarray(v, dtype=np.int32)
    # 5 selected sequences x width 10 = token rows 0 .. 49 of a source that has 40
    _refused(_gather_ln(i32(0, 1, 2, 3, 4)), "source row 44", "of 40")
    _refused(_gather_rows(i32(0, 1, 2, 3, 4)), "source row 44", "of 40")
    _refused(_gather_ln(i32(0, 1), row_map=i32(3, 4)), "source row 41")
    _refused(_gather_rows(i32(0, 1), row_map=i32(3, 4)), "source row 41")
    _refused(_gather_ln(i32(0, 1), row_map=i32(3, -1)), "source row")
    _refused(_gather_ln(i32(0, 1, 2), row_map=i32(0, 1)), "row_map is shorter")
    _refused(_gather_rows(i32(0, 1, 2), row_map=i32(0, 1)), "row_map is shorter")
    _refused(_gather_ln(None, n_sel=41), "more selected rows")
    # an out-of-range position is zeros (gather + LayerNorm) or position 0 (row gather), not a read: only the row matters; with the
    # shadow bit the position is what is left without it
    _refused(_gather_ln(i32(0, 1, 2, 3, 9 | (1 << 30))), "source row 49")
    _refused(_gather_rows(i32(0, 1, 2, 3, 77)), "source row 40")
    # the iteration table: only the row of the iteration the kernel reads is checked -- and it is
    table = np.zeros((4, 5), np.int32)
    table[2, 4] = 3
    _refused(_gather_rows(table, n_iters=4, it=2, src_rows=41), "source row 43")
    _refused(_gather_rows(table, n_iters=4, it=4), "bad argument")
    _refused(_gather_rows(i32(0, 1), row_bytes=24), "16 bytes")
    _refused(_gather_ln(i32(0, 1), d=2564), "2560")
    _refused(_gather_ln(i32(0, 1), d=130), "multiple of 4")


def test_lm_tail_entry_refusals():
    def run(n=2, d=128, V=33):
        g = np.zeros((n, d), F32)
        e = np.zeros((V, d), F32)
        b = np.zeros(V, F32)
        out = np.zeros((n, V), F32)
        k = ctypes.c_int(-1)
        return _lib.lib().pg_dbg_lm_tail(0, _lib.ptr(g), None, None, _lib.ptr(e), _lib.ptr(b), _lib.ptr(out), n, d, V, 1e-5, ctypes.byref(k))
    _refused(run(V=65), "1..64")
    _refused(run(V=0), "1..64")
    _refused(run(d=130), "multiple of 4")
    _refused(run(d=2564), "2560")
