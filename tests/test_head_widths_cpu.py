"""The head-width table on both sides of the C ABI: weights.HEAD_WIDTHS (Python) against csrc/head_width.h as the engine, the rotary
entry and the attention entry apply it -- the same widths, the same head counts at the boundary (max accepted, max + 1 refused), the
same architectures, the same row widths above 2560 features, and the q scale.  Every refusal is decided on the host before a device is
looked for, so "accepted" reads PG_ERR_NO_DEVICE here: the module needs a machine WITHOUT a GPU."""
import ctypes
import re

import numpy as np
import pytest

from protein_gibbs_sampler_amd import _lib, weights

WIDTHS = sorted(weights.HEAD_WIDTHS)
OTHER_ARCHS = [_lib.PG_ARCH_ESM1B, _lib.PG_ARCH_MSA1B, _lib.PG_ARCH_ESM1]


@pytest.fixture(autouse=True)
def _no_gpu():
    if _lib.lib().pg_device_count() > 0:
        pytest.skip("GPU present")


def engine_create(d_model, n_heads, arch=_lib.PG_ARCH_ESM2):
    """-> (return code, message) of pg_engine_create for a one-layer configuration of that width"""
    L = _lib.lib()
    cfg = _lib.ModelConfig(arch=arch, vocab=33, d_model=d_model, n_layers=1, n_heads=n_heads, d_ffn=256, max_positions=32, pad_idx=1,
                           mask_idx=32, cls_idx=0, eos_idx=2, token_dropout=1, max_msa_rows=0, layer_norm_eps=1e-5)
    h = ctypes.c_void_p()
    rc = L.pg_engine_create(ctypes.byref(cfg), None, 0, 0, 0, ctypes.byref(h))
    assert not h.value
    return rc, L.pg_last_error().decode()


def rope(H, hd):
    L = _lib.lib()
    x = np.zeros((2, 3 * H * hd), np.float32)
    return L.pg_dbg_rope_hd(0, _lib.PG_PREC_BF16, _lib.ptr(x), 1, 2, H, hd), L.pg_last_error().decode()


def attention(H, hd):
    L = _lib.lib()
    x = np.zeros((2, 3 * H * hd), np.float32)
    y = np.zeros((2, H * hd), np.float32)
    return L.pg_dbg_attention_hd(0, _lib.PG_PREC_BF16, _lib.ptr(x), _lib.ptr(y), 1, 2, H, hd, None, -1), L.pg_last_error().decode()


def reader(d_model, n_heads, base):
    return weights.config_from_checkpoint_v2(dict(encoder_embed_dim=d_model, encoder_layers=2, encoder_attention_heads=n_heads), [], base)


@pytest.mark.parametrize("hd", WIDTHS)
def test_engine_takes_the_most_heads_of_a_width_and_refuses_one_more(hd):
    most = weights.HEAD_WIDTHS[hd]["max_heads"]
    rc, msg = engine_create(hd * most, most)
    assert rc == _lib.PG_ERR_NO_DEVICE, (rc, msg)
    rc, msg = engine_create(hd * (most + 1), most + 1)
    assert rc == _lib.PG_ERR_INVALID, (rc, msg)


@pytest.mark.parametrize("arch", OTHER_ARCHS)
@pytest.mark.parametrize("hd", WIDTHS)
def test_engine_runs_the_esm2_only_widths_for_esm2_only(hd, arch):
    row = weights.HEAD_WIDTHS[hd]
    rc, msg = engine_create(hd * row["max_heads"], row["max_heads"], arch)
    assert rc == (_lib.PG_ERR_INVALID if row["esm2_only"] else _lib.PG_ERR_NO_DEVICE), (rc, msg)


@pytest.mark.parametrize("hd", WIDTHS)
def test_rope_entry_takes_the_most_heads_of_a_width_and_refuses_one_more(hd):
    most = weights.HEAD_WIDTHS[hd]["max_heads"]
    assert rope(most, hd)[0] == _lib.PG_ERR_NO_DEVICE
    assert rope(most + 1, hd)[0] == _lib.PG_ERR_INVALID


@pytest.mark.parametrize("hd, heads", [(24, 8), (48, 4)])
def test_widths_that_are_not_built_are_refused_with_the_list_of_those_that_are(hd, heads):
    for rc, msg in (engine_create(hd * heads, heads), rope(heads, hd), attention(heads, hd)):
        assert rc == _lib.PG_ERR_INVALID, (rc, msg)
        for w in WIDTHS:
            assert re.search(r"\b%d\b" % w, msg.replace("d_model %d with %d heads" % (hd * heads, heads), "")), (w, msg)


@pytest.mark.parametrize("hd", WIDTHS)
def test_checkpoint_reader_takes_the_most_heads_of_a_width_and_refuses_one_more(hd):
    row = weights.HEAD_WIDTHS[hd]
    most = row["max_heads"]
    assert weights.head_dim_of(row["config"]) == hd
    cfg = reader(hd * most, most, row["config"])
    assert (cfg["d_model"], cfg["n_heads"]) == (hd * most, most)
    with pytest.raises(ValueError, match="%d heads of dimension %d.*at most %d" % (most + 1, hd, most)):
        reader(hd * (most + 1), most + 1, row["config"])


def test_rows_above_2560_features_come_in_units_of_512_on_both_sides():
    base = weights.HEAD_WIDTHS[128]["config"]
    rc, msg = engine_create(2688, 21)
    assert rc == _lib.PG_ERR_INVALID and "multiples of 512" in msg, (rc, msg)
    with pytest.raises(ValueError, match="multiples of 512"):
        reader(2688, 21, base)
    rc, msg = engine_create(3072, 24)
    assert rc == _lib.PG_ERR_NO_DEVICE, (rc, msg)
    assert reader(3072, 24, base)["d_model"] == 3072


@pytest.mark.parametrize("hd", WIDTHS)
def test_q_scale_is_the_float32_inverse_root_of_the_width(hd):
    """what the numpy references scale q by, float32(hd ** -0.5), is the literal the engine folds into W_q, bit for bit"""
    folded = np.float32(weights.HEAD_WIDTHS[hd]["q_scale"])
    assert folded.view(np.uint32) == np.float32(hd ** -0.5).view(np.uint32)
