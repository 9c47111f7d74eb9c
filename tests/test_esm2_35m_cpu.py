"""ESM-2 35M (esm2_t12_35M_UR50D: 20 heads of 24, d_model 480) on the host.  Heads of 24 are no kernel width: the engine runs the model
embedded, every head in a slot of 32 and its rows 640 wide (include/pgibbs.h pg_engine_create_embedded).  Here: the configuration and
the table of embedded widths, what loads against the configuration, the embedded entry's refusals (no device is needed to be
refused), the run-shape image of every tensor role -- live values exactly where the layout says, 0.0 everywhere else -- and the rotary
table; and, as shared bodies of tests/_esm2_cpu_common.py, the rotary frequencies for heads of 24, the refusal of a head-24 file by the
other sizes and the command-line model maps.  The v2 file's round trip and inv_freq check and models.ESM2_35M are the esm2_35m rows of
tests/test_esm2_sizes_cpu.py.  Needs no GPU."""
import ctypes

import numpy as np
import pytest

import _esm2_cpu_common as common
from protein_gibbs_sampler_amd import _lib, weights

W, SLOT = 24, 32


def test_t12_config_values_and_the_embedded_table():
    cfg = weights.ESM2_T12_CONFIG
    assert (cfg["arch"], cfg["d_model"], cfg["n_layers"], cfg["n_heads"], cfg["d_ffn"], cfg["vocab"]) == (_lib.PG_ARCH_ESM2, 480, 12, 20, 1920, 33)
    same = ("max_positions", "pad_idx", "mask_idx", "cls_idx", "eos_idx", "token_dropout", "max_msa_rows", "layer_norm_eps")
    assert all(cfg[k] == weights.ESM2_T33_CONFIG[k] for k in same)
    assert weights.head_dim_of(cfg) == W and W not in weights.HEAD_DIMS and W not in weights.HEAD_WIDTHS      # 24 is not a kernel width
    row = weights.EMBEDDED_WIDTHS[W]
    assert row["slot"] == SLOT and row["config"] is cfg and row["file"] == "esm2_t12_35M_UR50D"
    assert (row["wrapper"], row["cli"]) == ("ESM2_35M", "esm2_35m")
    assert np.float32(row["q_scale"]) == np.float32(24 ** -0.5) and row["q_scale"] != weights.HEAD_WIDTHS[32]["q_scale"]
    assert weights.embedded_slot(cfg) == SLOT and weights.embedded_slot(weights.ESM2_T30_CONFIG) == 0
    assert weights.embedded_slot(weights.ESM1B_CONFIG) == 0
    # heads of 24 under another base: that configuration does not say "embedded" and goes to pg_engine_create, which refuses it
    assert weights.embedded_slot(weights.make_config(weights.ESM2_T6_CONFIG, d_model=384, n_heads=16)) == 0
    assert weights.embedded_slot(weights.make_config(cfg, d_model=384, n_heads=16)) == SLOT
    assert weights.embedded_slot(weights.make_config(cfg, d_model=1280, n_heads=20)) == 0                      # heads of 64 loaded here
    assert weights.make_config(cfg, d_model=96, n_layers=2, d_ffn=256)["n_heads"] == 4                        # the base's head width


def test_t12_takes_the_35m_sizes_from_hyper_parameters_alone():
    cfg = weights.config_from_checkpoint_v2(dict(encoder_embed_dim=480, encoder_layers=12, encoder_attention_heads=20, token_dropout=True),
                                            [], weights.ESM2_T12_CONFIG)
    assert (cfg["d_model"], cfg["n_heads"], cfg["d_ffn"], cfg["n_layers"]) == (480, 20, 1920, 12)
    with pytest.raises(ValueError, match="33 heads of dimension 24.*at most 32"):                              # the slot's limit
        weights.config_from_checkpoint_v2(dict(encoder_embed_dim=33 * 24, encoder_layers=2, encoder_attention_heads=33), [], weights.ESM2_T12_CONFIG)
    with pytest.raises(ValueError, match="esm2_150m"):                                                         # heads of 32 load against t30 only
        weights.config_from_checkpoint_v2(dict(encoder_embed_dim=640, encoder_layers=2, encoder_attention_heads=20), [], weights.ESM2_T12_CONFIG)


# ---- the embedded entry: refused, or past every check, before a device is looked for ---------------------------------------------------
def _create(embedded, slot=SLOT, **over):
    cfg = weights.make_config(weights.ESM2_T12_CONFIG, **over)
    c = _lib.ModelConfig(**{k: cfg[k] for k, _ in _lib.ModelConfig._fields_})
    h = ctypes.c_void_p()
    L = _lib.lib()
    if embedded:
        rc = L.pg_engine_create_embedded(ctypes.byref(c), slot, None, 0, 0, _lib.PG_PREC_BF16, ctypes.byref(h))
    else:
        rc = L.pg_engine_create(ctypes.byref(c), None, 0, 0, _lib.PG_PREC_BF16, ctypes.byref(h))
    msg = L.pg_last_error().decode()
    if rc == _lib.PG_OK:                    # a machine with a GPU: the checks passed and the upload found no tensors
        L.pg_engine_destroy(h)
    return rc, msg


# no device -> PG_ERR_NO_DEVICE; with one the same call gets as far as the (empty) tensor list -> PG_ERR_WEIGHTS.  Either way every
# configuration check lies behind it
PAST_THE_CHECKS = (_lib.PG_ERR_NO_DEVICE, _lib.PG_ERR_WEIGHTS)


def test_embedded_entry_admits_heads_of_24_in_slots_of_32():
    if _lib.lib().pg_device_count() == 0:
        assert _create(True)[0] == _lib.PG_ERR_NO_DEVICE
        assert _create(True, d_model=32 * 24, n_heads=32)[0] == _lib.PG_ERR_NO_DEVICE
    assert _create(True)[0] in PAST_THE_CHECKS                                              # 480 / 20
    assert _create(True, d_model=32 * 24, n_heads=32)[0] in PAST_THE_CHECKS                 # 32 heads of 24: rows of 1024
    assert _create(True, d_model=96, n_heads=4, d_ffn=256)[0] in PAST_THE_CHECKS


def test_embedded_entry_refusals():
    rc, msg = _create(True, d_model=33 * 24, n_heads=33)
    assert rc == _lib.PG_ERR_INVALID and "at most 32" in msg, msg
    rc, msg = _create(True, slot=24)
    assert rc == _lib.PG_ERR_INVALID and "head slot 24" in msg and "64 or 32, 128, 16" in msg, msg
    rc, msg = _create(True, slot=48)
    assert rc == _lib.PG_ERR_INVALID and "head slot 48" in msg, msg
    rc, msg = _create(True, d_model=640, n_heads=20)                                        # live width 32 in slots of 32
    assert rc == _lib.PG_ERR_INVALID and "smaller than its slot" in msg, msg
    rc, msg = _create(True, d_model=20 * 23, n_heads=20)                                    # an odd width
    assert rc == _lib.PG_ERR_INVALID and "multiple of 4" in msg, msg
    rc, msg = _create(True, d_model=20 * 26, n_heads=20)                                    # even, no multiple of 4
    assert rc == _lib.PG_ERR_INVALID and "multiple of 4" in msg, msg
    for arch in (_lib.PG_ARCH_ESM1B, _lib.PG_ARCH_ESM1, _lib.PG_ARCH_MSA1B):
        rc, msg = _create(True, arch=arch)
        assert rc == _lib.PG_ERR_INVALID and "PG_ARCH_ESM2 only" in msg, msg
    rc, msg = _create(True, arch=_lib.PG_ARCH_ESM1B, slot=48)                                # the architecture is asked first
    assert rc == _lib.PG_ERR_INVALID and "PG_ARCH_ESM2 only" in msg, msg
    rc, msg = _create(True, d_ffn=1920 + 64)                                                # then the run shape's own rules
    assert rc == _lib.PG_ERR_INVALID and "d_ffn of 128" in msg, msg


def test_pg_engine_create_still_refuses_heads_of_24():
    rc, msg = _create(False)
    assert rc == _lib.PG_ERR_INVALID and "d_model must be a multiple of 64" in msg, msg
    rc, msg = _create(False, d_model=384, n_heads=16)                                       # heads of 24 at a width the GEMMs take
    assert rc == _lib.PG_ERR_INVALID and "head dim must be 64 (every architecture) or 32, 128, 16 (ESM-2 only)" in msg, msg


# ---- the run-shape images ----------------------------------------------------------------------------------------------------------------
def _head_col(c, w=W, slot=SLOT):
    """where feature c of the q / k / v axis goes: head h keeps its slot, the low half at 0 .., the high half at slot / 2 .."""
    h, j = divmod(c, w)
    return h * slot + (j if j < w // 2 else j + (slot - w) // 2)


def _image(name, a, H, f, V=33):
    D = H * SLOT
    run = {"embed_tokens.weight": (V, D), "lm_head.bias": (V,)}.get(name)
    if run is None:
        rows = f if ".fc1." in name else D
        cols = f if name.endswith("fc2.weight") else D
        run = (rows, cols) if name.endswith(".weight") and "layer_norm" not in name else (rows,)
    out = np.full(run, np.nan, np.float32)
    _lib.check(_lib.lib().pg_embedded_image(name.encode(), _lib.ptr(a), a.size, H, W, SLOT, f, V, _lib.ptr(out), out.size))
    return out


@pytest.mark.parametrize("H, f", [(2, 256), (20, 1920)])
def test_images_hold_the_live_values_at_their_places_and_zeros_elsewhere(H, f):
    d, V = H * W, 33
    rng = np.random.default_rng(H)
    stream = np.arange(d)                                        # a residual-stream feature keeps its column
    head = np.asarray([_head_col(c) for c in range(d)])
    assert head[:W].tolist() == list(range(12)) + list(range(16, 28)) and head[W] == SLOT and len(set(head)) == d
    same_f, same_v = np.arange(f), np.arange(V)
    p = "layers.1."
    roles = [("embed_tokens.weight", (V, d), same_v, stream), ("lm_head.bias", (V,), same_v, None),
             (p + "self_attn.q_proj.weight", (d, d), head, stream), (p + "self_attn.k_proj.weight", (d, d), head, stream),
             (p + "self_attn.v_proj.weight", (d, d), head, stream), (p + "self_attn.q_proj.bias", (d,), head, None),
             (p + "self_attn.k_proj.bias", (d,), head, None), (p + "self_attn.v_proj.bias", (d,), head, None),
             (p + "self_attn.out_proj.weight", (d, d), stream, head), (p + "self_attn.out_proj.bias", (d,), stream, None),
             (p + "fc1.weight", (f, d), same_f, stream), (p + "fc1.bias", (f,), same_f, None),
             (p + "fc2.weight", (d, f), stream, same_f), (p + "fc2.bias", (d,), stream, None),
             (p + "self_attn_layer_norm.weight", (d,), stream, None), (p + "self_attn_layer_norm.bias", (d,), stream, None),
             (p + "final_layer_norm.weight", (d,), stream, None), ("emb_layer_norm_after.bias", (d,), stream, None),
             ("lm_head.layer_norm.weight", (d,), stream, None), ("lm_head.dense.weight", (d, d), stream, stream),
             ("lm_head.dense.bias", (d,), stream, None)]
    for name, shape, rmap, cmap in roles:
        a = (rng.standard_normal(shape).astype(np.float32) + np.float32(3.0))            # no zero among the live values
        a[a == 0] = 1.0
        img = _image(name, a, H, f, V)
        want = np.zeros_like(img)
        if cmap is None:
            want[rmap] = a
        else:
            want[np.ix_(rmap, cmap)] = a
        assert np.array_equal(img, want) and not np.signbit(img[want == 0]).any(), name
        assert (img != 0).sum() == a.size, name


def test_image_entry_refusals():
    L = _lib.lib()
    a = np.ones((48, 48), np.float32)
    out = np.zeros((64, 64), np.float32)
    ok = lambda name, numel, n_out, w=W, slot=SLOT: L.pg_embedded_image(name, _lib.ptr(a), numel, 2, w, slot, 256, 33, _lib.ptr(out), n_out)
    assert ok(b"lm_head.dense.weight", 48 * 48, 64 * 64) == _lib.PG_OK
    assert ok(b"lm_head.dense.weight", 48 * 47, 64 * 64) == _lib.PG_ERR_INVALID and b"expected 2304" in L.pg_last_error()
    assert ok(b"lm_head.dense.weight", 48 * 48, 64 * 63) == _lib.PG_ERR_INVALID
    assert ok(b"embed_positions.weight", 48 * 48, 64 * 64) == _lib.PG_ERR_INVALID and b"not a tensor of an ESM-2 model" in L.pg_last_error()
    assert ok(b"lm_head.dense.weight", 48 * 48, 64 * 64, w=32) == _lib.PG_ERR_INVALID       # no room in the slot


# ---- the rotary table --------------------------------------------------------------------------------------------------------------------
def _table(rows, w, slot):
    t = np.full((rows, slot), np.nan, np.float32)
    _lib.check(_lib.lib().pg_embedded_rope_table(rows, w, slot, _lib.ptr(t)))
    return t


def test_rope_table_of_heads_of_24_in_slots_of_32():
    rows = 1026
    t = _table(rows, W, SLOT)
    ang = (np.arange(rows, dtype=np.float32)[:, None] * weights.rotary_inv_freq(W)[None, :]).astype(np.float32)      # the float32 angle ...
    cos, sin = np.cos(ang.astype(np.float64)).astype(np.float32), np.sin(ang.astype(np.float64)).astype(np.float32)   # ... in double
    # both sides are a double libm value rounded once to float32, magnitudes <= 1: within one float32 rounding of each other
    assert np.abs(t[:, :12] - cos).max() <= 2.0 ** -23 and np.abs(t[:, 16:28] - sin).max() <= 2.0 ** -23
    assert (t[:, 12:16] == 1.0).all() and (t[:, 28:32] == 0.0).all() and not np.signbit(t[:, 28:32]).any()
    assert np.array_equal(t[0], np.r_[np.ones(16), np.zeros(16)].astype(np.float32))
    # a built width in its own slot: the table of that width (no pad columns)
    t32 = _table(300, 32, 32)
    a32 = (np.arange(300, dtype=np.float32)[:, None] * weights.rotary_inv_freq(32)[None, :]).astype(np.float32)
    assert np.abs(t32[:, :16] - np.cos(a32.astype(np.float64)).astype(np.float32)).max() <= 2.0 ** -23
    assert np.abs(t32[:, 16:] - np.sin(a32.astype(np.float64)).astype(np.float32)).max() <= 2.0 ** -23
    assert _lib.lib().pg_embedded_rope_table(4, 25, 32, _lib.ptr(t)) == _lib.PG_ERR_INVALID


# ---- the live-width row entries on the host: what tests/test_dbg_entries_cpu.py holds for the entries they extend -----------------------
def _live_cases():
    z = lambda *s, dt=np.float32: np.zeros(s, dt)
    x, g, h16 = z(4, 64), z(64), z(4, 64, dt=np.uint16)
    return {
        "pg_embedded_embed_rows": ([0, _lib.PG_PREC_BF16, z(1, 16, dt=np.int32), 1, 16, z(33, 64), 33, 64, None, 0, None, 0, None, None, g, g,
                                    1, 32, 1, 1e-5, 1.0, z(16, 64), z(16, 64, dt=np.uint16), 48], 2, "pg_embedded_embed_rows: bad argument"),
        "pg_embedded_layernorm_rows": ([0, _lib.PG_PREC_BF16, x, g, g, h16, 4, 4, 64, 1e-5, 0, 0, 0, None, 48], 2, "pg_embedded_layernorm_rows: bad argument"),
        "pg_embedded_gather_ln": ([0, _lib.PG_PREC_BF16, z(16, 64), 16, np.asarray([0, 1, 2, 3], np.int32), None, 0, 1, 4, g, g, h16, 4, 4, 64, 1e-5,
                                   0, 48], 2, "pg_embedded_gather_ln: bad argument"),
        "pg_embedded_lm_tail": ([0, z(4, 64), None, None, z(33, 64), z(33), z(4, 33), 4, 64, 33, 1e-5, None, 48], 1, "pg_embedded_lm_tail: bad argument"),
    }


def _call(name, args):
    rc = getattr(_lib.lib(), name)(*[_lib.ptr(a) if isinstance(a, np.ndarray) else a for a in args])
    return rc, _lib.lib().pg_last_error().decode()


@pytest.mark.parametrize("name", sorted(_live_cases()))
def test_live_row_entries_refuse_on_the_host_and_compute_nothing_without_a_device(name):
    args, index, message = _live_cases()[name]
    assert _call(name, args[:index] + [None] + args[index + 1:]) == (_lib.PG_ERR_INVALID, message)
    for bad in (0, 50, 68, -4):                                                             # the live width: a multiple of 4 in 4 .. d
        rc, msg = _call(name, args[:-1] + [bad])
        assert rc == _lib.PG_ERR_INVALID and msg == name + ": the live width must be a multiple of 4, at most d", (name, bad, msg)
    if _lib.lib().pg_device_count() == 0:
        assert _call(name, args) == (_lib.PG_ERR_NO_DEVICE, "no HIP device visible")
        assert _call(name, args[:-1] + [64]) == (_lib.PG_ERR_NO_DEVICE, "no HIP device visible")


def test_live_row_entries_take_16_bit_modes_only():
    for name in ("pg_embedded_embed_rows", "pg_embedded_layernorm_rows", "pg_embedded_gather_ln"):
        args = _live_cases()[name][0]
        rc, msg = _call(name, args[:1] + [_lib.PG_PREC_FP32] + args[2:])
        assert rc == _lib.PG_ERR_INVALID and msg == name + ": precision must be PG_PREC_BF16 or PG_PREC_F16"


# ---- the shared bodies (tests/_esm2_cpu_common.py) at this size -------------------------------------------------------------------------
def test_inv_freq_24_is_torchs():
    common.check_inv_freq_is_torchs("esm2_35m")


@pytest.mark.parametrize("base", common.other_bases("esm2_35m"))
def test_heads_of_24_met_by_the_other_wrappers_name_esm2_35m(tmp_path_factory, base):
    common.check_met_by_another_size("esm2_35m", base, tmp_path_factory)


def test_command_lines_accept_esm2_35m():
    common.check_command_lines_accept("esm2_35m")
