"""Model configurations, synthetic weights and checkpoint reading.

The reference obtains weights by `esm.pretrained.<name>()` (/root/reference/src/pgen/models.py:61-86),
which downloads fair-esm checkpoints.  There is no network here, so:
  * `synthetic_state_dict` builds a seeded random state dict with fair-esm's key names and shapes
     -- throughput does not depend on weight values;
  * `load_fair_esm_checkpoint` reads a real fair-esm `.pt` file when one is supplied, applying the
    same prefix stripping fair-esm applies, so real ESM-1b / MSA-1b weights can drive the engine.
"""
import os
import re

import numpy as np

from . import _lib

ESM1B_CONFIG = dict(arch=_lib.PG_ARCH_ESM1B, vocab=33, d_model=1280, n_layers=33, n_heads=20, d_ffn=5120, max_positions=1024,
                    pad_idx=1, mask_idx=32, cls_idx=0, eos_idx=2, token_dropout=1, max_msa_rows=0, layer_norm_eps=1e-5)
MSA1B_CONFIG = dict(arch=_lib.PG_ARCH_MSA1B, vocab=33, d_model=768, n_layers=12, n_heads=12, d_ffn=3072, max_positions=1024,
                    pad_idx=1, mask_idx=32, cls_idx=0, eos_idx=2, token_dropout=0, max_msa_rows=1024, layer_norm_eps=1e-5)


# ESM-1 (fair-esm "protein_bert_base": esm1_t6_43M / t12_85M / t34_670M_UR50S -- pgen.models.ESM6 / ESM12 / ESM34): sqrt(d) embedding
# scale, sinusoidal positions, no emb_layer_norm_before / after, bias_k / bias_v, LayerNorm eps 1e-12, untied embed_out, no token
# dropout, the 35-token "ESM-1" alphabet (include/pgibbs.h PG_ARCH_ESM1)
ESM1_T6_CONFIG = dict(arch=_lib.PG_ARCH_ESM1, vocab=35, d_model=768, n_layers=6, n_heads=12, d_ffn=3072, max_positions=1024,
                      pad_idx=1, mask_idx=33, cls_idx=32, eos_idx=2, token_dropout=0, max_msa_rows=0, layer_norm_eps=1e-12)
ESM1_T12_CONFIG = dict(ESM1_T6_CONFIG, n_layers=12)
ESM1_T34_CONFIG = dict(ESM1_T6_CONFIG, n_layers=34, d_model=1280, n_heads=20, d_ffn=5120)


# ESM-2 (fair-esm `ESM2`, esm2_t33_650M_UR50D -- models.ESM2): the ESM-1b block stack and LM head without a position table and without
# emb_layer_norm_before; positions enter through rotary embeddings of q and k in every layer (include/pgibbs.h PG_ARCH_ESM2).  Of
# the released sizes 650M and 3B have heads of 64, 150M heads of 32, 15B heads of 128 and 8M heads of 16, the four widths the attention
# and rotary kernels are built for.  35M has heads of 24 and d_model 480, which neither those kernels nor the GEMMs (multiples of 64) take:
# it runs EMBEDDED, every head in a slot of 32 and its rows 640 wide (EMBEDDED_WIDTHS below; include/pgibbs.h pg_engine_create_embedded).
ESM2_T33_CONFIG = dict(arch=_lib.PG_ARCH_ESM2, vocab=33, d_model=1280, n_layers=33, n_heads=20, d_ffn=5120, max_positions=1024,
                       pad_idx=1, mask_idx=32, cls_idx=0, eos_idx=2, token_dropout=1, max_msa_rows=0, layer_norm_eps=1e-5)
# esm2_t36_3B_UR50D -- models.ESM2_3B: 36 layers of 40 heads, 4.4 times the arithmetic of the 650M model per token
ESM2_T36_CONFIG = dict(ESM2_T33_CONFIG, d_model=2560, n_layers=36, n_heads=40, d_ffn=10240)
# esm2_t30_150M_UR50D -- models.ESM2_150M: 30 layers of 20 heads of 32; a quarter of the 650M model's GEMM work per token
ESM2_T30_CONFIG = dict(ESM2_T33_CONFIG, d_model=640, n_layers=30, n_heads=20, d_ffn=2560)
# esm2_t48_15B_UR50D -- models.ESM2_15B: 48 layers of 40 heads of 128; about 30 GB of 16-bit weights
ESM2_T48_CONFIG = dict(ESM2_T33_CONFIG, d_model=5120, n_layers=48, n_heads=40, d_ffn=20480)
# esm2_t6_8M_UR50D -- models.ESM2_8M: 6 layers of 20 heads of 16
ESM2_T6_CONFIG = dict(ESM2_T33_CONFIG, d_model=320, n_layers=6, n_heads=20, d_ffn=1280)
# esm2_t12_35M_UR50D -- models.ESM2_35M: 12 layers of 20 heads of 24.  head_slot is the configuration's own say that its heads run embedded
# in slots of that width (not a field of pg_model_config): a configuration derived from this one keeps it, one derived from another
# base with heads of 24 does not have it and stays refused by pg_engine_create
ESM2_T12_CONFIG = dict(ESM2_T33_CONFIG, d_model=480, n_layers=12, n_heads=20, d_ffn=1920, head_slot=32)
# The released sizes under their --model names: configuration, checkpoint file (without ".pt") and wrapper (models.*).  Head width and
# slot follow from the configuration (head_dim_of, embedded_slot); models.ESM2_MODELS and tools/esm2_bench.py read this table
ESM2_SIZES = {cli: dict(config=config, file=file, wrapper=wrapper, cli=cli) for cli, config, file, wrapper in (
    ("esm2", ESM2_T33_CONFIG, "esm2_t33_650M_UR50D", "ESM2"), ("esm2_3b", ESM2_T36_CONFIG, "esm2_t36_3B_UR50D", "ESM2_3B"),
    ("esm2_150m", ESM2_T30_CONFIG, "esm2_t30_150M_UR50D", "ESM2_150M"), ("esm2_15b", ESM2_T48_CONFIG, "esm2_t48_15B_UR50D", "ESM2_15B"),
    ("esm2_8m", ESM2_T6_CONFIG, "esm2_t6_8M_UR50D", "ESM2_8M"), ("esm2_35m", ESM2_T12_CONFIG, "esm2_t12_35M_UR50D", "ESM2_35M"))}
# The head widths the attention and rotary kernels are built for, row for row the table of csrc/head_width.h (tests/test_head_widths_cpu.py
# holds the two together): at most max_heads heads per row, for ESM-2 only or every architecture, q scaled by q_scale = width^-0.5 as
# float32; then the released size that needs the width at its widest -- its row of ESM2_SIZES (config, file, wrapper, cli)
HEAD_WIDTHS = {
    64: dict(max_heads=40, esm2_only=False, q_scale=0.125, **ESM2_SIZES["esm2_3b"]),
    32: dict(max_heads=32, esm2_only=True, q_scale=0.17677669529663687, **ESM2_SIZES["esm2_150m"]),
    128: dict(max_heads=40, esm2_only=True, q_scale=0.08838834764831845, **ESM2_SIZES["esm2_15b"]),
    16: dict(max_heads=32, esm2_only=True, q_scale=0.25, **ESM2_SIZES["esm2_8m"]),
}
HEAD_DIMS = tuple(HEAD_WIDTHS)
# Head widths that are no kernel width and run embedded in a slot of one (csrc/engine.hip init_embedded): the engine runs n_heads * slot
# features per row on zero-padded weights and scales q by q_scale = width^-0.5 as float32, the width's own
EMBEDDED_WIDTHS = {
    24: dict(slot=32, q_scale=float(np.float32(24 ** -0.5)), **ESM2_SIZES["esm2_35m"]),
}


def embedded_slot(cfg):
    """The slot width an ESM-2 configuration says its heads run embedded in (its head_slot, for a width of EMBEDDED_WIDTHS); 0: the
    configuration goes to pg_engine_create as it is."""
    row = EMBEDDED_WIDTHS.get(head_dim_of(cfg)) if cfg["arch"] == _lib.PG_ARCH_ESM2 else None
    return row["slot"] if row and cfg.get("head_slot") == row["slot"] else 0


MAX_HEADS_OF_32 = HEAD_WIDTHS[32]["max_heads"]
MAX_HEADS_OF_16 = HEAD_WIDTHS[16]["max_heads"]
MAX_HEADS_OF_128 = HEAD_WIDTHS[128]["max_heads"]
MAX_D_MODEL = 64 * HEAD_WIDTHS[64]["max_heads"]  # the row kernels hold at most kMaxChWide * 256 = 2560 features (csrc/ln_row.h) ...
MAX_D_MODEL_HD128 = 128 * MAX_HEADS_OF_128       # ... or, above them, whole 512-feature units up to kMaxCh5k * 256 = 5120: heads of 128
ESM2_650M_MAX_D_MODEL = 2048  # a wider file handed to a config of at most this width (models.ESM2) is refused: see below


def rotary_inv_freq(head_dim=64):
    """fair-esm RotaryEmbedding's `inv_freq` for heads of `head_dim` (64: the default; 32: ESM-2 150M; 128: ESM-2 15B; 16: ESM-2 8M; 24: ESM-2
    35M), float32:
    1.0 / (10000 ** (torch.arange(0, head_dim, 2).float() / head_dim)).  The power is taken in double and rounded to float32 -- the
    values torch's float32 pow gives (numpy's vectorised float32 power is one ulp off at i = 5 and 27 of 32), and what the engine
    builds its cos / sin table from (csrc/engine.hip rope_table)."""
    # the exponent is torch's float32 quotient: exact when head_dim is a power of two, rounded at 24 (i / 12 is no float32 value)
    e = (np.arange(0, head_dim, 2, dtype=np.float32) / np.float32(head_dim)).astype(np.float32)
    p = (10000.0 ** e.astype(np.float64)).astype(np.float32)
    return (np.float32(1.0) / p).astype(np.float32)


def head_dim_of(cfg):
    """d_model / n_heads of a configuration (0 when it does not divide)."""
    return cfg["d_model"] // cfg["n_heads"] if cfg["n_heads"] > 0 and cfg["d_model"] % cfg["n_heads"] == 0 else 0


def sinusoidal_positions(n_rows, d, pad_idx):
    """fairseq / fair-esm SinusoidalPositionalEmbedding.get_embedding in float32 ([sin | cos] halves, inv_freq =
    exp(-i log(10000) / (d/2 - 1)), padding row zero): the engine reads it as its `embed_positions.weight` table."""
    half = d // 2
    step = np.float32(np.log(10000.0) / (half - 1))
    inv = np.exp(np.arange(half, dtype=np.float32) * -step).astype(np.float32)
    ang = (np.arange(n_rows, dtype=np.float32)[:, None] * inv[None, :]).astype(np.float32)
    emb = np.concatenate([np.sin(ang), np.cos(ang)], axis=1).astype(np.float32)
    if d % 2:
        emb = np.concatenate([emb, np.zeros((n_rows, 1), np.float32)], axis=1)
    emb[pad_idx] = 0
    return emb


def make_config(base, **overrides):
    cfg = dict(base)
    cfg.update(overrides)
    if "n_heads" not in overrides and "d_model" in overrides:
        cfg["n_heads"] = cfg["d_model"] // (head_dim_of(base) or 64)      # the base configuration's head width (64 but for ESM-2 150M)
    return cfg


def tensor_shapes(cfg):
    """name -> shape for every tensor the engine reads (fair-esm state-dict keys)."""
    d, f, V = cfg["d_model"], cfg["d_ffn"], cfg["vocab"]
    if cfg["arch"] == _lib.PG_ARCH_ESM1:
        s = {"embed_tokens.weight": (V, d), "embed_positions.weight": (cfg["max_positions"] + cfg["pad_idx"] + 1, d),
             "embed_out.weight": (V, d), "embed_out.bias": (V,)}
    elif cfg["arch"] == _lib.PG_ARCH_ESM2:        # no position table, no emb_layer_norm_before
        s = {"embed_tokens.weight": (V, d),
             "emb_layer_norm_after.weight": (d,), "emb_layer_norm_after.bias": (d,),
             "lm_head.dense.weight": (d, d), "lm_head.dense.bias": (d,),
             "lm_head.layer_norm.weight": (d,), "lm_head.layer_norm.bias": (d,), "lm_head.bias": (V,)}
    else:
        s = {"embed_tokens.weight": (V, d),
             "embed_positions.weight": (cfg["max_positions"] + cfg["pad_idx"] + 1, d),
             "emb_layer_norm_before.weight": (d,), "emb_layer_norm_before.bias": (d,),
             "emb_layer_norm_after.weight": (d,), "emb_layer_norm_after.bias": (d,),
             "lm_head.dense.weight": (d, d), "lm_head.dense.bias": (d,),
             "lm_head.layer_norm.weight": (d,), "lm_head.layer_norm.bias": (d,), "lm_head.bias": (V,)}

    def lin(p, o, i):
        s[p + ".weight"] = (o, i)
        s[p + ".bias"] = (o,)

    def ln(p):
        s[p + ".weight"] = (d,)
        s[p + ".bias"] = (d,)

    for i in range(cfg["n_layers"]):
        p = "layers.%d." % i
        if cfg["arch"] in (_lib.PG_ARCH_ESM1B, _lib.PG_ARCH_ESM1, _lib.PG_ARCH_ESM2):
            for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
                lin(p + "self_attn." + n, d, d)
            if cfg["arch"] == _lib.PG_ARCH_ESM1:
                s[p + "self_attn.bias_k"] = (d,)
                s[p + "self_attn.bias_v"] = (d,)
            ln(p + "self_attn_layer_norm")
            lin(p + "fc1", f, d)
            lin(p + "fc2", d, f)
            ln(p + "final_layer_norm")
        else:
            for blk in ("row_self_attention", "column_self_attention"):
                for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
                    lin(p + blk + ".layer." + n, d, d)
                ln(p + blk + ".layer_norm")
            lin(p + "feed_forward_layer.layer.fc1", f, d)
            lin(p + "feed_forward_layer.layer.fc2", d, f)
            ln(p + "feed_forward_layer.layer_norm")
    if cfg["arch"] == _lib.PG_ARCH_MSA1B:
        s["msa_position_embedding"] = (1, cfg["max_msa_rows"], 1, d)
    return s


def synthetic_state_dict(cfg, seed=0, std=0.02, embed_std=None, ln_jitter=0.0):
    """Seeded random weights: N(0, std^2) matrices/biases, LayerNorm gamma = 1 (+jitter), beta = 0 (+jitter)."""
    rng = np.random.default_rng(seed)
    es = std if embed_std is None else embed_std
    out = {}
    for name, shape in tensor_shapes(cfg).items():
        is_ln = "layer_norm" in name
        if is_ln and name.endswith(".weight"):
            a = 1.0 + ln_jitter * rng.standard_normal(shape, dtype=np.float32)
        elif is_ln:
            a = ln_jitter * rng.standard_normal(shape, dtype=np.float32)
        elif name == "embed_positions.weight" and cfg["arch"] == _lib.PG_ARCH_ESM1:
            a = sinusoidal_positions(shape[0], shape[1], cfg["pad_idx"])
        elif name.startswith("embed_") or name == "msa_position_embedding":
            a = es * rng.standard_normal(shape, dtype=np.float32)
        elif name.endswith("bias_k") or name.endswith("bias_v"):
            a = 0.3 * rng.standard_normal(shape, dtype=np.float32)
        else:
            a = std * rng.standard_normal(shape, dtype=np.float32)
        out[name] = np.ascontiguousarray(a, dtype=np.float32)
    return out


def _strip_fair_esm_prefixes(name):
    """fair-esm's `_load_model_and_alphabet_core_v1` (esm/pretrained.py, [recalled]: the package is not installed here) drops
    everything up to and including "encoder." and "sentence_encoder." from v1 checkpoint keys
    (`encoder.sentence_encoder.layers.0...` -> `layers.0...`, `encoder.lm_head.dense.weight` -> `lm_head.dense.weight`)."""
    for marker in ("sentence_encoder.", "encoder."):
        if marker in name:
            name = name.split(marker, 1)[1]
    if name.startswith("decoder."):            # ESM-1 ("protein_bert_base") checkpoints: everything under `decoder.`
        name = name[len("decoder."):]
    return name[len("model."):] if name.startswith("model.") else name


def _swap_row_column(name):
    """MSA Transformer checkpoints only: fair-esm's loader exchanges "row" and "column" in every key (its lambda `prs3`):
    in esm_msa1b_t12_100M_UR50S.pt the tensors stored as `row_self_attention.*` belong to the module's
    `column_self_attention` and vice versa.  All of them are d x d, so loading them unswapped would not fail -- it would
    silently put the tied-row weights into column attention."""
    if "row" in name:
        return name.replace("row", "column")
    return name.replace("column", "row")


def normalise_state_dict(sd, cfg, fair_esm_layout=True):
    """fair-esm checkpoint keys -> the engine's keys.

    fair_esm_layout=True applies what fair-esm's own loader does to an on-disk checkpoint: prefix stripping, and for the
    MSA Transformer the row<->column swap.  Pass False for a state dict that already has module names (e.g. one taken
    from a constructed fair-esm model with `model.state_dict()`, or `synthetic_state_dict`).
    Shapes are checked exactly; a tied decoder (`lm_head.weight`) must equal `embed_tokens.weight`."""
    want = tensor_shapes(cfg)
    is_msa = cfg["arch"] == _lib.PG_ARCH_MSA1B
    named = {}
    for k, v in sd.items():
        name = k
        if cfg["arch"] == _lib.PG_ARCH_ESM2 and name.endswith("rot_emb.inv_freq"):
            # a buffer fair-esm recomputes when it builds the module; the engine computes it too -- a file that disagrees is not ESM-2's
            got = (v.detach().cpu().float().numpy() if hasattr(v, "detach") else np.asarray(v, dtype=np.float32)).reshape(-1)
            hd = head_dim_of(cfg) or 64
            want_f = rotary_inv_freq(hd)
            if got.shape != want_f.shape or not np.allclose(got, want_f, rtol=1e-6, atol=0.0):
                raise ValueError("tensor %r disagrees with rotary inv_freq = 1 / 10000^(2i/%d) for heads of %d: the engine's rotary "
                                 "embedding implements that formula only" % (k, hd, hd))
            continue
        if fair_esm_layout:
            name = _strip_fair_esm_prefixes(name)
            if is_msa:
                name = _swap_row_column(name)
        arr = v.detach().cpu().float().numpy() if hasattr(v, "detach") else np.asarray(v, dtype=np.float32)
        if cfg["arch"] == _lib.PG_ARCH_ESM1:
            # fair-esm's ESM-1 module names -> the engine's: the untied output projection is a bare Parameter pair, bias_k / bias_v
            # are stored [1, 1, d]; the sinusoidal table is a buffer (`embed_positions._float_tensor`) that is regenerated here
            name = {"embed_out": "embed_out.weight", "embed_out_bias": "embed_out.bias"}.get(name, name)
            if name.endswith("self_attn.bias_k") or name.endswith("self_attn.bias_v"):
                arr = arr.reshape(-1)
        named[name] = arr
    if cfg["arch"] == _lib.PG_ARCH_ESM1 and "embed_positions.weight" not in named:
        named["embed_positions.weight"] = sinusoidal_positions(cfg["max_positions"] + cfg["pad_idx"] + 1, cfg["d_model"], cfg["pad_idx"])
    if cfg["arch"] == _lib.PG_ARCH_ESM1 and "embed_out.bias" not in named and "embed_out.weight" in named:
        named["embed_out.bias"] = np.zeros(cfg["vocab"], dtype=np.float32)          # final_bias = False checkpoints
    if "lm_head.weight" in named and cfg["arch"] != _lib.PG_ARCH_ESM1:
        if "embed_tokens.weight" not in named:
            named["embed_tokens.weight"] = named["lm_head.weight"]
        elif not np.array_equal(named["lm_head.weight"], named["embed_tokens.weight"]):
            raise ValueError("checkpoint has an untied lm_head.weight: this engine implements the tied decoder of ESM-1b / MSA-1b / ESM-2")
    out = {}
    for name, shape in want.items():
        if name not in named:
            continue
        arr = named[name]
        if tuple(arr.shape) != tuple(shape):
            raise ValueError("tensor %r has shape %s, expected %s" % (name, tuple(arr.shape), tuple(shape)))
        out[name] = np.ascontiguousarray(arr, dtype=np.float32)
    missing = [k for k in want if k not in out]
    if missing:
        raise KeyError("checkpoint is missing %d tensors, e.g. %s" % (len(missing), missing[:3]))
    if fair_esm_layout and cfg.get("token_dropout") and cfg["arch"] != _lib.PG_ARCH_ESM2:
        # (ESM-1b only: fair-esm's loader does this for `roberta_large` files and NOT for ESM-2 ones, whose <mask> row is used as
        # stored by the tied decoder -- [recalled], no real checkpoint is available offline.)
        # fair-esm zeroes the <mask> embedding row when it loads an ESM-1b checkpoint ("For token drop", [recalled]); the
        # forward never reads that row as an input (masked positions are zeroed), but the tied decoder does: after loading,
        # logit[<mask>] = lm_head.bias[<mask>] only.  The samplers never draw <mask> (it is not in valid_aa_idx) and
        # log_likelihood gathers the log-softmax at real residues, whose normaliser includes that bias-only term -- exactly
        # what fair-esm computes after the same zeroing.  [recalled]: not checkable offline; a real checkpoint file decides.
        out["embed_tokens.weight"] = out["embed_tokens.weight"].copy()
        out["embed_tokens.weight"][cfg["mask_idx"]] = 0.0
    return out


_ARCH_OF = {"roberta_large": _lib.PG_ARCH_ESM1B, "protein_bert_base": _lib.PG_ARCH_ESM1, "msa_transformer": _lib.PG_ARCH_MSA1B}
_ARCH_NAME = {_lib.PG_ARCH_ESM1B: "ESM-1b", _lib.PG_ARCH_ESM1: "ESM-1", _lib.PG_ARCH_MSA1B: "MSA-1b", _lib.PG_ARCH_ESM2: "ESM-2"}


def checkpoint_args(blob):
    """The hyper-parameters a fair-esm v1 checkpoint carries ({"args": Namespace | dict}) with ONE prefix dropped per
    architecture, as fair-esm's loader drops it before it builds the module (its lambda `pra`, esm/pretrained.py [recalled]):
    `encoder_` for roberta_large and msa_transformer, `decoder_` for protein_bert_base -- `encoder_embed_dim` -> `embed_dim`,
    `decoder_layers` -> `layers`, ...  Keys with the other prefix stay as they are (they are leftovers of the training namespace
    that fair-esm never reads), so a collision such as `encoder_embed_dim` vs `decoder_embed_dim` cannot be resolved by dict
    order.  {} when the file has none."""
    a = blob.get("args") if isinstance(blob, dict) else None
    if a is None:
        return {}
    raw = dict(a) if isinstance(a, dict) else dict(vars(a))
    pre = "decoder_" if raw.get("arch") == "protein_bert_base" else "encoder_"
    out = {}
    for k, v in raw.items():
        if pre in k:
            stripped = "".join(k.split(pre)[1:])
            out[stripped] = v                      # the prefixed form wins over an unprefixed leftover of the same name
    for k, v in raw.items():
        if pre not in k:
            out.setdefault(k, v)
    return out


def _take(cfg, take, explicit):
    """cfg.update(take), the file's own hyper-parameters; with explicit=True (the caller passed `config=`) a disagreement raises"""
    bad = {k: (cfg[k], v) for k, v in take.items() if cfg[k] != v} if explicit else None
    if bad:
        raise ValueError("config= disagrees with the checkpoint's own hyper-parameters: %s (given, in the file)" % bad)
    cfg.update(take)


def _count_layers(cfg, take, state_names, explicit):
    """-> cfg with the number of layers the tensors show, which may stand in for a number nobody stated and must agree with a stated one"""
    n_layers_seen = 1 + max([int(m.group(1)) for m in (re.match(r"layers\.(\d+)\.", n) for n in state_names) if m] or [-1])
    if n_layers_seen and n_layers_seen != cfg["n_layers"]:
        if "n_layers" in take or explicit:
            raise ValueError("checkpoint holds %d layers but its hyper-parameters say %d" % (n_layers_seen, cfg["n_layers"]))
        cfg["n_layers"] = n_layers_seen
    return cfg


def config_from_checkpoint(args, state_names, base_cfg, explicit=False):
    """The engine configuration a checkpoint asks for: `base_cfg` (the wrapper's architecture defaults) overridden by the
    checkpoint's own hyper-parameters -- what `esm.pretrained.*` builds the module from in the reference
    (/root/reference/src/pgen/models.py:61-86) -- instead of a fixed dict per wrapper.  Read: arch, embed_dim, layers,
    attention_heads, ffn_embed_dim, max_positions, token_dropout, emb_layer_norm_before, final_bias, embed_positions_msa.
    What fair-esm HONOURS for that architecture and the engine does not implement raises ValueError naming the flag; flags fair-esm
    itself never reads for the architecture (released `args` are the internal training namespace and may carry such leftovers:
    `token_dropout` in an msa_transformer file -- MSATransformer has no token dropout --, `final_bias` outside ESM-1 --
    RobertaLMHead always has a bias --, an `emb_layer_norm_before` value that the tensors contradict -- fair-esm decides it from the
    tensors) are ignored with a warning, as the loader the reference relies on would load the file.  With
    explicit=True (the caller passed `config=`) a disagreement between that config and the file raises instead of silently
    picking one.  NOT validated against the args of the real released .pt files (none are available offline)."""
    import warnings
    cfg = dict(base_cfg)
    arch = args.get("arch")
    if arch is not None:
        if arch not in _ARCH_OF:
            raise ValueError("checkpoint arch %r is not one of the architectures of pgen.models (roberta_large = ESM-1b / ESM-1v, "
                             "protein_bert_base = ESM-1, msa_transformer = ESM-MSA-1b)" % (arch,))
        if _ARCH_OF[arch] != cfg["arch"]:
            raise ValueError("checkpoint arch %r does not match the requested %s engine" % (arch, _ARCH_NAME[cfg["arch"]]))
    take = {}
    for key, name in (("embed_dim", "d_model"), ("layers", "n_layers"), ("attention_heads", "n_heads"), ("ffn_embed_dim", "d_ffn"),
                      ("max_positions", "max_positions")):
        if args.get(key) is not None:
            take[name] = int(args[key])
    esm1b = cfg["arch"] == _lib.PG_ARCH_ESM1B
    if esm1b and "token_dropout" in args:
        take["token_dropout"] = 1 if args["token_dropout"] else 0
    _take(cfg, take, explicit)
    if cfg["n_heads"] * 64 != cfg["d_model"]:
        raise ValueError("checkpoint has %d heads of dimension %g: the engine's attention kernels implement head dimension 64 "
                         "(every model of pgen.models)" % (cfg["n_heads"], cfg["d_model"] / max(1, cfg["n_heads"])))
    has_ln_before = any(n.startswith("emb_layer_norm_before") for n in state_names)
    if cfg["arch"] in (_lib.PG_ARCH_ESM1B, _lib.PG_ARCH_MSA1B):
        # fair-esm decides this flag from the tensors (`has_emb_layer_norm_before`), not from args
        if not has_ln_before:
            raise ValueError("checkpoint was trained without emb_layer_norm_before: the %s engine always applies it (every released "
                             "ESM-1b / ESM-1v / ESM-MSA-1b checkpoint has it)" % _ARCH_NAME[cfg["arch"]])
        if args.get("emb_layer_norm_before") is False:
            warnings.warn("checkpoint args say emb_layer_norm_before=False but the file holds emb_layer_norm_before.*: going by the "
                          "tensors, as fair-esm does")
        if args.get("final_bias") is False:
            warnings.warn("final_bias=False in a %s checkpoint is ignored: only ESM-1's embed_out reads it, RobertaLMHead always has "
                          "a bias" % _ARCH_NAME[cfg["arch"]])
    elif has_ln_before:
        raise ValueError("ESM-1 checkpoint with emb_layer_norm_before tensors: the ESM-1 engine has no embedding LayerNorms")
    elif args.get("emb_layer_norm_before"):
        warnings.warn("checkpoint args say emb_layer_norm_before=True but the file holds no such tensors: going by the tensors, as "
                      "fair-esm does")
    if cfg["arch"] == _lib.PG_ARCH_MSA1B and args.get("embed_positions_msa") is False:
        raise ValueError("embed_positions_msa=False: the MSA engine adds msa_position_embedding (esm_msa1b_t12_100M_UR50S has it)")
    if args.get("token_dropout"):
        if cfg["arch"] == _lib.PG_ARCH_ESM1:
            raise ValueError("token_dropout=True in an ESM-1 checkpoint: fair-esm's ProteinBertModel would apply it, the ESM-1 engine "
                             "does not implement it (none of esm1_t6 / t12 / t34 sets it)")
        if cfg["arch"] == _lib.PG_ARCH_MSA1B:
            warnings.warn("token_dropout=True in an msa_transformer checkpoint is ignored: fair-esm's MSATransformer never reads it")
    return _count_layers(cfg, take, state_names, explicit)


def checkpoint_cfg_v2(blob):
    """The model hyper-parameters of a fair-esm v2 checkpoint ({"cfg": {"model": Namespace | mapping}, "model": state dict} -- the
    ESM-2 files; fair-esm's `_load_model_and_alphabet_core_v2` reads `encoder_layers`, `encoder_embed_dim`, `encoder_attention_heads`
    and `token_dropout` from it, [recalled]) as a dict; None when `blob` is not in that layout."""
    c = blob.get("cfg") if isinstance(blob, dict) and "args" not in blob else None
    m = (c.get("model") if isinstance(c, dict) else getattr(c, "model", None)) if c is not None else None
    if m is None:
        return None
    return dict(m) if isinstance(m, dict) else dict(vars(m))


def config_from_checkpoint_v2(model_cfg, state_names, base_cfg, explicit=False):
    """The engine configuration an ESM-2 (v2) checkpoint asks for: `base_cfg` overridden by the file's encoder_layers /
    encoder_embed_dim / encoder_attention_heads / token_dropout; d_ffn is 4 x embed_dim (fair-esm's ESM2 has no other).  Sizes the
    engine cannot run raise ValueError naming the reason."""
    cfg = dict(base_cfg)
    take = {}
    for key, name in (("encoder_embed_dim", "d_model"), ("encoder_layers", "n_layers"), ("encoder_attention_heads", "n_heads")):
        if model_cfg.get(key) is not None:
            take[name] = int(model_cfg[key])
    if "d_model" in take:
        take["d_ffn"] = 4 * take["d_model"]
    if "token_dropout" in model_cfg:
        take["token_dropout"] = 1 if model_cfg["token_dropout"] else 0
    _take(cfg, take, explicit)
    # Head width (HEAD_WIDTHS).  64 loads against every base configuration; a width built for ESM-2 only loads against a configuration
    # whose own heads have that width (32: ESM2_T30_CONFIG, models.ESM2_150M, and so on) -- a wrapper promises its model, as ESM2 refuses
    # the 3B file below; 24, an embedded width (EMBEDDED_WIDTHS), loads against ESM2_T12_CONFIG only and then under its slot's limits.  Then the engine's own order: heads per row, row width (csrc/engine.hip, csrc/ln_row.h).
    hd = cfg["d_model"] / max(1, cfg["n_heads"])
    has = "checkpoint has %d heads of dimension %g: " % (cfg["n_heads"], hd)
    row = HEAD_WIDTHS.get(hd)
    emb = EMBEDDED_WIDTHS.get(hd)
    own = emb or (row if row and row["esm2_only"] else None)      # a width that loads only against a configuration whose heads have it
    if own and head_dim_of(base_cfg) != hd:
        raise ValueError(has + "the engine's attention kernels implement head dimension 64 for the configuration it was loaded against; "
                         "load %s (heads of %g) with models.%s / --model %s" % (own["file"], hd, own["wrapper"], own["cli"]))
    if emb:
        row = dict(HEAD_WIDTHS[emb["slot"]], **ESM2_SIZES[emb["cli"]])      # the slot's limits, the size's own names
    if row is None:
        raise ValueError(has + "the engine's attention kernels implement head dimension 64 (every model of pgen.models) and, for ESM-2, "
                         + ", ".join("%d (%s)" % (w, r["file"]) for w, r in HEAD_WIDTHS.items() if r["esm2_only"]))
    if cfg["n_heads"] > row["max_heads"]:
        raise ValueError(has + "the engine's rotary and row kernels hold at most %d of them per row (d_model %d > %d; %s has %d)"
                         % (row["max_heads"], cfg["d_model"], hd * row["max_heads"], row["file"], row["config"]["n_heads"]))
    if cfg["d_model"] > MAX_D_MODEL and cfg["d_model"] % 512:
        raise ValueError("checkpoint has d_model %d > %d: the engine's row kernels (LayerNorm, embedding, LM head, rotation) take "
                         "multiples of 512 up to %d there" % (cfg["d_model"], MAX_D_MODEL, MAX_D_MODEL_HD128))
    # models.ESM2 / --model esm2 promise the 650M model: a 3B file is 4.4 times the work and is loaded on purpose, not by accident
    if cfg["d_model"] > ESM2_650M_MAX_D_MODEL and base_cfg["d_model"] <= ESM2_650M_MAX_D_MODEL:
        raise ValueError("checkpoint has d_model %d > %d, wider than the ESM-2 650M configuration it was loaded against: load "
                         % (cfg["d_model"], ESM2_650M_MAX_D_MODEL) + "%(file)s with models.%(wrapper)s / --model %(cli)s" % ESM2_SIZES["esm2_3b"])
    if any(n.startswith("emb_layer_norm_before") or n.startswith("embed_positions") for n in state_names):
        raise ValueError("ESM-2 checkpoint with emb_layer_norm_before / embed_positions tensors: the ESM-2 engine has neither")
    return _count_layers(cfg, take, state_names, explicit)


def load_fair_esm_checkpoint(path, cfg, return_config=False, explicit_config=False):
    """Read a fair-esm `.pt` file ({"args": ..., "model": state dict}; for an ESM-2 `cfg` the v2 layout {"cfg": {"model": ...},
    "model": state dict}) as the reference does through `esm.pretrained.*` (/root/reference/src/pgen/models.py:61,86).  `cfg` gives
    the architecture (and the defaults of a file without `args`); sizes and flags come from the checkpoint's own hyper-parameters
    (config_from_checkpoint, config_from_checkpoint_v2).  return_config=True -> (state dict, cfg)."""
    import torch
    blob = torch.load(path, map_location="cpu", weights_only=False)
    sd = blob["model"] if isinstance(blob, dict) and "model" in blob else blob
    args = checkpoint_args(blob)
    v2 = checkpoint_cfg_v2(blob) if not args else None
    if cfg["arch"] == _lib.PG_ARCH_ESM2:
        if args:
            raise ValueError("checkpoint in fair-esm's v1 layout (arch %r): not an ESM-2 file" % (args.get("arch"),))
        names = [_strip_fair_esm_prefixes(k) for k in sd]
        cfg2 = config_from_checkpoint_v2(v2 or {}, names, cfg, explicit=explicit_config)
        out = normalise_state_dict(sd, cfg2, fair_esm_layout=True)
        return (out, cfg2) if return_config else out
    if v2 is not None:
        raise ValueError("checkpoint in fair-esm's v2 layout (ESM-2): not one of the models of pgen.models -- load it with models.ESM2")
    is_msa = cfg["arch"] == _lib.PG_ARCH_MSA1B
    names = [_swap_row_column(_strip_fair_esm_prefixes(k)) if is_msa else _strip_fair_esm_prefixes(k) for k in sd]
    cfg2 = config_from_checkpoint(args, names, cfg, explicit=explicit_config)
    out = normalise_state_dict(sd, cfg2, fair_esm_layout=True)
    return (out, cfg2) if return_config else out


def to_fair_esm_checkpoint_layout(sd, cfg):
    """Inverse of the key mapping above: engine/module names -> the on-disk fair-esm key layout (used to write test
    fixtures and to export weights): `encoder.sentence_encoder.` prefix on trunk tensors, `encoder.` on the LM head, and
    row<->column exchanged for the MSA Transformer.  ESM-2 (v2 files): the same prefixes, the tied decoder also stored as
    `encoder.lm_head.weight`, and every layer's `self_attn.rot_emb.inv_freq` buffer; `to_fair_esm_checkpoint_v2` adds the `cfg`."""
    is_msa = cfg["arch"] == _lib.PG_ARCH_MSA1B
    out = {}
    for name, v in sd.items():
        k = _swap_row_column(name) if is_msa else name
        k = ("encoder." + k) if k.startswith("lm_head.") else ("encoder.sentence_encoder." + k)
        out[k] = v
    if cfg["arch"] == _lib.PG_ARCH_ESM2:
        out["encoder.lm_head.weight"] = sd["embed_tokens.weight"]
        for i in range(cfg["n_layers"]):
            out["encoder.sentence_encoder.layers.%d.self_attn.rot_emb.inv_freq" % i] = rotary_inv_freq(head_dim_of(cfg) or 64)
    return out


def to_fair_esm_checkpoint_v2(sd, cfg, namespace=True):
    """A whole ESM-2 checkpoint blob in fair-esm's v2 layout, ready for torch.save: {"cfg": {"model": Namespace (or a dict with
    namespace=False)}, "model": state dict of tensors}."""
    import argparse

    import torch
    m = dict(encoder_layers=cfg["n_layers"], encoder_embed_dim=cfg["d_model"], encoder_attention_heads=cfg["n_heads"],
             token_dropout=bool(cfg["token_dropout"]))
    model = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in to_fair_esm_checkpoint_layout(sd, cfg).items()}
    return {"cfg": {"model": argparse.Namespace(**m) if namespace else m}, "model": model}


def find_cached_checkpoint(filename):
    p = os.path.join(os.path.expanduser("~/.cache/torch/hub/checkpoints"), filename)
    return p if os.path.exists(p) else None


# ---- the contact regression head (fair-esm's ContactPredictionHead: one logistic regression over n_layers * n_heads channels) ----
_CONTACT_KEYS = ("contact_head.regression.weight", "contact_head.regression.bias")


def contact_regression_path(path):
    """Where fair-esm keeps the contact regression of the ESM-1b / ESM-1v / ESM-2 checkpoint `path`: the sibling
    `<stem>-contact-regression.pt` ({"model": {"contact_head.regression.weight", "contact_head.regression.bias"}})."""
    stem, ext = os.path.splitext(path)
    return stem + "-contact-regression" + (ext or ".pt")


def _contact_head_of(sd, cfg, where):
    """(weight float32 [n_layers * n_heads], bias) from a state dict's contact_head.regression.{weight, bias} under any of fair-esm's
    prefixes, None when it holds neither.  A shape that is not the model's raises, naming both."""
    found = {}
    for k, v in sd.items():
        name = _strip_fair_esm_prefixes(k)
        if name in _CONTACT_KEYS:
            found[name] = np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float32)
    if not found:
        return None
    if len(found) != 2:
        raise ValueError("%s holds %s without %s" % (where, *[k for k in _CONTACT_KEYS if k in found], *[k for k in _CONTACT_KEYS if k not in found]))
    w, b = found[_CONTACT_KEYS[0]], found[_CONTACT_KEYS[1]]
    n = cfg["n_layers"] * cfg["n_heads"]
    if w.shape not in ((1, n), (n,)):
        raise ValueError("%s: contact_head.regression.weight has shape %r, the model of %d layers x %d heads needs %r"
                         % (where, tuple(w.shape), cfg["n_layers"], cfg["n_heads"], (1, n)))
    if b.size != 1:
        raise ValueError("%s: contact_head.regression.bias has shape %r, not %r" % (where, tuple(b.shape), (1,)))
    return np.ascontiguousarray(w.reshape(-1)), float(b.reshape(-1)[0])


def contact_head_from_checkpoint(path, cfg):
    """The contact regression that goes with the fair-esm checkpoint `path` of a model `cfg`: (weight float32 [n_layers * n_heads]
    in channel order l * n_heads + h, bias), taken from the file itself when it carries contact_head.regression.* and otherwise from
    its sibling contact_regression_path(path); None when neither has one.  load_fair_esm_checkpoint does not look at these keys."""
    import torch
    for p in (path, contact_regression_path(path)):
        if not os.path.exists(p):
            continue
        blob = torch.load(p, map_location="cpu", weights_only=False)
        sd = blob["model"] if isinstance(blob, dict) and "model" in blob else blob
        head = _contact_head_of(sd, cfg, p)
        if head is not None:
            return head
    return None


def synthetic_contact_head(cfg, seed=0, std=1.0, bias=-1.0):
    """A seeded contact regression for a model `cfg`: weight N(0, std^2) float32 [n_layers * n_heads], and the bias."""
    rng = np.random.default_rng([seed, 0xC0])
    return (std * rng.standard_normal(cfg["n_layers"] * cfg["n_heads"])).astype(np.float32), float(bias)
