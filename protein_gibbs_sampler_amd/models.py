"""Model wrappers with the three attributes the samplers expect: `.model`, `.alphabet`,
`.batch_converter` -- the plug-in contract of /root/reference/src/pgen/models.py:59-88.

`.model` is a NativeMaskedLM (HIP engine handle) instead of a fair-esm nn.Module.  Weights: a real
fair-esm checkpoint when one is given or found in torch's hub cache.  Without one the constructor RAISES
(as `esm.pretrained.*` fails in the reference when it cannot load) unless the caller opts in to seeded
synthetic weights of the same architecture with `synthetic=True` (benchmarks, tests): samples from those
are not biologically meaningful.
"""

from . import weights as _w
from .alphabet import Alphabet
from .engine import NativeMaskedLM


def _resolve_weights(cfg, state_dict, checkpoint, filename, seed, synthetic, explicit_config=False):
    """-> (state dict, config).  A checkpoint file brings its own hyper-parameters (weights.config_from_checkpoint): `cfg` is the
    wrapper's architecture and the default for files that carry none."""
    if state_dict is not None:
        return state_dict, cfg
    path = checkpoint or _w.find_cached_checkpoint(filename)
    if path:
        return _w.load_fair_esm_checkpoint(path, cfg, return_config=True, explicit_config=explicit_config)
    if not synthetic:
        raise FileNotFoundError(
            "no %s checkpoint: pass checkpoint=<path to the fair-esm .pt file> (CLI: --checkpoint) or place it in "
            "~/.cache/torch/hub/checkpoints/.  Seeded synthetic weights of the same architecture are available only as an "
            "explicit opt-in (synthetic=True / --synthetic-weights): output sampled from them is not biologically "
            "meaningful." % filename)
    return _w.synthetic_state_dict(cfg, seed=seed), cfg


class _Wrapper:
    def __init__(self, cfg, alphabet, msa, state_dict, checkpoint, filename, seed, precision, synthetic, explicit_config=False):
        sd, cfg = _resolve_weights(cfg, state_dict, checkpoint, filename, seed, synthetic, explicit_config)
        self.cfg = cfg
        self.alphabet = alphabet
        self.batch_converter = alphabet.get_batch_converter(msa=msa)
        self.model = NativeMaskedLM(cfg, sd, precision)
        self._contact_source = None      # the files a contact regression was looked for in (none: weights handed in as a state dict)
        if self.has_contacts or self.has_row_contacts:
            self._load_contact_head(state_dict, checkpoint, filename, seed, synthetic)

    # ESM-1b, ESM-1v and every ESM-2 come with a contact regression over their attention maps (predict_contacts); the MSA Transformer's
    # is over its tied row-attention maps and has names of its own (has_row_contacts, predict_row_contacts); ESM-1 (bias key) has none
    has_contacts = True
    has_row_contacts = False

    def _load_contact_head(self, state_dict, checkpoint, filename, seed, synthetic):
        if state_dict is not None:
            return
        path = checkpoint or _w.find_cached_checkpoint(filename)
        if path:
            self._contact_source = "%s or %s" % (path, _w.contact_regression_path(path))
            # a regression that is not this model's (contact_head.* has always been ignored on load) must not keep the model from
            # sampling: it is left out, and predict_contacts says why
            try:
                head = _w.contact_head_from_checkpoint(path, self.cfg)
            except ValueError as e:
                head = None
                self._contact_source += "; refused: %s" % e
        else:
            head = _w.synthetic_contact_head(self.cfg, seed) if synthetic else None
        if head is not None:
            (self.model.set_row_contact_head if self.has_row_contacts else self.model.set_contact_head)(*head)

    def predict_contacts(self, tokens):
        """fair-esm's model.predict_contacts(tokens): float32 [B, T-2, T-2].  NotImplementedError for the models without a contact
        entry, RuntimeError naming the files looked in when the checkpoint came without a regression."""
        if not self.has_contacts:
            raise NotImplementedError("%s has no contact prediction in this package (ESM-1b, ESM-1v and ESM-2 only%s)"
                                      % (type(self).__name__, "; the MSA Transformer's is predict_row_contacts" if self.has_row_contacts else ""))
        if not self.model.has_contact_head:
            raise RuntimeError("%s: no contact regression loaded (looked in %s): pass one with .model.set_contact_head(weight, bias)"
                               % (type(self).__name__, self._contact_source or "nothing: the weights were handed in as a state dict"))
        return self.model.predict_contacts(tokens)


class ESM1b(_Wrapper):
    """esm1b_t33_650M_UR50S (models.py:59-62)."""

    def __init__(self, state_dict=None, checkpoint=None, seed=0, precision="auto", config=None, synthetic=False):
        super().__init__(config or dict(_w.ESM1B_CONFIG), Alphabet(True, True), False, state_dict, checkpoint,
                         "esm1b_t33_650M_UR50S.pt", seed, precision, synthetic, config is not None)


class ESM1v(_Wrapper):
    """esm1v_t33_650M_UR90S (models.py:64-67): same architecture as ESM-1b, different weights."""

    def __init__(self, state_dict=None, checkpoint=None, seed=0, precision="auto", config=None, synthetic=False):
        super().__init__(config or dict(_w.ESM1B_CONFIG), Alphabet(True, True), False, state_dict, checkpoint,
                         "esm1v_t33_650M_UR90S_1.pt", seed, precision, synthetic, config is not None)


def _size(cli):
    """(configuration, checkpoint file name) of a released ESM-2 size: its row of weights.ESM2_SIZES"""
    return _w.ESM2_SIZES[cli]["config"], _w.ESM2_SIZES[cli]["file"] + ".pt"


class _ESM2(_Wrapper):
    """ESM-2 family: the ESM-1b alphabet, <cls> prepended and <eos> appended; the v2 checkpoint layout."""
    _cfg, _file = None, None

    def __init__(self, state_dict=None, checkpoint=None, seed=0, precision="auto", config=None, synthetic=False):
        super().__init__(config or dict(self._cfg), Alphabet(True, True), False, state_dict, checkpoint,
                         self._file, seed, precision, synthetic, config is not None)


class ESM2(_ESM2):
    """esm2_t33_650M_UR50D: fair-esm's ESM-2 at 650M parameters (not a model of the original pgen package; the successor of ESM-1b
    in fair-esm) -- rotary position embeddings, no emb_layer_norm_before, the ESM-1b alphabet and LM head.  Reads the v2 checkpoint
    layout (weights.load_fair_esm_checkpoint).  This wrapper promises the 650M model: a checkpoint wider than d_model 2048 (the 3B
    file, 4.4 times the work per token) is refused with a message naming ESM2_3B, and the 150M file (heads of 32) with one naming
    ESM2_150M, the 15B file (heads of 128) with one naming ESM2_15B, the 8M file (heads of 16) with one naming ESM2_8M and the 35M
    file (heads of 24, which run embedded in slots of 32) with one naming ESM2_35M."""
    _cfg, _file = _size("esm2")


class ESM2_3B(_ESM2):
    """esm2_t36_3B_UR50D: ESM-2 at 3B parameters -- 36 layers, d_model 2560, 40 heads of 64, d_ffn 10240; about 5.7 GB of 16-bit
    weights on the device (17 GB in precision="fp32").  The same wrapper as ESM2 (v2 checkpoint layout, ESM-1b alphabet and LM head)
    with the wider configuration; the widest model the engine's row kernels hold (csrc/ln_row.h).  Sizes come from the file: a
    narrower checkpoint with heads of 64 (the 650M file included) loads here without remark and runs as the model it is -- only the
    opposite mismatch, a 3B file met by ESM2, is refused."""
    _cfg, _file = _size("esm2_3b")


class ESM2_150M(_ESM2):
    """esm2_t30_150M_UR50D: ESM-2 at 150M parameters -- 30 layers, d_model 640, 20 heads of 32, d_ffn 2560; a quarter of the 650M
    model's GEMM work per token, the size to iterate a design loop with.  The same wrapper as ESM2 with the head-32 instantiations of
    the attention and rotary kernels (csrc/attn_frag.h).  Sizes come from the file: any checkpoint with heads of 32 (at most 32 of
    them) or of 64 loads here and runs as the model it is; heads of 32 load ONLY here -- ESM2 and ESM2_3B refuse them by name."""
    _cfg, _file = _size("esm2_150m")


class ESM2_15B(_ESM2):
    """esm2_t48_15B_UR50D: ESM-2 at 15B parameters -- 48 layers, d_model 5120, 40 heads of 128, d_ffn 20480.  The same wrapper as ESM2
    with the head-128 instantiations of the attention and rotary kernels (csrc/attn_frag.h) and the 20-chunk row kernels
    (csrc/ln_row.h).  Sizes come from the file: any checkpoint with heads of 128 (at most 40 of them; d_model a multiple of 512 above
    2560) or of 64 loads here and runs as the model it is; heads of 128 load ONLY here -- ESM2, ESM2_3B and ESM2_150M refuse them by
    name.  Device footprint of the weights, hipMemGetInfo before / after engine creation on an MI355X (profiles/esm2_15b_bench_mi355x.json):
    16-bit modes 2.573 GB at 4 layers and 5.090 GB at 8, i.e. 0.629 GB per layer and 30.3 GB at 48 layers; strict mode
    (precision="fp32") 4.096 GB at 2 layers and 7.713 GB at 4, i.e. 1.809 GB per layer and 87.3 GB at 48.  The 48-layer figures are
    extrapolated from those measurements: the full model has not been created (its synthetic fp32 weights are 60 GB on the host)."""
    _cfg, _file = _size("esm2_15b")


class ESM2_8M(_ESM2):
    """esm2_t6_8M_UR50D: ESM-2 at 8M parameters -- 6 layers, d_model 320, 20 heads of 16, d_ffn 1280; the smallest released size, the
    one to tune a design loop of thousands of chains on.  The same wrapper as ESM2 with the head-16 instantiations of the attention and
    rotary kernels (csrc/attn_frag.h: a half-depth score MFMA, 32-byte LDS rows).  Sizes come from the file: any checkpoint with heads
    of 16 (at most 32 of them, d_model a multiple of 64) or of 64 loads here and runs as the model it is; heads of 16 load ONLY here --
    ESM2, ESM2_3B, ESM2_150M and ESM2_15B refuse them by name."""
    _cfg, _file = _size("esm2_8m")


class ESM2_35M(_ESM2):
    """esm2_t12_35M_UR50D: ESM-2 at 35M parameters -- 12 layers, d_model 480, 20 heads of 24, d_ffn 1920.  No kernel is built for heads
    of 24 and the GEMMs take multiples of 64, so the engine runs this model EMBEDDED in a shape it already runs: every head in a slot of
    32, rows of 640 features whose last 160 are structurally zero -- the geometry of ESM2_150M, 1.48 times the model's own GEMM work and
    1.33 times its attention work.  A zero-padded transformer computes the same function except in LayerNorm, whose kernels normalise
    over the 480 live features (include/pgibbs.h pg_engine_create_embedded).  Sizes come from the file: any
    checkpoint with heads of 24 (at most 32 of them) or of 64 loads here and runs as the model it is; heads of 24 load ONLY here -- the
    other wrappers refuse them by name."""
    _cfg, _file = _size("esm2_35m")


# the ESM-2 wrappers under their command-line names (--model)
ESM2_MODELS = {cli: globals()[row["wrapper"]] for cli, row in _w.ESM2_SIZES.items()}


class ESM_MSA1(_Wrapper):
    """esm_msa1b_t12_100M_UR50S (models.py:84-88) with the reference's patched MSA batch converter."""
    has_contacts = False      # no [B, T] contacts entry: the maps are the tied row attention's, over tokens [B, R, C]
    has_row_contacts = True   # fair-esm's return_contacts=True: the regression over the n_layers x n_heads row-attention maps

    def __init__(self, state_dict=None, checkpoint=None, seed=0, precision="auto", config=None, synthetic=False):
        super().__init__(config or dict(_w.MSA1B_CONFIG), Alphabet(True, False), True, state_dict, checkpoint,
                         "esm_msa1b_t12_100M_UR50S.pt", seed, precision, synthetic, config is not None)

    def predict_row_contacts(self, tokens):
        """fair-esm's MSATransformer.predict_contacts(tokens) for tokens [B, R, C]: float32 [B, C-1, C-1], the contact probabilities of
        the query sequence's residues (row 0; only <cls> is cut).  RuntimeError naming the files looked in when the checkpoint came
        without a regression."""
        if not self.model.has_row_contact_head:
            raise RuntimeError("%s: no contact regression loaded (looked in %s): pass one with .model.set_row_contact_head(weight, bias)"
                               % (type(self).__name__, self._contact_source or "nothing: the weights were handed in as a state dict"))
        return self.model.predict_row_contacts(tokens)


class _ESM1(_Wrapper):
    """ESM-1 family (models.py:69-82): the 35-token "ESM-1" alphabet, <cls> prepended, no <eos>."""
    _cfg, _file = None, None
    has_contacts = False      # the bias key changes the softmax and the map shape

    def __init__(self, state_dict=None, checkpoint=None, seed=0, precision="auto", config=None, synthetic=False):
        super().__init__(config or dict(self._cfg), Alphabet(True, False, arch="ESM-1"), False, state_dict, checkpoint,
                         self._file, seed, precision, synthetic, config is not None)


class ESM6(_ESM1):
    """esm1_t6_43M_UR50S (models.py:69-72): the model the reference's own unit tests load (test/test_esm_sampler.py:10-18)."""
    _cfg, _file = _w.ESM1_T6_CONFIG, "esm1_t6_43M_UR50S.pt"


class ESM12(_ESM1):
    """esm1_t12_85M_UR50S (models.py:74-77)."""
    _cfg, _file = _w.ESM1_T12_CONFIG, "esm1_t12_85M_UR50S.pt"


class ESM34(_ESM1):
    """esm1_t34_670M_UR50S (models.py:79-82)."""
    _cfg, _file = _w.ESM1_T34_CONFIG, "esm1_t34_670M_UR50S.pt"
