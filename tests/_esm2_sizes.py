"""One row per released ESM-2 size, keyed by its --model name: everything in which the shared test bodies (tests/_esm2_gpu_common.py,
tests/_esm2_cpu_common.py; run by tests/test_gpu_esm2_sizes.py, tests/test_esm2_sizes_cpu.py and each size's own file) differ from
size to size, with the reason next to the value.
A field that is None or absent means the size has no such test; the comment says why.  What is peculiar to one size stays in that
size's own file (tests/test_gpu_esm2*.py, tests/test_esm2*_cpu.py).  Wrapper, configuration and file name come from the product's own
table, weights.ESM2_SIZES; the figures restated here (`shape`, `max_heads`) are the tests' independent statement of them.
Host-side fields: `shape` (d_model, n_layers, n_heads, d_ffn of the released model), `max_heads` per row at the width, `cut` (a d_model
and the head count make_config must derive from it), `v2_file` (the cut written as a v2 checkpoint file, and its d_model, n_layers,
n_heads, d_ffn), `other_table` (the head width whose inv_freq table is the wrong one to find in that file)."""
from protein_gibbs_sampler_amd import models, weights

LONG_SEQ = "MRHGDISSSNDTVGVAVVNYKMPRLHTAAEVLDNAR"
# the sequence lengths of the forward test.  16 / 27: one 16- / 32-row tile (weight-streaming GEMMs), 64 ... 288: the attention kernels'
# key-count boundaries, 600: the long-sequence kernel; three sequences per batch, one at 600
FWD_BATCHES = [(3 if T < 300 else 1, T) for T in (16, 27, 64, 160, 258, 288, 600)]
# max |engine - reference| per unit of logit std: the 650M tests' bounds (0.25 and 0.04 at logit std 5).  35M: the same kernels at the
# same run shape as 150M, not refitted
FWD_TOL_PER_STD = {"bf16": 0.05, "fp16": 0.008}
# T, H and precision of the attention test (the decorator of each width's own file).  16 ... 576: rungs of the whole-sequence ladder (576 = the last one), 577 and 1026: the long-sequence kernel
# (two and four 288-key tiles)
ATTENTION_T = [16, 27, 258, 300, 576, 577, 1026]
ATTENTION_H = [2, 20]
PRECISIONS = ["fp32", "bf16", "fp16"]
ROPE_T, ROPE_H = [1, 27, 258, 1026], [4, 20, 32]

SIZES = {
    "esm2": dict(
        hd=64, shape=(1280, 33, 20, 5120), max_heads=40,
        case=dict(n_layers=6, d=768, std=0.03, embed_std=0.15),                 # logit std ~5 at d = 768
        label="6 x 768",
        # absolute bounds: this model's logit std is 5, where they are the per-std bounds of the other sizes
        forward=dict(shapes={"": {}}, tol={"bf16": 0.25, "fp16": 0.04}, per_std=False),
        full=dict(std=0.025, embed_std=0.3, T=258),                              # logit std ~10
        sampler=dict(n_layers=4, d=256), seq=LONG_SEQ,
        single_chain=dict(n_layers=3, d=256, seed=13),
        # 64 chains x 258 tokens as 2 and 8 contiguous shards
        shards=dict(case={}, worlds=(2, 8), B=64, split_child=False),
    ),
    "esm2_3b": dict(
        hd=64, shape=(2560, 36, 40, 10240), max_heads=40,
        case=dict(n_layers=3, d=2560, std=0.017, embed_std=0.1),                # logit std ~5 at d = 2560; 236 M weights on the host
        # forward: tests/test_gpu_esm2_3b.py keeps its own (three lengths, two sequences per batch, the padded batch under the last
        # length's std); its bound is 0.08 bf16 / 0.008 fp16 per unit of logit std, 2.5 x the first measured run
        forward=None,
        # synthetic weights that put the logit std of the 36 x 2560 model near 10 (measured 10.20; the 650M test's 0.025 / 0.3 would give
        # ~15: the tied decoder's logits scale with embed_std * sqrt(d_model)); 66 tokens: the numpy reference of 36 x 2560 is the cost
        full=dict(std=0.018, embed_std=0.21, T=66, logit_std=(7.0, 14.0)),       # first measured run: 6.87e-4
        sampler={}, seq="MRHGDISSSNDTVGVAVVNY",                                  # 20 residues: the reference runs 3 x 2560 on the host
        single_chain=dict(seed=13), child_timeout=600,
        # a 32-chain job (8256 token rows) as 2 and 4 contiguous shards
        shards=dict(case={}, worlds=(2, 4), B=32, split_child=False),
    ),
    "esm2_150m": dict(
        hd=32, shape=(640, 30, 20, 2560), max_heads=32, cut=(128, 4), other_table=64,
        v2_file=dict(cut=dict(d_model=128, n_layers=2, d_ffn=512), shape=(128, 2, 4, 512)),      # four heads of 32
        case=dict(n_layers=6, d=640, std=0.03, embed_std=0.15),
        label="6 x 640, 20 heads of 32",
        # q as the engine hands it over: scaled, |score| of a few units
        attention=dict(q_draw=0.35),
        forward=dict(shapes={"": {}}, tol=FWD_TOL_PER_STD, per_std=True),
        full=dict(std=0.035, embed_std=0.3, T=258),
        auto=dict(case=dict(n_layers=2, d=128), full_synthetic=False),
        other_archs=dict(d_model=128, n_heads=4),
        sampler=dict(n_layers=4, d=256), seq=LONG_SEQ,
        single_chain=dict(n_layers=3, d=256, seed=13),
        # 64 chains x 20 heads at 18 key blocks: the whole job and the 32- and 8-chain shards each end in a partial round that the
        # attention launch splits -- and with PGIBBS_ATTN_SPLIT=0 (read once per process: a child) the same bits come out
        shards=dict(case=dict(n_layers=3), worlds=(2, 8), B=64, split_child=True),
    ),
    "esm2_15b": dict(
        hd=128, shape=(5120, 48, 40, 20480), max_heads=40, cut=(256, 2), other_table=64,
        v2_file=dict(cut=dict(d_model=256, n_layers=2, d_ffn=1024), shape=(256, 2, 2, 1024)),    # two heads of 128
        # a deeper small model: 4 layers x 256, two heads of 128
        case=dict(n_layers=4, d=256, std=0.045, embed_std=0.2),
        # forward: tests/test_gpu_esm2_15b.py keeps its own (one layer at the full width; std and error over the live tokens; bounds
        # 2.5 x FWD_MEASURED); attention and rotation: its derived-bound tests
        forward=None,
        full=None,                                                               # 48 x 5120: 60 GB of synthetic fp32 weights on the host
        other_archs=dict(d_model=256, n_heads=2),
        sampler={}, seq=LONG_SEQ,
        single_chain=dict(n_layers=3, seed=13),
        # 18 key blocks: one workgroup per CU; 2, 4 and 8 contiguous shards
        shards=dict(case=dict(n_layers=3), worlds=(2, 4, 8), B=64, split_child=False),
    ),
    "esm2_8m": dict(
        hd=16, shape=(320, 6, 20, 1280), max_heads=32, cut=(128, 8), other_table=32,
        v2_file=dict(cut=dict(n_layers=2), shape=(320, 2, 20, 1280)),
        case=dict(n_layers=6, d=320, std=0.03, embed_std=0.15),                 # esm2_t6_8M_UR50D's own shape
        label="6 x 320, 20 heads of 16",
        # q is drawn at 0.5 so that the score's spread is the head-32 test's (0.35 sqrt(32) = 0.5 sqrt(16)); the bounds are that test's
        attention=dict(q_draw=0.5),
        forward=dict(shapes={"": {}}, tol=FWD_TOL_PER_STD, per_std=True, full_size=True),
        full=None,                                                               # the 6 x 320 model of the forward test IS the full size
        auto=dict(case=dict(n_layers=2, d=128), full_synthetic=False),
        other_archs=dict(d_model=128, n_heads=8),
        sampler=dict(n_layers=4), seq=LONG_SEQ,
        single_chain=dict(n_layers=3, seed=13),
        # 64 chains x 20 heads at 18 key blocks (four workgroups per CU: 1024 slots): the whole job is 1280 pairs, a full round and a
        # quarter that the attention launch splits; the 32- and 8-chain shards are partial rounds -- and with PGIBBS_ATTN_SPLIT=0 (read
        # once per process: a child) the same bits come out
        shards=dict(case=dict(n_layers=3), worlds=(2, 8), B=64, split_child=True),
    ),
    "esm2_35m": dict(
        hd=24, shape=(480, 12, 20, 1920), max_heads=32, other_table=32,
        v2_file=dict(cut=dict(n_layers=2), shape=(480, 2, 20, 1920)),
        # the reference forms the exponent i / 12 in double where torch rounds the quotient to float32: one to three ulps apart, within
        # what the HuggingFace fixture allows; the product's rotary_inv_freq(24) is held to torch's bits
        ref_inv_freq_is_torchs=False,
        case=dict(n_layers=2, d=480, std=0.03, embed_std=0.15),
        label="heads of 24",
        # attention and rotation run on the head-32 kernels (150M's tests); the live-width row kernels: tests/test_gpu_esm2_35m.py.
        # The reference runs the NATURAL model (heads of 24, rows of 480 / 96); the engine its embedding in slots of 32 (rows of 640 / 128)
        forward=dict(shapes={"35m": dict(d=480), "4 heads": dict(d=96, d_ffn=256)}, tol=FWD_TOL_PER_STD, per_std=True),
        full=dict(std=0.035, embed_std=0.3, T=258),
        # full_synthetic: models.ESM2_35M(synthetic=True) builds and runs the whole 12 x 480 model.  35M only: the other sizes' tests build
        # no full-size engine here, and this suite builds no engine that was not built before it
        auto=dict(case=dict(d=96, d_ffn=256), full_synthetic=True),
        other_archs=None,                                                        # 24 is no kernel width: test_gpu_esm2_35m.py's refusals
        sampler=dict(n_layers=4), seq=LONG_SEQ,
        single_chain=dict(n_layers=3, seed=13),
        shards=dict(case=dict(n_layers=3), worlds=(2, 4, 8), B=64, split_child=False),
    ),
}
for _cli, _row in SIZES.items():
    _row.update(cli=_cli, base=weights.ESM2_SIZES[_cli]["config"], file=weights.ESM2_SIZES[_cli]["file"],
                wrapper=getattr(models, weights.ESM2_SIZES[_cli]["wrapper"]))

# tests/golden/esm2_hf_<name>.npz (make_golden_esm2.py): the size whose base configuration the fixture's overrides apply to, then
# (d_model, n_heads, n_layers) and the token batch it must hold
HF_FIXTURES = {"small": ("esm2", (256, 4, 4), (3, 66)), "mid": ("esm2", (640, 10, 6), (2, 258)), "hd32": ("esm2_150m", (640, 20, 6), (2, 258)),
               "hd128": ("esm2_15b", (512, 4, 6), (2, 258)), "hd16": ("esm2_8m", (320, 20, 6), (2, 258)), "hd24": ("esm2_35m", (480, 20, 12), (2, 258))}


def having(field):
    """the --model names of the sizes whose row has `field`"""
    return [cli for cli, row in SIZES.items() if row.get(field) is not None]
