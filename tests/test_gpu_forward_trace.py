"""The launch list of the engine's forward, pinned.  With profiling on, every case below records for each profiling class the pair
(launches, kernel texts) -- `prof_get(c)[1]` and `prof_get_kernels(c)` -- and the pairs must equal tests/golden/forward_trace.json.
The cases are the smallest shapes that reach each branch of csrc/engine.hip's trunks, pruned tail and LM head (DESIGN.md section 16
prints the op sequence each of them walks); two layers, synthetic weights.

The fixture is a recording of the PARENT commit's library, never of the code under test:

    PGIBBS_LIB_PATH=<libpgibbs.so built at the parent commit> python tests/test_gpu_forward_trace.py --record

writes it together with the device's CU count.  The kernel texts hold tile counts, which follow the CU count, so they are compared
only on a device with the recorded count; the launch counts are compared on every device."""
import json
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from protein_gibbs_sampler_amd import _lib, weights  # noqa: E402
from protein_gibbs_sampler_amd.engine import NativeMaskedLM  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forward_trace.json")
CLASSES = ("gemm_other", "gemm_qkv", "gemm_out", "gemm_fc1", "gemm_fc2", "attention", "layernorm", "embed", "head", "sample", "rope")
BASE = {"esm1b": weights.ESM1B_CONFIG, "esm2": weights.ESM2_T33_CONFIG, "esm1": weights.ESM1_T6_CONFIG, "msa1b": weights.MSA1B_CONFIG}


def _tokens(cfg, shape, pad=()):
    tok = np.random.default_rng(1).integers(4, 24, shape).astype(np.int32)
    tok[..., 0] = cfg["cls_idx"]
    for where in pad:
        tok[where] = cfg["pad_idx"]
    return tok


def _params(cfg, seed=5):
    return _lib.make_sample_params(True, cfg["mask_idx"], 0, float("inf"), 1.0, list(range(4, 24)), rng_seed=seed)


def _forward(shape, pad=()):
    return lambda lm: lm.forward_logits(_tokens(lm.cfg, shape, pad))


def _gibbs(shape, iters):
    """gibbs_run, P = 2: positions 3 and 9 of every token row, every iteration."""
    def run(lm):
        idx = np.tile(np.array([3, 9], dtype=np.int32), (iters,) + shape[:-1] + (1,))
        lm.gibbs_run(_tokens(lm.cfg, shape), idx, _params(lm.cfg))
    return run


def _single_batch(lm):
    """generate_single on 2 templates of 4 x 40: two steps, row 3 masked, row 0 sampled at 2 positions."""
    idx = np.tile(np.array([3, 9], dtype=np.int32), (2, 2, 1))
    lm.gibbs_single_batch_run(_tokens(lm.cfg, (2, 4, 40)), 3, 0, idx, [1, 0], [_params(lm.cfg, 5 + b) for b in range(2)])


_S = np.s_
# (architecture, precision, case, call), with the branch of the forward the case is there for
CASES = [
    ("esm1b", "bf16", "forward 3x100", _forward((3, 100))),                                        # tile GEMMs
    ("esm1b", "bf16", "forward 3x100 ragged", _forward((3, 100), (_S[1, 60:], _S[2, 17:]))),       # <pad> key mask
    ("esm1b", "bf16", "gibbs 8x40 P2 x2", _gibbs((8, 40), 2)),                                     # pruned tail on tile GEMMs
    ("esm1b", "bf16", "forward 1x30", _forward((1, 30))),                                          # the whole persistent launch
    ("esm1b", "bf16", "gibbs 1x30 P2 x3", _gibbs((1, 30), 3)),                                     # partial persistent launch + folded pruned tail (eager: profiling)
    ("esm1b", "fp16", "forward 3x100", _forward((3, 100))),
    ("esm1b", "fp32", "forward 2x40", _forward((2, 40))),
    ("esm1b", "fp32", "gibbs 2x40 P2", _gibbs((2, 40), 1)),
    ("esm2", "bf16", "forward 1x30", _forward((1, 30))),                                           # folded LayerNorm per layer, with rotation
    ("esm2", "bf16", "gibbs 1x30 P2", _gibbs((1, 30), 1)),
    ("esm2", "bf16", "forward 3x100", _forward((3, 100))),
    ("esm2", "fp32", "forward 2x40", _forward((2, 40))),
    ("esm1", "bf16", "forward 2x40", _forward((2, 40))),                                           # bias key, untied head
    ("esm1", "fp32", "forward 2x40", _forward((2, 40))),
    ("msa1b", "bf16", "forward 1x4x40", _forward((1, 4, 40))),                                     # column attention unfused
    ("msa1b", "bf16", "forward 1x32x20", _forward((1, 32, 20))),                                   # column attention fused
    ("msa1b", "bf16", "forward 2x4x40 ragged", _forward((2, 4, 40), (_S[1, :, 30:], _S[1, 3, :]))),  # scores through scratch, pad column mask
    ("msa1b", "bf16", "gibbs 1x8x40 P2", _gibbs((1, 8, 40), 1)),                                   # pruned MSA tail
    ("msa1b", "bf16", "single batch 2 x 4x40", _single_batch),
    ("msa1b", "fp32", "forward 1x4x40", _forward((1, 4, 40))),
]
IDS = ["%s-%s %s" % c[:3] for c in CASES]


class _Engines:
    """One engine per (architecture, precision), built on first use and kept for the module."""

    def __init__(self):
        self.made = {}

    def get(self, arch, precision):
        if (arch, precision) not in self.made:
            cfg = weights.make_config(BASE[arch], n_layers=2)
            sd = weights.synthetic_state_dict(cfg, seed=3, std=0.03, embed_std=0.05, ln_jitter=0.1)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                self.made[(arch, precision)] = NativeMaskedLM(cfg, sd, precision).to("cuda:0")
        return self.made[(arch, precision)]


def _trace(lm, call):
    lm.prof_enable(True)
    try:
        lm.prof_reset()
        call(lm)
        return {c: [lm.prof_get(c)[1], lm.prof_get_kernels(c)] for c in CLASSES}
    finally:
        lm.prof_enable(False)


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def engines():
    return _Engines()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("arch,precision,case,call", CASES, ids=IDS)
def test_forward_launch_list(engines, golden, arch, precision, case, call):
    want = golden["cases"]["%s-%s %s" % (arch, precision, case)]
    got = _trace(engines.get(arch, precision), call)
    for c in CLASSES:
        print("%-10s %4d  %s" % (c, got[c][0], got[c][1]))
    assert {c: got[c][0] for c in CLASSES} == {c: want[c][0] for c in CLASSES}
    if _n_cu() == golden["n_cu"]:
        assert got == want


def _record():
    if not os.environ.get("PGIBBS_LIB_PATH"):
        sys.exit("--record: set PGIBBS_LIB_PATH to the parent commit's libpgibbs.so (the fixture is never made with the code under test)")
    engines = _Engines()
    cases = {i: _trace(engines.get(arch, precision), call) for i, (arch, precision, _, call) in zip(IDS, CASES)}
    with open(GOLDEN, "w") as f:
        json.dump({"n_cu": _n_cu(), "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases" % (GOLDEN, len(cases)))


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: PGIBBS_LIB_PATH=<parent build> python tests/test_gpu_forward_trace.py --record")
    _record()
