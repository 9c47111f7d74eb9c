"""Plan and launch agree: with profiling on, an engine forward records under "attention" exactly the text `pg_dbg_attention_plan`
gives for the shape and the device's own CU count (tests/test_attention_plan_cpu.py pins those texts for 256 CUs)."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from protein_gibbs_sampler_amd import _lib, models, weights

pytestmark = pytest.mark.gpu


def _plan(precision, n_seq, T, H, pad):
    buf = ctypes.create_string_buffer(256)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    _lib.check(_lib.lib().pg_dbg_attention_plan(0, precision, n_seq, T, 0, H, 64, pad, 0, 1, 0, n_cu, buf, len(buf)))
    return buf.value.decode()


# a 32-chain shard (the last round is split), a ragged batch (<pad> mask), strict mode at config 2's length
@pytest.mark.parametrize("precision,B,T,ragged", [("bf16", 32, 258, False), ("bf16", 3, 100, True), ("fp16", 33, 258, False), ("fp32", 2, 258, False)])
def test_forward_records_the_plan(precision, B, T, ragged):
    cfg = weights.make_config(weights.ESM1B_CONFIG, n_layers=2)
    sd = weights.synthetic_state_dict(cfg, seed=3, std=0.03, embed_std=0.05, ln_jitter=0.1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lm = models.ESM1b(state_dict=sd, config=cfg, precision=precision).model.to("cuda:0")
    tok = np.random.default_rng(1).integers(4, 24, (B, T))
    tok[:, 0] = 0
    if ragged:
        tok[1, 60:] = 1
        tok[2, 17:] = 1
    lm.prof_enable(True)
    lm.prof_reset()
    lm.forward_logits(tok)
    recorded = lm.prof_get_kernels("attention")
    lm.prof_enable(False)
    want = _plan({"bf16": _lib.PG_PREC_BF16, "fp16": _lib.PG_PREC_F16, "fp32": _lib.PG_PREC_FP32}[precision], B, T, cfg["n_heads"], int(ragged))
    print("\n[%s %d x %d%s] attention: %s" % (precision, B, T, " ragged" if ragged else "", recorded))
    assert recorded == want and not want.startswith("error")
