"""ESM-2 150M (esm2_t30_150M_UR50D: heads of 32; models.ESM2_150M) on the HIP engine: the head-32 attention kernels alone
(pg_dbg_attention_hd: the whole-sequence ladder, the long-sequence kernel, <pad> keys, three precisions) and the head-32 rotation
(pg_dbg_rope_hd) against numpy, the engine forward against the numpy reference and a HuggingFace fixture, and the refusals of heads of
32 elsewhere -- each the shared body of tests/_esm2_gpu_common.py at this size.  The full-size model, precision="auto" and the sampler
are the esm2_150m rows of tests/test_gpu_esm2_sizes.py."""
import pytest

import _esm2_gpu_common as common
from _esm2_sizes import ATTENTION_H, ATTENTION_T, PRECISIONS, ROPE_H, ROPE_T
from protein_gibbs_sampler_amd import models, weights

pytestmark = pytest.mark.gpu

SIZE = "esm2_150m"


# ---- the shared bodies (tests/_esm2_gpu_common.py) at this size: the head-32 kernels alone, the forward, the refusals elsewhere -------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("H", ATTENTION_H)
@pytest.mark.parametrize("T", ATTENTION_T)
def test_attention_hd32_against_numpy(T, H, precision):
    common.check_attention_hd(SIZE, T, H, precision)


@pytest.mark.parametrize("H", ROPE_H)
@pytest.mark.parametrize("T", ROPE_T)
def test_rope_hd32_against_numpy(T, H):
    common.check_rope_hd(SIZE, T, H)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_esm2_150m_forward_against_the_reference(precision):
    common.check_forward(SIZE, "", precision)


def test_esm2_150m_forward_against_huggingface_logits():
    common.check_huggingface_logits("hd32")


@pytest.mark.parametrize("base, name", [("ESM1B_CONFIG", "ESM-1b"), ("MSA1B_CONFIG", "ESM-MSA-1b"), ("ESM1_T6_CONFIG", "ESM-1")])
def test_engine_refuses_heads_of_32_for_the_other_architectures(base, name):
    assert common.OTHER_ARCHS[name][0] == base
    common.check_other_architectures_refuse_the_width(SIZE, name)


def test_engine_names_the_widths_that_run():
    cfg = weights.make_config(weights.ESM2_T30_CONFIG, n_layers=1, d_model=384, n_heads=16, d_ffn=512, max_positions=40)      # heads of 24
    sd = weights.synthetic_state_dict(cfg, seed=1)
    with pytest.raises(Exception, match=r"head dim must be 64 .* or 32"):
        common.model(models.ESM2_150M, cfg, sd, "bf16").model.to("cuda:0")
