"""Every released ESM-2 size on the HIP engine, one suite: the tests that are one item per size, each a body of
tests/_esm2_gpu_common.py run at every size whose row of tests/_esm2_sizes.py has the test, the --model name as the parameter id.  The
engine forward at the released shape in strict mode, precision="auto", the sampler (positions, draws, likelihoods, substitution tables,
hipGraph replay, shards), and the refusals of the rotary and strict attention entries.  The tests with many cases per size (the
head-width kernels against numpy, the forward over the sequence lengths, the HuggingFace fixtures, the other architectures' refusals)
run the same shared bodies from each size's own file, tests/test_gpu_esm2.py and its _3b, _150m, _15b, _8m and _35m siblings, next to
what is peculiar to the size."""
import pytest

import _esm2_gpu_common as common
from _esm2_sizes import having

pytestmark = pytest.mark.gpu


# ---- the attention and rotation kernels of a width -------------------------------------------------------------------------------------
def test_attention_hd_at_64_is_pg_dbg_attention():
    common.check_attention_hd_at_64_is_pg_dbg_attention()


@pytest.mark.parametrize("size", having("attention"))
def test_rope_hd_refuses_one_head_too_many(size):
    common.check_rope_hd_refuses_one_head_too_many(size)


# ---- forward ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", having("full"))
def test_full_size_strict_logits(size):
    common.check_full_size_strict_logits(size)


@pytest.mark.parametrize("size", having("auto"))
def test_auto_precision_and_synthetic_default(size):
    common.check_auto_precision(size)


# ---- the sampler --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", having("sampler"))
def test_sampler_positions_draws_and_likelihoods(size):
    common.check_sampler(size)


@pytest.mark.parametrize("size", having("single_chain"))
def test_single_chain_replays_a_graph_and_equals_the_eager_loop(size):
    common.check_single_chain(size)


@pytest.mark.parametrize("size", having("shards"))
def test_shards_reproduce_the_whole_job(size):
    common.check_shards(size)
