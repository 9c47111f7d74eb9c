"""Every released ESM-2 size on the host, one suite over the rows of tests/_esm2_sizes.py (the --model name is the parameter id): the
tests that are one item per size, each a body of tests/_esm2_cpu_common.py -- the configuration's values, and a v2 checkpoint file with
heads of the size's width: the round trip, the inv_freq check, the wrapper.  The rotary frequencies, that file's refusal by every other
size's configuration and the command-line model maps run the same shared bodies from each size's own file, tests/test_esm2_cpu.py and
its _3b, _150m, _15b, _8m and _35m siblings, next to what is peculiar to the size.  Needs no GPU."""
import pytest

import _esm2_cpu_common as common
from _esm2_sizes import SIZES, having


# 650M and 35M keep their own: test_esm2_cpu.py::test_config_and_tensor_names, test_esm2_35m_cpu.py::test_t12_config_values_and_the_embedded_table
@pytest.mark.parametrize("size", [s for s in SIZES if s not in ("esm2", "esm2_35m")])
def test_config_values(size):
    common.check_config_values(size)


@pytest.mark.parametrize("size", having("v2_file"))
def test_v2_round_trip_with_heads_of_the_width(size, tmp_path_factory):
    common.check_v2_round_trip(size, tmp_path_factory)


@pytest.mark.parametrize("size", having("v2_file"))
def test_inv_freq_check_at_the_width(size, tmp_path_factory, tmp_path):
    common.check_inv_freq_check(size, tmp_path_factory, tmp_path)


@pytest.mark.parametrize("size", having("v2_file"))
def test_models_wrapper_reads_a_v2_file_without_a_gpu(size, tmp_path_factory):
    common.check_wrapper_reads_a_v2_file(size, tmp_path_factory)
