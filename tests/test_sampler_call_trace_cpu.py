"""What the samplers hand to the engine, call by call, pinned as digests: ESM_sampler and ESM_MSA_sampler are driven through the
recording fake engine of _fake_engine.py, and for every case one sha256 covers the trace (method names, every array's dtype, shape
and bytes, the scalars, every SampleParams field, the set_job_items sequence), the returned value, the interpreter's and torch's
RNG right after the call, and the sampler's last_run.  The fake's answers are functions of its inputs, so the host arithmetic
behind the calls (float32 summation order, table placement) is in the digest too.

The constants were taken on the commit before the samplers' shared helpers existed (one batch runner, one padded table, one
strided-mask builder) and must never be regenerated from a tree whose sampler code is the thing under test."""
import hashlib
import itertools
import random

import numpy as np
import pytest
import torch

from protein_gibbs_sampler_amd import esm_msa_sampler, esm_sampler
from _fake_engine import fake_engine_model

_TEMPLATES = [["MEPAATGQ", "MEP-ATGQ", "MKPAATGQ"], ["MEPAATGQ", "MEP-ATGQ", "MKPAATGQ"], ["ACDEFGHIKLMN", "ACDEFGHIKLMN"],
              ["MEPAATGA", "MEP-ATGC", "MKPAATGD"], ["ACD", "ACE"]]
_EXCL = [None, [0, 3], [], [1], None]
ESM_SEEDS = ["MEPAATGQEAEECAHSGRGEAW", "MKPAATGQEA"]
ESM_SEQS = ["MEPAA", "MKPAATGQ", "W"]                                       # lengths 5, 8, 1
MSA2 = ["MEPAATGQ", "MEP-ATGQ"]
GAPPED = ["ME-AAT-Q", "MEPAATGQ", "MKPA-TGQ"]                               # the target row (0) has gaps
RAGGED = [["MEPAATGQ", "MEP-ATGQ", "MKPAATGQ"], ["ACD-FG", "ACDEFG"], ["-KPAATG-", "MEPAATGQ", "MEPA-TGQ"]]     # depths 3, 2, 3
ALL_GAP = ["----", "ACDE"]


def _canon(x):
    """Anything the samplers return or record, as nested tuples of plain values (arrays by dtype, shape and bytes)."""
    if hasattr(x, "numpy") and not isinstance(x, np.ndarray):
        x = x.numpy()
    if isinstance(x, np.ndarray):
        return ("array", x.dtype.str, x.shape, hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest())
    if isinstance(x, dict):
        return ("dict",) + tuple((k, _canon(x[k])) for k in sorted(x))
    if isinstance(x, (list, tuple)):
        return (type(x).__name__,) + tuple(_canon(v) for v in x)
    if isinstance(x, (float, np.floating)):
        return ("float", np.float64(x).tobytes().hex())
    return repr(x)


def _sampler(msa, device="gpu"):
    cls = esm_msa_sampler.ESM_MSA_sampler if msa else esm_sampler.ESM_sampler
    return cls(fake_engine_model(msa), device=device)


def _digest(seed, run, msa, record=False):
    """run(sampler) under fixed seeds -> 16 hex digits over (trace, result or exception, both RNGs afterwards, last_run)."""
    s = _sampler(msa)
    s.record = record
    random.seed(seed)
    torch.manual_seed(seed + 1000)
    try:
        result = _canon(run(s))
    except Exception as e:                      # noqa: BLE001  (the exception's type and text are what is pinned)
        result = ("raised", type(e).__name__, str(e))
    after = (random.getrandbits(32), int(torch.randint(0, 2**31, (1,)).item()))
    return hashlib.sha256(repr((s.model.model.trace, result, after, _canon(s.last_run))).encode()).hexdigest()[:16]


def _drain(gen):
    return list(gen)


CASES = {}


def _case(name, msa, record=False):
    def add(fn):
        CASES[name] = (len(CASES), fn, msa, record)
        return fn
    return add


# ---- ESM_sampler.generate ---------------------------------------------------------------------------------------------------------
_GEN = dict(batch_size=5, num_iters=3, num_positions=4, show_progress_bar=False)
_case("esm_generate", False)(lambda s: s.generate(9, list(ESM_SEEDS), **_GEN))
_case("esm_generate_in_order", False)(lambda s: s.generate(9, list(ESM_SEEDS), in_order=True, leader_length=2, **_GEN))
_case("esm_generate_all_positions", False)(lambda s: s.generate(9, list(ESM_SEEDS), **dict(_GEN, num_positions=0)))
_case("esm_generate_indexes", False)(lambda s: s.generate(9, list(ESM_SEEDS), indexes=[3, -2, 3, 7], **_GEN))
_case("esm_generate_record", False, record=True)(lambda s: s.generate(9, list(ESM_SEEDS), **_GEN))

# ---- ESM_MSA_sampler.generate -----------------------------------------------------------------------------------------------------
_MGEN = dict(batch_size=3, num_iters=2, num_positions=3, show_progress_bar=False)
_case("msa_generate", True)(lambda s: s.generate(11, list(MSA2), **_MGEN))
_case("msa_generate_in_order", True)(lambda s: s.generate(11, list(MSA2), in_order=True, **_MGEN))
_case("msa_generate_percent", True)(lambda s: s.generate(11, list(MSA2), num_positions_percent=50, **_MGEN))
_case("msa_generate_record", True, record=True)(lambda s: s.generate(11, list(MSA2), **_MGEN))

# ---- generate_single_batch / generate_single ------------------------------------------------------------------------------------
for _mb in (1, 2, 4):
    _case("single_batch_max%d" % _mb, True, record=True)(
        lambda s, mb=_mb: s.generate_single_batch(_TEMPLATES, steps=3, passes=2, burn_in=1, target_index=-1, k=1,
                                                  exclude_positions=_EXCL, max_batch=mb))
_case("single", True, record=True)(lambda s: s.generate_single(_TEMPLATES[3], steps=3, passes=2, burn_in=1, target_index=-1, k=1,
                                                              exclude_positions=[1]))

# ---- ESM_sampler.log_likelihood_batch / masked_marginals_batch --------------------------------------------------------------------
for _md, _bs in itertools.product((1, 3, float("inf")), (None, 2)):
    _case("esm_loglik_md%s_bs%s" % (_md, _bs), False)(
        lambda s, md=_md, bs=_bs: _drain(s.log_likelihood_batch(ESM_SEQS, with_masking=True, mask_distance=md, batch_size=bs)))
    for _norm in ("vocab", "columns"):
        _case("esm_marginals_md%s_bs%s_%s" % (_md, _bs, _norm), False)(
            lambda s, md=_md, bs=_bs, norm=_norm: _drain(s.masked_marginals_batch(ESM_SEQS, with_masking=True, mask_distance=md,
                                                                                  batch_size=bs, normalise=norm)))
for _bs in (None, 2):
    _case("esm_loglik_unmasked_bs%s" % _bs, False)(
        lambda s, bs=_bs: _drain(s.log_likelihood_batch(ESM_SEQS, with_masking=False, batch_size=bs)))
    for _norm in ("vocab", "columns"):
        _case("esm_marginals_unmasked_bs%s_%s" % (_bs, _norm), False)(
            lambda s, bs=_bs, norm=_norm: _drain(s.masked_marginals_batch(ESM_SEQS, with_masking=False, batch_size=bs, normalise=norm)))

# ---- ESM_MSA_sampler.log_likelihood_batch / masked_marginals_batch ----------------------------------------------------------------
for _gaps, _md, _bs in itertools.product((False, True), (2, float("inf")), (1, 2)):
    _case("msa_loglik_gaps%d_md%s_bs%d" % (_gaps, _md, _bs), True)(
        lambda s, g=_gaps, md=_md, bs=_bs: _drain(s.log_likelihood_batch([GAPPED, MSA2], count_gaps=g, mask_distance=md, batch_size=bs)))
    _case("msa_marginals_gaps%d_md%s_bs%d" % (_gaps, _md, _bs), True)(
        lambda s, g=_gaps, md=_md, bs=_bs: _drain(s.masked_marginals_batch([GAPPED, MSA2], count_gaps=g, mask_distance=md, batch_size=bs)))
for _ti in (0, -1):
    _case("msa_loglik_unmasked_ragged_ti%d" % _ti, True)(
        lambda s, ti=_ti: _drain(s.log_likelihood_batch(RAGGED, target_index=ti, with_masking=False, batch_size=2)))
    _case("msa_marginals_unmasked_ragged_ti%d" % _ti, True)(
        lambda s, ti=_ti: _drain(s.masked_marginals_batch(RAGGED, target_index=ti, with_masking=False, batch_size=2, normalise="columns")))
_case("msa_loglik_all_gap_masked", True)(lambda s: _drain(s.log_likelihood_batch([ALL_GAP], count_gaps=False)))
_case("msa_loglik_all_gap_unmasked", True)(lambda s: _drain(s.log_likelihood_batch([ALL_GAP], with_masking=False, count_gaps=False)))

# ---- probs_single -----------------------------------------------------------------------------------------------------------------
for _steps, _bs, _ti in itertools.product((None, 3), (None, 2), (-1, 0)):
    _case("probs_single_steps%s_bs%s_ti%d" % (_steps, _bs, _ti), True)(
        lambda s, st=_steps, bs=_bs, ti=_ti: s.probs_single(GAPPED, steps=st, target_index=ti, show_progress_bar=False, batch_size=bs))

EXPECTED = {
    "esm_generate": "656dd0d7a5323323",
    "esm_generate_in_order": "5823c8f56862376a",
    "esm_generate_all_positions": "96b81f8ae19d9ad4",
    "esm_generate_indexes": "27ae4b3e8ecb3093",
    "esm_generate_record": "8fb5b39a14908d6c",
    "msa_generate": "926e3beacfa5e4bb",
    "msa_generate_in_order": "c7e8020d9c7b5062",
    "msa_generate_percent": "4eb6a9f6631b118d",
    "msa_generate_record": "42b1e0857e60b925",
    "single_batch_max1": "c0b0851e5cbfc5c2",
    "single_batch_max2": "a6038098390b62ed",
    "single_batch_max4": "f3da95bdd8a3ca9f",
    "single": "cf2e6f3672cd1c5d",
    "esm_loglik_md1_bsNone": "0d6c8692364052ca",
    "esm_marginals_md1_bsNone_vocab": "af61d0b9ef547cde",
    "esm_marginals_md1_bsNone_columns": "2848d2056f3b4c61",
    "esm_loglik_md1_bs2": "7753168be3bbbc68",
    "esm_marginals_md1_bs2_vocab": "e54a7310ca1d42da",
    "esm_marginals_md1_bs2_columns": "ba17693b9248bf5f",
    "esm_loglik_md3_bsNone": "47c20f4506a880f8",
    "esm_marginals_md3_bsNone_vocab": "4c20f00167066227",
    "esm_marginals_md3_bsNone_columns": "d6d986339d7ff09d",
    "esm_loglik_md3_bs2": "505db1039037852c",
    "esm_marginals_md3_bs2_vocab": "0dda0ef818a70d1c",
    "esm_marginals_md3_bs2_columns": "5dfa05c7b1ed9b41",
    "esm_loglik_mdinf_bsNone": "f25116c036b5247e",
    "esm_marginals_mdinf_bsNone_vocab": "669a298256cfbea5",
    "esm_marginals_mdinf_bsNone_columns": "a0049d81be4af61d",
    "esm_loglik_mdinf_bs2": "8631737ea989777e",
    "esm_marginals_mdinf_bs2_vocab": "f275375b72c3790c",
    "esm_marginals_mdinf_bs2_columns": "1573bf34b0c67929",
    "esm_loglik_unmasked_bsNone": "f5e936dba89fb458",
    "esm_marginals_unmasked_bsNone_vocab": "174532def9d8ea02",
    "esm_marginals_unmasked_bsNone_columns": "78016a6cc94379a5",
    "esm_loglik_unmasked_bs2": "c80b604609a196e1",
    "esm_marginals_unmasked_bs2_vocab": "082b7f570d967161",
    "esm_marginals_unmasked_bs2_columns": "f16aaeb46a7429dc",
    "msa_loglik_gaps0_md2_bs1": "01be34d6ad7c6e13",
    "msa_marginals_gaps0_md2_bs1": "ade55283ad9d79a1",
    "msa_loglik_gaps0_md2_bs2": "c584c1f37af8c8b5",
    "msa_marginals_gaps0_md2_bs2": "21250b3e82586e86",
    "msa_loglik_gaps0_mdinf_bs1": "cb0d77d92d55d0a1",
    "msa_marginals_gaps0_mdinf_bs1": "f54cae91a184a07d",
    "msa_loglik_gaps0_mdinf_bs2": "01dc38080457f699",
    "msa_marginals_gaps0_mdinf_bs2": "c104782a76f49ba0",
    "msa_loglik_gaps1_md2_bs1": "67319c0e431dcc05",
    "msa_marginals_gaps1_md2_bs1": "4be8a3cb89bdcea8",
    "msa_loglik_gaps1_md2_bs2": "fbf8d7aa70976557",
    "msa_marginals_gaps1_md2_bs2": "098b6c18f42013d3",
    "msa_loglik_gaps1_mdinf_bs1": "2abecc4f4572c9dc",
    "msa_marginals_gaps1_mdinf_bs1": "90a1071a8993b7f4",
    "msa_loglik_gaps1_mdinf_bs2": "d27df564b4fb44b3",
    "msa_marginals_gaps1_mdinf_bs2": "f33f323c0707c4e1",
    "msa_loglik_unmasked_ragged_ti0": "5b36cb97fe51db52",
    "msa_marginals_unmasked_ragged_ti0": "0eb115ca1cc080b9",
    "msa_loglik_unmasked_ragged_ti-1": "37265d9909c015b3",
    "msa_marginals_unmasked_ragged_ti-1": "a2dd0a3898abd09f",
    "msa_loglik_all_gap_masked": "56ff99b352a54439",
    "msa_loglik_all_gap_unmasked": "c91ac80ab3c6cf5e",
    "probs_single_stepsNone_bsNone_ti-1": "f8a49a8c6a69d54f",
    "probs_single_stepsNone_bsNone_ti0": "feb4d08673070b41",
    "probs_single_stepsNone_bs2_ti-1": "c91e67ab0ed1d05b",
    "probs_single_stepsNone_bs2_ti0": "8ca1ef06eb547601",
    "probs_single_steps3_bsNone_ti-1": "642cc51dcfe4c413",
    "probs_single_steps3_bsNone_ti0": "4912043b788c1a5e",
    "probs_single_steps3_bs2_ti-1": "27a15175f7946bc7",
    "probs_single_steps3_bs2_ti0": "5fba4c70d5a78f1b",
}


@pytest.mark.parametrize("name", list(CASES))
def test_call_trace_digest(name, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    seed, run, msa, record = CASES[name]
    assert _digest(seed, run, msa, record) == EXPECTED[name]


def test_probs_single_brackets_its_chunks_with_the_job_size(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    s = _sampler(True)
    random.seed(0)
    s.probs_single(GAPPED, steps=3, show_progress_bar=False, batch_size=2)
    names = [t[0] for t in s.model.model.trace]
    assert names == ["set_job_items", "forward_logprob_table", "forward_logprob_table", "set_job_items"]
    assert s.model.model.job_items == [3, 0]


# ---- the no-GPU refusals of every public method on device="cpu", by message text -----------------------------------------------
_ESM_NO_GPU = "ESM_sampler.%s needs device 'gpu'/'cuda:N' on an MI355X: there is no CPU implementation"
_MSA_NO_GPU = ("ESM_MSA_sampler.%s needs device 'gpu'/'cuda:N' on an MI355X: the Gibbs hot path is implemented as HIP kernels only, "
               "there is no CPU implementation")
NO_GPU = [
    (False, lambda s: s.generate(2, "MEPAA", show_progress_bar=False),
     "ESM_sampler.generate needs device 'gpu'/'cuda:N' on an MI355X: this package implements the Gibbs hot path as HIP kernels only "
     "and has no CPU implementation"),
    (False, lambda s: s.log_likelihood("MEPAA"), _ESM_NO_GPU % "log_likelihood_batch"),
    (False, lambda s: _drain(s.log_likelihood_batch(ESM_SEQS)), _ESM_NO_GPU % "log_likelihood_batch"),
    (False, lambda s: s.masked_marginals("MEPAA"), _ESM_NO_GPU % "masked_marginals_batch"),
    (False, lambda s: _drain(s.masked_marginals_batch(ESM_SEQS, normalise="softmax")), _ESM_NO_GPU % "masked_marginals_batch"),
    (False, lambda s: s.score_mutations("MEPAA", ["M1A"]), _ESM_NO_GPU % "masked_marginals_batch"),
    (True, lambda s: s.generate(2, MSA2, show_progress_bar=False), _MSA_NO_GPU % "generate"),
    (True, lambda s: s.generate_single(MSA2), _MSA_NO_GPU % "generate_single"),
    (True, lambda s: s.generate_single_batch([MSA2]), _MSA_NO_GPU % "generate_single"),
    (True, lambda s: s.log_likelihood(MSA2), _MSA_NO_GPU % "log_likelihood_batch"),
    (True, lambda s: _drain(s.log_likelihood_batch([MSA2])), _MSA_NO_GPU % "log_likelihood_batch"),
    (True, lambda s: _drain(s.masked_marginals_batch([MSA2], normalise="softmax")), _MSA_NO_GPU % "masked_marginals_batch"),
    (True, lambda s: s.probs_single(MSA2, show_progress_bar=False), _MSA_NO_GPU % "probs_single"),
]


@pytest.mark.parametrize("case", range(len(NO_GPU)))
def test_cpu_device_refusals_word_for_word(case):
    msa, call, text = NO_GPU[case]
    s = _sampler(msa, device="cpu")
    random.seed(4)
    state, tstate = random.getstate(), torch.get_rng_state()
    with pytest.raises(RuntimeError) as e:
        call(s)
    assert str(e.value) == text
    assert random.getstate() == state and torch.equal(torch.get_rng_state(), tstate)      # refused before any draw
    assert s.model.model.trace == []


# ---- refusals that are decided on the host before any engine call, by message text -------------------------------------------
_NORMALISE = "normalise must be 'vocab' or 'columns', got 'softmax'"
REFUSALS = [
    (False, lambda s: _drain(s.masked_marginals_batch(ESM_SEQS, normalise="softmax")), ValueError, _NORMALISE),
    (True, lambda s: _drain(s.masked_marginals_batch([MSA2], normalise="softmax")), ValueError, _NORMALISE),
    (True, lambda s: s.generate_single_batch(_TEMPLATES, exclude_positions=[None]), ValueError,
     "exclude_positions: expected one list (or None) per MSA"),
    (True, lambda s: s.generate_single(MSA2, target_index=2), IndexError, "index 2 is out of bounds for dimension 0 with size 2"),
    (True, lambda s: s.generate_single(MSA2, target_index=-3), IndexError, "index -3 is out of bounds for dimension 0 with size 2"),
    (True, lambda s: s.probs_single(MSA2, target_index=5, show_progress_bar=False), IndexError,
     "index 5 is out of bounds for dimension 0 with size 2"),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_host_side_refusals_word_for_word(case, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    msa, call, exc, text = REFUSALS[case]
    s = _sampler(msa)
    random.seed(4)
    state = random.getstate()
    with pytest.raises(exc) as e:
        call(s)
    assert str(e.value) == text and random.getstate() == state and s.model.model.trace == []


if __name__ == "__main__":          # prints the table of digests of the tree it is run in (see the module docstring before using it)
    torch.cuda.is_available = lambda: True
    torch.cuda.device_count = lambda: 1
    for _name, (_seed, _run, _msa, _record) in CASES.items():
        print('    "%s": "%s",' % (_name, _digest(_seed, _run, _msa, _record)))
