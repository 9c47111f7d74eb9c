"""Masked-marginal substitution tables, the parts that need no GPU: the three C-ABI entries are declared and bound, the device-pointer
entry refuses bad arguments on the host, the mask bins of probs_single follow CPython's random.shuffle, mutation strings, both
command lines' parsers and table writers, and the 'no CPU implementation' errors."""
import io
import os
import random
import re
import warnings

import numpy as np
import pytest

from protein_gibbs_sampler_amd import _lib, esm_msa_sampler, esm_sampler, models, pgen_msa_seq_probs, seq_probs_esm, weights
from protein_gibbs_sampler_amd.esm_msa_sampler import partition

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pg_logprob_table_device", "pg_esm_forward_logprob_table", "pg_msa_forward_logprob_table")


def test_header_and_signature_table_hold_the_three_entries():
    hdr = open(os.path.join(ROOT, "include", "pgibbs.h")).read()
    declared = set(re.findall(r"\b(pg_[a-z0-9_]+)\s*\(", hdr))
    bound = {n: a for n, _, a in _lib.SIGNATURES}
    for name in ENTRIES:
        assert name in declared and name in bound and hasattr(_lib.lib(), name)
    assert len(bound["pg_logprob_table_device"]) == 14 and len(bound["pg_esm_forward_logprob_table"]) == 13
    assert len(bound["pg_msa_forward_logprob_table"]) == 14
    assert "#define PG_TABLE_NORM_VOCAB 0" in hdr and "#define PG_TABLE_NORM_COLUMNS 1" in hdr
    assert _lib.TABLE_NORMS == {"vocab": 0, "columns": 1}
    for cite in ("pgen_msa_seq_probs.py:31-45", "esm_sampler.py:340-345"):
        assert cite in hdr


def _table(V=33, n_cols=20, norm=0, n_sel=2, P=3, logits=True, idx=True, cols=True, out=True, width=4):
    # the pointers are never dereferenced on the host: any non-null value stands for a device buffer in the refusal tests
    buf = np.zeros(16, dtype=np.float32)
    p = lambda on: _lib.ptr(buf) if on else None
    L = _lib.lib()
    rc = L.pg_logprob_table_device(None, p(logits), 8, width, V, p(idx), None, n_sel, P, p(cols), n_cols, norm, p(out), None)
    return rc, L.pg_last_error().decode()


@pytest.mark.parametrize("kw,msg", [
    (dict(V=0), "V must be in 1..64"), (dict(V=65, n_cols=20), "V must be in 1..64"),
    (dict(n_cols=0), "n_cols must be in 1..V"), (dict(n_cols=34), "n_cols must be in 1..V"),
    (dict(norm=2), "unknown norm"), (dict(norm=-1), "unknown norm"),
    (dict(n_sel=-1), "negative count"), (dict(P=-1), "negative count"),
    (dict(logits=False), "null argument"), (dict(idx=False), "null argument"), (dict(cols=False), "null argument"),
    (dict(out=False), "null argument"), (dict(width=0), "bad shape")])
def test_table_device_entry_refuses_on_the_host(kw, msg):
    rc, err = _table(**kw)
    assert rc == _lib.PG_ERR_INVALID and msg in err, (rc, err)


def test_table_device_entry_without_a_device_answers_as_the_gather_entry():
    L = _lib.lib()
    if L.pg_device_count() > 0:
        pytest.skip("GPU present")
    buf = np.zeros(16, dtype=np.float32)
    b = _lib.ptr(buf)
    assert L.pg_logprob_table_device(None, b, 8, 4, 33, b, None, 0, 3, b, 20, 0, b, None) == _lib.PG_OK      # nothing to do
    assert L.pg_logprob_gather_device(None, b, 8, 4, 33, b, None, b, 0, 3, b) == _lib.PG_OK
    want = L.pg_logprob_gather_device(None, b, 8, 4, 33, b, None, b, 2, 3, b)
    got = L.pg_logprob_table_device(None, b, 8, 4, 33, b, None, 2, 3, b, 20, 0, b, None)
    assert want != _lib.PG_OK and got == want


def _msa_sampler_cpu():
    cfg = weights.make_config(weights.MSA1B_CONFIG, d_model=128, n_layers=1, d_ffn=256, max_positions=40, max_msa_rows=8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return esm_msa_sampler.ESM_MSA_sampler(models.ESM_MSA1(state_dict=weights.synthetic_state_dict(cfg, seed=1), config=cfg), device="cpu")


def _esm_sampler_cpu():
    cfg = weights.make_config(weights.ESM1B_CONFIG, d_model=128, n_layers=1, d_ffn=256, max_positions=40)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return esm_sampler.ESM_sampler(models.ESM1b(state_dict=weights.synthetic_state_dict(cfg, seed=1), config=cfg), device="cpu")


@pytest.mark.parametrize("steps", [1, 3, 10, 15])       # 1, 3, L, L + 5 for L = 10
def test_probs_single_bins_follow_cpythons_shuffle(steps):
    s, L = _msa_sampler_cpu(), 10
    random.seed(7)
    want = list(range(1, L + 1))
    random.shuffle(want)
    state = random.getstate()
    random.seed(7)
    got = s._probs_single_bins(L, steps)
    assert got == partition(want, steps) and random.getstate() == state
    assert sorted(p for b in got for p in b) == list(range(1, L + 1)) and len(got) == min(steps, L)
    random.seed(7)
    assert s._probs_single_bins(L, None) == partition(want, L)          # None: one bin per position


def test_parse_mutation_and_wild_type_mismatch():
    assert esm_sampler.parse_mutation("A24G") == ("A", 23, "G")
    assert esm_sampler.parse_mutation(" m1k ") == ("M", 0, "K")
    for bad in ("A0G", "24G", "A24", "AG", "A24GG", "B24G", "A24X", "A-3G", "", None, 24):
        with pytest.raises(ValueError, match="Invalid mutation"):
            esm_sampler.parse_mutation(bad)
    s = _esm_sampler_cpu()
    with pytest.raises(ValueError, match=r"'C2G'.*has 'R' at position 2, not 'C'"):
        s.score_mutations("MRHGD", ["M1A", "C2G"])
    with pytest.raises(ValueError, match=r"'D9A'.*beyond the sequence of 5"):
        s.score_mutations("MRHGD", ["D9A"])
    assert s.score_mutations("MRHGD", []) == []
    with pytest.raises(RuntimeError, match="no CPU implementation"):       # valid mutations reach the table, which needs the GPU
        s.score_mutations("MRHGD", ["M1A"])


def test_cpu_devices_raise_the_no_cpu_implementation_error():
    e, m = _esm_sampler_cpu(), _msa_sampler_cpu()
    msa = ["ACDEFGHIKL", "AC-EFGHIKL"]
    state = random.getstate()
    for call in (lambda: e.masked_marginals("ACDEFGHIKL"), lambda: next(e.masked_marginals_batch(["ACDEFGHIKL"])),
                 lambda: m.probs_single(msa, show_progress_bar=False), lambda: next(m.masked_marginals_batch([msa]))):
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            call()
    assert random.getstate() == state                                       # refused before the shuffle


def test_unknown_normalisation_is_refused_by_name():
    lm = _esm_sampler_cpu().model.model
    with pytest.raises(ValueError, match="normalise must be 'vocab' or 'columns'"):
        lm.forward_logprob_table(np.zeros((1, 4), np.int32), [0], [[1]], [4, 5], normalise="softmax")


def test_both_parsers():
    a = pgen_msa_seq_probs.build_parser().parse_args(["--msa", "in.a2m", "-o", "out.tsv"])
    assert (a.msa, a.o, a.steps, a.model, a.device, a.precision, a.synthetic_weights, a.batch_size) == \
        ("in.a2m", "out.tsv", None, "esm_msa1", "gpu", "auto", False, None)
    a = pgen_msa_seq_probs.build_parser().parse_args(["--msa", "x", "-o", "y", "--steps", "4", "--device", "cuda:1", "--precision", "fp32",
                                                      "--synthetic-weights", "--seed", "3"])
    assert (a.steps, a.device, a.precision, a.synthetic_weights, a.seed) == (4, "cuda:1", "fp32", True, 3)
    for argv in (["-o", "y"], ["--msa", "x"], ["--msa", "x", "-o", "y", "--model", "esm1b"]):
        with pytest.raises(SystemExit):
            pgen_msa_seq_probs.build_parser().parse_args(argv)
    b = seq_probs_esm.build_parser().parse_args([])
    assert (b.i, b.o, b.model, b.device, b.mask_distance, b.batch_size, b.masking_off, b.normalise, b.csv) == \
        (None, None, "esm1v", "gpu", None, None, False, "vocab", False)
    b = seq_probs_esm.build_parser().parse_args(["-i", "a.fa", "-o", "t.tsv", "--mask_distance", "6", "--batch_size", "2", "--model", "esm2",
                                                 "--normalise", "columns", "--checkpoint", "w.pt"])
    assert (b.i, b.o, b.mask_distance, b.batch_size, b.model, b.normalise, b.checkpoint) == ("a.fa", "t.tsv", 6, 2, "esm2", "columns", "w.pt")
    with pytest.raises(ValueError, match="both set"):
        seq_probs_esm.cli(["--masking_off", "--mask_distance", "3"])
    with pytest.raises(ValueError, match=">= 1"):
        seq_probs_esm.cli(["--mask_distance", "0"])


def test_msa_probability_table_writer_by_hand():
    toks, target = ["-", "A", "C"], "CAC-"
    probs = np.asarray([[0.1, 0.2, 0.25, 0.5], [0.2, 0.7, 0.5, 0.25], [0.7, 0.1, 0.25, 0.25]], dtype=np.float32)
    buf = io.StringIO()
    pgen_msa_seq_probs.write_table(buf, probs, toks, target)
    lines = buf.getvalue().split("\n")
    assert lines[0] == "\tC\tA\tC\t-" and lines[1] == "-\t0.1\t0.2\t0.25\t0.5" and lines[3] == "C\t0.69999999\t0.1\t0.25\t0.25"
    assert lines[4:] == ["position\t1\t2\t3\t4", "consensus\tC\tA\tA\t-", "different\t0\t0\t1\t0", ""]
    back = pgen_msa_seq_probs.read_table(io.StringIO(buf.getvalue()))
    assert back["target"] == target and back["toks"] == toks and back["position"] == [1, 2, 3, 4]
    assert back["consensus"] == "CAA-" and back["different"] == [0, 0, 1, 0]
    assert np.array_equal(back["probs"].astype(np.float32), np.asarray([[float("%.8g" % v) for v in r] for r in probs], dtype=np.float32))
    with pytest.raises(ValueError, match=r"expected a \[3, 5\] table"):
        pgen_msa_seq_probs.table_rows(probs, toks, "CAC-A")


def test_substitution_table_writer_by_hand():
    import csv
    toks = list("LAGV")
    buf = io.StringIO()
    w = csv.writer(buf, delimiter="\t", lineterminator="\n")
    seq_probs_esm.write_header(w, toks)
    logp = np.log(np.asarray([[0.5, 0.25, 0.125, 0.125], [0.25, 0.25, 0.25, 0.25]], dtype=np.float32))
    seq_probs_esm.write_rows(w, "q1", "LG", logp, np.asarray([1.2130076, 1.3862944], dtype=np.float32))
    seq_probs_esm.write_rows(w, "q2", "V", logp[1:], np.asarray([1.3862944], dtype=np.float32))
    lines = buf.getvalue().split("\n")
    assert lines[0] == "id\tposition\twt\tL\tA\tG\tV\tentropy"
    assert lines[1] == "q1\t1\tL\t-0.69314718\t-1.3862944\t-2.0794415\t-2.0794415\t1.2130076"
    assert lines[3] == "q2\t1\tV\t-1.3862944\t-1.3862944\t-1.3862944\t-1.3862944\t1.3862944" and lines[4] == ""
    got_toks, table = seq_probs_esm.read_table(io.StringIO(buf.getvalue()))
    assert got_toks == toks and sorted(table) == ["q1", "q2"] and table["q1"]["seq"] == "LG" and table["q2"]["seq"] == "V"
    assert np.allclose(table["q1"]["logp"], logp, rtol=1e-7) and table["q1"]["entropy"] == [1.2130076, 1.3862944]
    with pytest.raises(ValueError, match="not a substitution table"):
        seq_probs_esm.read_table(io.StringIO("id\tscore\nq\t1\n"))
