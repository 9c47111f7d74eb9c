"""Kernel-level parity of the attention kernels on the MI355X, every template form through its debug entry against the float64
reference of tests/_attention_reference.py, element by element under the bound derived there (never a figure fitted to a kernel):

  * attention_kernel / attention_long_kernel at every edge of the key-block ladder, head dimensions 64 and 32, bf16 and fp16 operands,
    plain, with <pad> keys, with ESM-1's bias key and with both, the SPLIT form, on six input families (gaussian, negative scores,
    late maximum on the last key / on the first key of the last 288-key tile, unity, integer-coded v);
  * the strict kernels (split-bf16 MFMA) at their tile edges;
  * the MSA column attention with <pad> rows and an all-<pad> column in the three precisions, the padded tied-row attention on the
    engine's route below and above 576 columns, the plain tied-row attention whole and split over the rows.

Every launch's recorded plan text is compared with pg_dbg_attention_plan's answer for the device's own CU count and with the form the
case is meant to run; the last test checks that no form of the list went unlaunched.  Rows whose QUERY is <pad> in a chain are only
required to be finite (fair-esm computes them and nobody reads them); nothing else is excluded.  PGIBBS_ATTN_FRACTIONS=<file>
appends the largest fraction of the bound per form and flavour (the table in DESIGN.md)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _attention_reference as ar
from protein_gibbs_sampler_amd import _lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREC = {"bf16": _lib.PG_PREC_BF16, "f16": _lib.PG_PREC_F16, "f32": _lib.PG_PREC_FP32}
REL = 6e-5                   # tests/test_gpu_strict_kernels.py's bound of the strict kernels on gaussian inputs
SEEN = set()                 # (kernel, form) of every launch of this process
RAN = set()                  # the chain cases that ran in this process
FRACTIONS = {}               # (kernel, form, flavour) -> largest |err| / bound


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _plan(kind, prec, n, T, R, H, hd, pad, bias, row_step=1):
    buf = ctypes.create_string_buffer(256)
    _lib.check(_lib.lib().pg_dbg_attention_plan(kind, prec, n, T, R, H, hd, int(pad), int(bias), row_step, 0, _n_cu(), buf, 256))
    return buf.value.decode()


def _run_chain(fmt, qkv, H, hd, tok, bk, bv):
    B, T = qkv.shape[:2]
    ctx = np.full((B, T, H * hd), np.nan, np.float32)
    plan = ctypes.create_string_buffer(256)
    _lib.check(_lib.lib().pg_dbg_attention_kv(0, PREC[fmt], _lib.ptr(qkv), _lib.ptr(ctx), B, T, H, hd, None if tok is None else _lib.ptr(tok),
                                              ar.PAD, None if bk is None else _lib.ptr(bk), None if bv is None else _lib.ptr(bv), plan, 256))
    return ctx, plan.value.decode()


def _note(key, frac):
    FRACTIONS[key] = max(FRACTIONS.get(key, 0.0), frac)
    path = os.environ.get("PGIBBS_ATTN_FRACTIONS")
    if path:
        with open(path, "a") as f:
            f.write("%s\t%.4f\n" % (" ".join(map(str, key)), frac))


def _form(pad, bias):
    return {(False, False): "plain", (True, False): "pad", (False, True): "bias", (True, True): "pad+bias"}[(pad, bias)]


def _check_chain(fmt, T, hd, pad, bias, families, n_seq=None, H=None, want_split=False):
    """one shape in one form: every family under the bound, unity exactly 1, the recorded plan the intended one"""
    H = H or (2 if hd == 64 and T <= 576 else 1)          # two heads where the bias key's [bias_k | bias_v] layout can go wrong
    tok = ar.pad_tokens(T) if pad else None
    n_seq = n_seq or (3 if pad else 2)
    strict = fmt == "f32"
    want = _plan(0, PREC[fmt], n_seq, T, 0, H, hd, pad, bias)
    kb = ar.expected_rung(T, bias)
    if not strict:
        assert want.startswith(("whole kb%d" % kb if kb else "long t288") + " hd%d" % hd + (" pad" if pad else "") + (" bias" if bias else "")), want
        # the plan splits the pairs of a partial last round: every plain case of a few pairs and >= 64 tokens is the SPLIT form here;
        # the plain form of those lengths runs with the split switched off (test_plain_form_without_the_split)
        split = " split" in want
        assert split or not want_split, want
        assert not split or (not pad and not bias and T >= 64 and os.environ.get("PGIBBS_ATTN_SPLIT") != "0"), want
        form = "split" if split else _form(pad, bias)
        if hd == 64:
            kernel = "whole" if kb else "long"
        else:
            kernel, form = "hd32", form if kb else {"plain": "long", "pad": "long pad"}[form]
    else:
        kernel, form = "strict hd%d" % hd, _form(pad, bias)
        assert "split-f32" in want and (" pad" in want) == pad and (" bias" in want) == bias, want
    live = np.ones((n_seq, T), bool) if tok is None else tok != ar.PAD
    for family in families:
        if family == "late_tile" and T <= 288:
            continue                                    # the same key as every family's first
        peak = ar.last_real_key(tok) if pad and family == "late_last" else None
        qkv = ar.family_qkv(family, T, n_seq, T, H, hd, peak=peak)
        if pad:
            ar.poison_pad(qkv, tok, H, hd)
        qkv = ar.round_to(fmt, qkv)
        bk, bv = (ar.round_to(fmt, x) for x in ar.family_bias(family, T, H, hd)) if bias else (None, None)
        ctx, ran = _run_chain(fmt, qkv, H, hd, tok, bk, bv)
        assert ran == want, (ran, want)
        assert np.isfinite(ctx).all(), (family, "non-finite context (rows of <pad> queries included)")
        res = ar.chain_attention(qkv, H, hd, tok, bias_k=bk, bias_v=bv)
        err = np.abs(ctx - res.ref)[live]
        if strict and family == "gaussian":
            b = np.full(err.shape, REL * max(1.0, np.abs(res.ref[live]).max()))
        else:
            b = (ar.bound_strict(res) if strict else ar.bound(res, fmt))[live]
        frac = float((err / np.maximum(b, 1e-300)).max())
        print("%s %s %s T=%d %s: %.3f of the bound" % (kernel, form, fmt, T, family, frac))
        assert (err <= b).all(), (family, fmt, T, hd, pad, bias, frac)
        if family == "unity":
            # every exponential is 1, the sum an integer, 1 / l within an ulp: exactly 1 after the 16-bit rounding; the strict
            # kernels return hi + lo of an fp32 product l * (1 / l), within an ulp of 1
            assert (ctx[live] == 1.0).all() if not strict else np.abs(ctx[live] - 1.0).max() <= 2.0 ** -23, (fmt, T, hd, pad, bias)
        _note((kernel, form, fmt), frac)
    SEEN.add((kernel, form))


FAMILIES = ar.FAMILIES
CHAIN_CASES = [(hd, fmt, T) for hd in (64, 32) for fmt in ("bf16", "f16") for T in ar.rung_edge_lengths()]


@pytest.mark.parametrize("hd,fmt,T", CHAIN_CASES)
def test_attention_at_every_rung_edge(hd, fmt, T):
    for pad, bias in ((False, False), (True, False), (False, True), (True, True)):
        if bias and hd != 64:
            continue                                    # the plan refuses it: test_attention_reference_cpu.py
        _check_chain(fmt, T, hd, pad, bias, FAMILIES)
    RAN.add((hd, fmt, T))


@pytest.mark.parametrize("hd,fmt,n_seq,T,H", [(64, "bf16", 26, 258, 20), (64, "f16", 26, 258, 20), (32, "bf16", 33, 130, 32)])
def test_split_form_under_the_bound(hd, fmt, n_seq, T, H):
    """more (sequence, head) pairs than resident workgroups: the last round's pairs run as several workgroups each"""
    _check_chain(fmt, T, hd, False, False, ("negative", "intcode", "unity"), n_seq=n_seq, H=H, want_split=True)
    RAN.add((hd, fmt, n_seq, T, H))


_PLAIN_CHILD = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_gpu_attention_kernels as t
hd, fmt = int(sys.argv[1]), sys.argv[2]
for T in t.ar.rung_edge_lengths():
    if 64 <= T <= 576:
        t._check_chain(fmt, T, hd, False, False, t.FAMILIES)
assert t.SEEN == {("whole" if hd == 64 else "hd32", "plain")}, t.SEEN
print("plain form OK")
"""


@pytest.mark.parametrize("hd,fmt", [(64, "bf16"), (64, "f16"), (32, "bf16"), (32, "f16")])
def test_plain_form_without_the_split(hd, fmt):
    """PGIBBS_ATTN_SPLIT=0 (read once per process, hence the child): the plain form -- what whole rounds of pairs run, the Gibbs path
    -- at the rung edges where a small batch is split"""
    env = dict(os.environ, PGIBBS_ATTN_SPLIT="0")
    p = subprocess.run([sys.executable, "-c", _PLAIN_CHILD % (ROOT, os.path.join(ROOT, "tests")), str(hd), fmt], capture_output=True, text=True,
                       env=env, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "plain form OK" in p.stdout
    SEEN.add(("whole" if hd == 64 else "hd32", "plain"))


STRICT_LENGTHS = [64, 65, 160, 161, 288, 289, 700]


@pytest.mark.parametrize("T", STRICT_LENGTHS)
def test_strict_attention_forms(T):
    for hd, pad, bias in ((64, False, False), (64, True, False), (64, False, True), (64, True, True), (32, False, False), (32, True, False)):
        _check_chain("f32", T, hd, pad, bias, FAMILIES)


# ---- MSA ---------------------------------------------------------------------------------------------------------------------------------
def _run_msa(which, qkv, H, scale, tok):
    B, R, C = qkv.shape[:3]
    ctx = np.full((B, R, C, H * 64), np.nan, np.float32)
    plan = ctypes.create_string_buffer(256)
    _lib.check(_lib.lib().pg_dbg_msa_attention_tok(0, which, _lib.ptr(qkv), _lib.ptr(ctx), B, R, C, H, float(scale),
                                                   None if tok is None else _lib.ptr(tok), ar.PAD, plan, 256))
    return ctx, plan.value.decode()


def _msa_tokens(B, R, C):
    """alignment 0 is narrower (<pad> key columns, row 0 included) and holds scattered <pad>; the last alignment is shallower (<pad>
    rows) and has one column that is all <pad>"""
    tok = np.full((B, R, C), 5, np.int32)
    tok[0, :, C - max(1, C // 7):] = ar.PAD
    tok[0, 1::3, 2] = ar.PAD
    tok[-1, R - max(1, R // 3):] = ar.PAD
    tok[-1, :, min(3, C - 1)] = ar.PAD
    return tok


def _msa_qkv(family, fmt, B, R, C, H, gain, tok, column):
    T = R if column else C
    if column:        # a family is a function of (sequence, key): build it per column and put the columns side by side
        qkv = ar.family_qkv(family, C + R, B * C, R, H, 64).reshape(B, C, R, -1).transpose(0, 2, 1, 3).copy()
    else:
        qkv = ar.family_qkv(family, C + R, B * R, C, H, 64, gain=gain).reshape(B, R, C, -1)
    if tok is not None:
        ar.poison_pad(qkv, tok, H, 64)
    return ar.round_to(fmt, qkv)


def _check_msa(which, fmt, out_fmt, B, R, C, H, padded, families, want_text):
    column = which in (1, 3, 5)
    strict = fmt == "f32" or (padded and not column)            # the ragged tied-row route runs the fp32-scores kernels
    scale = 0.125 / np.sqrt(R)
    tok = _msa_tokens(B, R, C) if padded else None
    for family in families:
        if family == "late_tile":
            continue
        qkv = _msa_qkv(family, "bf16" if (padded and not column and fmt != "f32") else fmt, B, R, C, H, R * scale, tok, column)
        ctx, ran = _run_msa(which, qkv, H, scale, tok)
        assert all(t in ran for t in want_text), (ran, want_text)
        assert np.isfinite(ctx).all(), family
        res = ar.column_attention(qkv, H, tok) if column else ar.tied_row_attention(qkv, H, scale, tok)
        err = np.abs(ctx - res.ref)
        if strict and family == "gaussian" and fmt == "f32":
            b = np.full(err.shape, REL * max(1.0, np.abs(res.ref).max()))
        else:
            b = ar.bound_strict(res, out_fmt) if strict else ar.bound(res, fmt)
        frac = float((err / np.maximum(b, 1e-300)).max())
        kernel = ("column" if column else "tied row") + (" pad" if padded else "")
        print("%s %s %s B=%d R=%d C=%d %s: %.3f of the bound" % (kernel, fmt, ran, B, R, C, family, frac))
        assert (err <= b).all(), (family, which, B, R, C, frac)
        if family == "unity" and column and not strict:
            real_col = np.ones((B, 1, C), bool) if tok is None else (tok != ar.PAD).any(1, keepdims=True)
            assert (ctx[np.broadcast_to(real_col, (B, R, C))] == 1.0).all()       # an all-<pad> column: uniform over e = exp2(rounding), bound only
        _note((kernel, "rc>1" if "reduce" in ran else "", fmt), frac)


@pytest.mark.parametrize("which,fmt", [(1, "bf16"), (5, "f16"), (3, "f32")])
@pytest.mark.parametrize("B,R,C", [(2, 9, 20), (2, 33, 7), (1, 70, 5)])
def test_column_attention_with_padded_rows(which, fmt, B, R, C):
    """<pad> keys get -10000, not -inf: the column that is all <pad> softmaxes to the uniform row, finite"""
    _check_msa(which, fmt, None, B, R, C, 2, True, FAMILIES, ["pad"])
    _check_msa(which, fmt, None, B, R, C, 2, False, ("negative", "intcode"), ["hd64"])


@pytest.mark.parametrize("which,fmt,out_fmt", [(0, "bf16", "bf16"), (2, "f32", None)])
@pytest.mark.parametrize("B,R,C", [(2, 3, 70), (2, 3, 600)])
def test_padded_tied_row_attention_on_the_engines_route(which, fmt, out_fmt, B, R, C):
    """a batch with <pad> takes launch_msa_row_attention_f32, from widened 16-bit q, k, v in the 16-bit modes"""
    _check_msa(which, fmt, out_fmt, B, R, C, 1, True, ("gaussian", "negative", "late_last", "unity", "intcode"), ["row-split-f32"])


@pytest.mark.parametrize("which,fmt", [(0, "bf16"), (4, "f16")])
@pytest.mark.parametrize("B,R,C,mode", [(2, 5, 70, "rc1"), (1, 8, 70, "reduce"), (1, 4, 300, "rc1"), (1, 16, 300, "reduce")])
def test_plain_tied_row_attention_whole_and_split(which, fmt, B, R, C, mode):
    _check_msa(which, fmt, None, B, R, C, 1, False, ("gaussian", "negative", "late_last", "unity", "intcode"), ["row kb", mode])


# ---- coverage ------------------------------------------------------------------------------------------------------------------------------
EXPECTED_FORMS = ({("whole", f) for f in ("plain", "pad", "bias", "pad+bias", "split")} | {("long", f) for f in ("plain", "pad", "bias", "pad+bias")} |
                  {("hd32", f) for f in ("plain", "pad", "split", "long", "long pad")})


def test_every_form_was_launched():
    """the forms the cases above plan, from the plans alone (so that this test stands on its own) -- and, when the whole file ran in
    this process, the forms its launches recorded"""
    planned = set()
    for hd, fmt, T in CHAIN_CASES:
        kb = ar.expected_rung(T, False)
        for pad, bias in ((False, False), (True, False), (False, True), (True, True)):
            if bias and hd != 64:
                continue
            text = _plan(0, PREC[fmt], 3 if pad else 2, T, 0, 2 if hd == 64 and T <= 576 else 1, hd, pad, bias)
            whole = text.startswith("whole")
            assert whole or text.startswith("long"), text
            form = "split" if " split" in text else _form(" pad" in text, " bias" in text)
            planned.add(("whole" if whole else "long", form) if hd == 64 else ("hd32", form if whole else {"plain": "long", "pad": "long pad"}[form]))
    for hd, n_seq, T, H in ((64, 26, 258, 20), (32, 33, 130, 32)):
        assert " split" in _plan(0, PREC["bf16"], n_seq, T, 0, H, hd, False, False)
        planned.add(("whole" if hd == 64 else "hd32", "split"))
    assert planned == EXPECTED_FORMS, planned ^ EXPECTED_FORMS
    chain_seen = {s for s in SEEN if not s[0].startswith("strict")}
    assert chain_seen <= EXPECTED_FORMS
    if len(RAN) == len(CHAIN_CASES) + 3:            # a selection of cases (-k) can only be held to the inclusion above
        assert chain_seen == EXPECTED_FORMS, chain_seen ^ EXPECTED_FORMS
