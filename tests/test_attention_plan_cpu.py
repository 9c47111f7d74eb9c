"""The attention dispatch, without a GPU: `pg_dbg_attention_plan` prints what plan_attention (csrc/attention.hip), plan_attention_f32 /
plan_msa_row_f32 (csrc/attention_f32.hip) and plan_msa_row (csrc/msa_attention.hip) pick for a shape, in the text a launch records for
`pg_prof_get_kernels(..., "attention")`.  The expected strings are the decisions of the build BEFORE the dispatch became plan
functions, worked out from that launch code for an MI355X (256 CUs) and compared with what its launches put on the device:
tools/attention_plan_sweep.py launches these tables under `rocprofv3 --kernel-trace` and checks each kernel template,
grid and workgroup size in the trace against the text here (`--check`).  The cases it cannot launch through a debug entry point -- a
refusal, a <pad> mask on strided sequences, a job-level `order_bh` -- follow from the same code by hand.  A change of these tables
changes which kernel runs for a measured shape, and says so here.

Every table runs in a child process with the PGIBBS_ATTN* switches removed (they are read once per process)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CU = 256
BF16, FP32, F16 = 0, 1, 2        # PG_PREC_* of include/pgibbs.h

CHILD = """
import ctypes, json, sys
sys.path.insert(0, %r)
from protein_gibbs_sampler_amd import _lib
L = _lib.lib()
out = []
for args in json.loads(sys.argv[1]):
    buf = ctypes.create_string_buffer(256)
    _lib.check(L.pg_dbg_attention_plan(*args, int(sys.argv[2]), buf, len(buf)))
    out.append(buf.value.decode())
print(json.dumps(out))
""" % ROOT


def att(n_seq, T, H=20, hd=64, pad=0, bias=0, row_step=1, precision=BF16):
    """full attention over n_seq sequences of T tokens: the arguments of pg_dbg_attention_plan up to n_cu"""
    return (0, precision, n_seq, T, 0, H, hd, pad, bias, row_step, 0)


def row(B, R, C, H=12, order_bh=0, precision=BF16, pad=0):
    """tied row attention of B alignments of R rows x C columns"""
    return (1, precision, B, C, R, H, 64, pad, 0, 1, order_bh)


def strict(n_seq, T, **kw):
    return att(n_seq, T, precision=FP32, **kw)


def plans(cases, n_cu=N_CU, **switches):
    env = {k: v for k, v in os.environ.items() if not k.startswith("PGIBBS_ATTN")}
    env.update(switches)
    r = subprocess.run([sys.executable, "-c", CHILD, json.dumps(cases), str(n_cu)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def check(table, **switches):
    got = plans([list(c) for c, _ in table], **switches)
    wrong = [(c, g, w) for (c, w), g in zip(table, got) if g != w]
    assert not wrong, "\n".join("%r: plan %r, expected %r" % t for t in wrong)


# ---- 16-bit operands: chains and strided sequences (ESM-1b / ESM-2 650M: 20 heads of 64; slots = 512 up to 20 key blocks, 256 beyond)
CHAINS = [
    (att(256, 258), "whole kb18 hd64 5120wg"),                         # config 2
    (att(64, 258), "whole kb18 hd64 split2 1024+512wg"),               # 64-chain shard: 1280 pairs = two rounds + half a round
    (att(32, 258), "whole kb18 hd64 split4 512+512wg"),                # 32-chain shard: one round + a quarter
    (att(33, 258), "whole kb18 hd64 split3 512+444wg"),                # 660 pairs: 512 whole + 148 x 3
    (att(1, 27), "whole kb2 hd64 20wg"),                               # config 1
    (att(8, 64), "whole kb4 hd64 160wg"),                              # four query blocks: nothing to split
    (att(8, 65), "whole kb6 hd64 160wg"),
    (att(8, 200), "whole kb14 hd64 split3 0+480wg"),                   # less than one round: every pair split
    (att(8, 576), "whole kb36 hd64 160wg"),                            # one workgroup per CU: 160 of 256 slots, no split
    (att(8, 577), "long t288 hd64 1600wg"),
    (att(2, 1024), "long t288 hd64 640wg"),
    (att(513, 128, H=12, row_step=513), "whole kb8 hd64 6156wg"),      # MSA column attention of config 5: strided, never split
    # <pad> mask and ESM-1's bias key on both sides of a coarse rung (the bias forms: ESM-1 6 x 768, 12 heads)
    (att(2, 288, pad=1), "whole kb18 hd64 pad 40wg"),
    (att(2, 289, pad=1), "whole kb20 hd64 pad 40wg"),
    (att(3, 287, H=12, bias=1), "whole kb18 hd64 bias 36wg"),          # 288 keys
    (att(3, 288, H=12, bias=1), "whole kb24 hd64 bias 36wg"),          # 289 keys: no 20-block rung with the bias key
    (att(3, 200, H=12, bias=1), "whole kb18 hd64 bias 36wg"),
    (att(3, 100, H=12, pad=1, bias=1), "whole kb8 hd64 pad bias 36wg"),
    (att(1, 600, H=12, bias=1), "long t288 hd64 bias 120wg"),
    (att(1, 600, H=12, pad=1, bias=1), "long t288 hd64 pad bias 120wg"),
    (att(2, 600, pad=1), "long t288 hd64 pad 400wg"),
]
# ESM-2 150M: 20 heads of 32; resident workgroups per CU 4 up to 20 key blocks, 3 up to 26, 2 beyond
HEAD32 = [
    (att(256, 258, hd=32), "whole kb18 hd32 5120wg"),
    (att(32, 258, hd=32), "whole kb18 hd32 640wg"),                    # 640 of 1024 slots
    (att(64, 258, hd=32), "whole kb18 hd32 split4 1024+1024wg"),
    (att(48, 400, hd=32), "whole kb26 hd32 split4 768+768wg"),
    (att(32, 500, hd=32), "whole kb32 hd32 split4 512+512wg"),
    (att(2, 100, hd=32, pad=1), "whole kb8 hd32 pad 40wg"),
    (att(3, 600, hd=32), "long t288 hd32 600wg"),
    (att(3, 600, hd=32, pad=1), "long t288 hd32 pad 600wg"),
]
# ---- strict fp32: (key blocks per tile, query blocks per wave) out of (4,1) (10,1) (10,2) (10,3) (6,5) (8,5) (10,5)
STRICT = [
    (strict(2, 27), "split-f32 kb4 nqb1 hd64 40wg"),
    (strict(2, 64), "split-f32 kb4 nqb1 hd64 40wg"),
    (strict(3, 64, H=12, bias=1), "split-f32 kb10 nqb1 hd64 bias 36wg"),       # 65 keys
    (strict(2, 65), "split-f32 kb10 nqb2 hd64 40wg"),
    (strict(2, 129), "split-f32 kb10 nqb3 hd64 40wg"),
    (strict(2, 193), "split-f32 kb8 nqb5 hd64 40wg"),                  # 256 padded keys against 288 and 320
    (strict(256, 258), "split-f32 kb6 nqb5 hd64 5120wg"),              # config 2: 288 padded keys beat 320
    (strict(3, 258, H=12, bias=1), "split-f32 kb6 nqb5 hd64 bias 36wg"),       # 259 keys
    (strict(2, 330), "split-f32 kb8 nqb5 hd64 80wg"),                  # two query chunks per pair
    (strict(2, 258, hd=32), "split-f32 kb6 nqb5 hd32 40wg"),
    (strict(2, 100, hd=32, pad=1), "split-f32 kb10 nqb2 hd32 pad 40wg"),
    (strict(513, 128, H=12, row_step=513), "split-f32 kb10 nqb2 hd64 6156wg"),        # MSA column attention of config 5
    (strict(513, 128, H=12, row_step=513, pad=1), "split-f32 kb10 nqb2 hd64 pad 6156wg"),
]
# ---- MSA tied row attention (ESM-MSA-1b: 12 heads), both precisions
ROWS = [
    (row(64, 32, 257), "row kb18 w9 rc1 1536wg"),                                       # BASELINE config 4
    (row(1, 128, 513), "row kb34 w8 rc8 480wg, reduce 480x1w, 480wg"),                  # config 5: split-R
    (row(1, 32, 301), "row kb24 w8 rc8 288wg, reduce 288x1w, 288wg"),                   # one template: the 20 -> 24 exception
    (row(4, 32, 301), "row kb24 w8 rc3 432wg, reduce 1152x1w, 432wg"),                  # four as one job: still below two rounds
    (row(4, 32, 301, order_bh=12), "row kb20 w8 rc8 1152wg, reduce 1152x1w, 1152wg"),   # four templates, split as one: 20 blocks
    (row(64, 32, 140), "row kb10 w9 rc1 768wg"),
    (row(2, 8, 64), "row kb4 w4 rc2 48wg, reduce 96x1w, 48wg"),
    (row(64, 32, 257, precision=F16), "row kb18 w9 rc1 1536wg"),
    (row(64, 32, 257, precision=FP32), "row-split-f32 kb10 kt2 7680wg, 122880wg"),
    (row(1, 128, 513, precision=FP32), "row-split-f32 kb10 kt4 432wg, 13824wg"),
    (row(2, 8, 64, precision=FP32), "row-split-f32 kb4 kt1 24wg, 192wg"),
    (row(2, 8, 64, precision=FP32, pad=1), "row-split-f32 kb4 kt1 24wg, 192wg"),
]
REFUSED = [
    (att(2, 100, hd=48), "error: attention: head dimension 48: the kernels are built for 64 (every architecture) or 32, 128, 16 (ESM-2 only)"),
    (att(2, 100, hd=32, bias=1), "error: attention: the bias_k / bias_v key (ESM-1) is built for heads of 64 only"),
    (att(2, 0), "error: attention: empty sequence"),
    (att(200000000, 27), "error: attention: too many sequences"),
    (att(100000000, 600), "error: attention: too many sequences"),      # the long kernel's grid: pairs x ten query chunks
    (strict(2, 100, hd=48), "error: attention: head dimension 48: the kernels are built for 64 (every architecture) or 32, 128, 16 (ESM-2 only)"),
    (strict(2, 100, hd=32, bias=1), "error: attention: the bias_k / bias_v key (ESM-1) is built for heads of 64 only"),
    (strict(2, 0), "error: attention: empty sequence"),
    (strict(200000000, 27), "error: attention: too many sequences"),
    (row(1, 32, 0), "error: row attention: empty alignment"),
    (row(1, 32, 577), "error: row attention: alignments wider than 576 token columns (<cls> + 575 residues) take the fp32-scores path"),
]


def test_chains_and_strided_sequences():
    check(CHAINS)


def test_heads_of_32():
    check(HEAD32)


def test_strict_attention():
    check(STRICT)


def test_msa_row_attention():
    check(ROWS)


def test_refusals():
    check(REFUSED)


# the switches: name -> (environment, table)
SWITCHED = {
    "no split of the last round": ({"PGIBBS_ATTN_SPLIT": "0"}, [
        (att(32, 258), "whole kb18 hd64 640wg"), (att(33, 258), "whole kb18 hd64 660wg"), (att(64, 258, hd=32), "whole kb18 hd32 1280wg")]),
}


@pytest.mark.parametrize("name", sorted(SWITCHED))
def test_switches(name):
    env, table = SWITCHED[name]
    check(table, **env)


def test_removed_switches_are_inert():
    """the names of the switches that left the library (the all-VALU strict kernels, forced strict tile pairs, the coarse ladder, the
    tiled kernel at head 128) select nothing any more: every default text, and a head-128 chain at T = 258 on the whole-sequence kernel"""
    removed = dict(PGIBBS_ATTN_F32="valu", PGIBBS_ATTN_F32_NQB="1", PGIBBS_ATTN_F32_KB="10", PGIBBS_ATTN_LADDER="0", PGIBBS_ATTN_HD128_WHOLE="0")
    table, hd128 = CHAINS + STRICT + ROWS, list(att(256, 258, H=40, hd=128))
    got = plans([list(c) for c, _ in table] + [hd128], **removed)
    assert got[:-1] == [w for _, w in table]
    assert got[-1:] == plans([hd128]) and got[-1].startswith("whole kb18 hd128 ")


def test_other_cu_counts():
    """the split of the last round counts the device's own CUs: 640 pairs are one round + a quarter of 512 slots, but fit 304 x 2"""
    assert plans([list(att(32, 258))], n_cu=304) == ["whole kb18 hd64 split4 608+128wg"]


def test_bad_arguments_are_refused():
    from protein_gibbs_sampler_amd import _lib
    import ctypes
    buf = ctypes.create_string_buffer(64)
    f = _lib.lib().pg_dbg_attention_plan
    ok = list(att(32, 258))
    assert f(*ok, N_CU, buf, len(buf)) == _lib.PG_OK
    assert f(*ok, 0, buf, len(buf)) == _lib.PG_ERR_INVALID                   # n_cu
    assert f(*ok, N_CU, None, 0) == _lib.PG_ERR_INVALID
    assert f(*att(0, 258), N_CU, buf, len(buf)) == _lib.PG_ERR_INVALID       # no sequences
    assert f(*att(32, 258, H=0), N_CU, buf, len(buf)) == _lib.PG_ERR_INVALID
    assert f(*att(32, 258, precision=7), N_CU, buf, len(buf)) == _lib.PG_ERR_INVALID
    assert f(2, *ok[1:], N_CU, buf, len(buf)) == _lib.PG_ERR_INVALID         # kind
    assert f(*row(1, 0, 301), N_CU, buf, len(buf)) == _lib.PG_ERR_INVALID    # no alignment rows
