"""The GEMM dispatch table, without a GPU: `pg_dbg_gemm_plan` prints what `plan_gemm` (csrc/gemm_bf16.hip) picks for a shape in the
text a launch records for `pg_prof_get_kernels`.  The expected strings are what the launches of the build BEFORE the dispatch became
one function recorded on an MI355X (256 CUs) -- a change of this table changes which kernel runs for a measured shape, and says so here.

Every table runs in a child process with the PGIBBS_GEMM* switches removed (they are read once per process)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CU = 256
BF16, BF16_GELU, RESID, F32 = 0, 1, 2, 3      # the EPI_* values of csrc/kernels.h

CHILD = """
import ctypes, json, sys
sys.path.insert(0, %r)
from protein_gibbs_sampler_amd import _lib
L = _lib.lib()
out = []
for (M, N, K, epi, variant, have_ws, m_live) in json.loads(sys.argv[1]):
    buf = ctypes.create_string_buffer(256)
    _lib.check(L.pg_dbg_gemm_plan(M, N, K, epi, variant, have_ws, m_live, %d, buf, len(buf)))
    out.append(buf.value.decode())
print(json.dumps(out))
""" % (ROOT, N_CU)


def plans(cases, **switches):
    env = {k: v for k, v in os.environ.items() if not k.startswith("PGIBBS_GEMM")}
    env.update(switches)
    r = subprocess.run([sys.executable, "-c", CHILD, json.dumps(cases)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def check(table, **switches):
    got = plans([list(c) for c, _ in table], **switches)
    wrong = [(c, g, w) for (c, w), g in zip(table, got) if g != w]
    assert not wrong, "\n".join("%r: plan %r, expected %r" % t for t in wrong)


# the four projections of a layer with the engine's epilogues: (N, K, epilogue, split-K scratch on offer)
def layer(d, f):
    return [(3 * d, d, BF16, 0), (d, d, RESID, 1), (f, d, BF16_GELU, 0), (d, f, RESID, 1)]


def rows(M, shapes, texts, variant=2, m_live=0):
    return [((M, n, k, e, variant, ws, m_live), t) for (n, k, e, ws), t in zip(shapes, texts)]


ESM, MSA = layer(1280, 5120), layer(768, 3072)
PRODUCTION = (
    # config 2: 256 chains x 258 tokens
    rows(66048, ESM, ["w16-256x256 3840t + tail64 480t", "pp256x256 1280t + tail64 160t", "w16-256x256 5120t + tail64 640t",
                      "pp256x256 1280t + tail64 160t"])
    # 64- and 32-chain shards: 325 / 165 tiles of 256 rows in the residual GEMMs become 430 / 220 of 192
    + rows(16640, ESM, ["w16-256x256 975t", "pp192x256 430t + tail64 40t", "w16-256x256 1280t + tail64 320t", "pp192x256 430t + tail64 40t"])
    + rows(8448, ESM, ["w16-256x256 495t", "pp192x256 220t", "w16-256x256 660t", "pp192x256 220t"])
    + rows(8448, ESM[1:2], ["pp192x256 220t"], m_live=8256)
    + rows(16640, ESM[3:], ["pp192x256 430t + tail64 40t"], m_live=16512)
    # the measured case where 250 tiles of 192 rows + 40 tail tiles lose against 190 tiles of 256 rows
    + rows(9728, [ESM[1], ESM[3]], ["pp256x256 190t", "pp256x256 190t"])
    # small jobs
    + rows(1024, ESM, ["tile128x128 240t", "tile64x64 320t", "tile128x128 320t", "tile128x128 80t x4k"])
    + rows(64, ESM, ["tile64x64 60t", "tile64x64 20t", "tile64x64 80t", "tile64x64 20t x4k"])
    # config 1: one chain of 27 tokens; fc2 as four K-splits when it is offered scratch, in one piece when not
    + rows(32, ESM, ["skinny8w 240t", "skinny8w 80t", "skinny8w 320t", "skinny8w 80t x4k"])
    + [((32, 1280, 5120, RESID, 2, 0, 0), "skinny8w 80t"), ((1024, 1280, 5120, RESID, 2, 0, 0), "tile64x64 320t")]
    # ESM-2 3B's fc2: K = 10240 as eight splits
    + [((M, 2560, 10240, RESID, 2, 1, 0), t) for M, t in ((32, "skinny8w 160t x8k"), (64, "tile64x64 40t x8k"), (1024, "tile64x64 640t"),
                                                         (66048, "pp256x256 2560t + tail64 320t"))]
    # ESM-MSA-1b: 768 wide
    + rows(66048, MSA, ["w16-256x256 2304t + tail64 288t", "pp256x256 768t + tail64 96t", "w16-256x256 3072t + tail64 384t",
                        "pp256x256 768t + tail64 96t"])
    + rows(16640, MSA, ["w16-256x256 585t", "pp256x256 195t", "w16-256x256 768t + tail64 192t", "pp256x256 195t"])
    + rows(32, MSA, ["skinny8w 144t", "skinny8w 48t", "skinny8w 192t", "skinny8w 48t x3k"])
    # shapes the dispatch refuses
    + [((100, 1280, 1280, BF16, 2, 0, 0), "error: gemm: M must be a multiple of 16 and N of 64"),
       ((1000, 1280, 1280, BF16, 2, 0, 0), "error: gemm: M must be a multiple of 128 and N of 64"),
       ((1024, 1280, 1312, BF16, 2, 0, 0), "error: gemm: K must be a multiple of 64")]
)

# the micro-benchmark variants (table in csrc/kernels_ops.inc); a variant outside the table is an error at every shape
VARIANTS = [
    ((66048, 3840, 1280, BF16, 1, 0, 0), "tile256x256-lockstep 3870t"),
    ((1024, 1280, 1280, RESID, 1, 1, 0), "tile256x256-lockstep 20t"),
    ((32, 1280, 5120, RESID, 1, 1, 0), "tile64x64 20t"),
    ((1024, 1280, 1280, RESID, 6, 1, 0), "tile64x64 320t"),
    ((1024, 1280, 1280, RESID, 7, 1, 0), "tile128x128 80t"),
    ((8448, 1280, 5120, RESID, 8, 1, 0), "pp192x256 220t"),
    ((16640, 1280, 1280, RESID, 8, 0, 0), "pp192x256 430t + tail64 40t"),
    ((66048, 3840, 1280, BF16, 20, 0, 0), "pp256x256 3870t"),
    ((66048, 3840, 1280, BF16, 21, 0, 0), "error: gemm: unknown variant"),
    ((66048, 3840, 1280, BF16, 80, 0, 0), "w16-256x256 3870t"),
    ((66048, 1280, 1280, RESID, 80, 0, 0), "w16-256x256 1290t"),
    ((64, 3840, 1280, BF16, 21, 0, 0), "error: gemm: unknown variant"),
]


def test_production_dispatch():
    check(PRODUCTION)


def test_benchmark_variants():
    check(VARIANTS)


def test_without_192_row_tiles():
    check(rows(16640, ESM, ["w16-256x256 975t", "pp256x256 325t", "w16-256x256 1280t + tail64 320t", "pp256x256 325t"])
          + rows(8448, ESM, ["w16-256x256 495t", "pp256x256 165t", "w16-256x256 660t", "pp256x256 165t"])
          + rows(66048, ESM[1:2], ["pp256x256 1280t + tail64 160t"]), PGIBBS_GEMM_T192="0")


def test_without_tail_tiles():
    check(rows(66048, ESM, ["w16-256x256 3870t", "pp192x256 1720t", "w16-256x256 5160t", "pp192x256 1720t"])
          + rows(16640, ESM, ["w16-256x256 975t", "pp192x256 430t + tail64 40t", "w16-256x256 1300t", "pp192x256 430t + tail64 40t"])
          + rows(66048, MSA, ["w16-256x256 2322t", "pp256x256 774t", "w16-256x256 3096t", "pp256x256 774t"]), PGIBBS_GEMM_TAIL="0")


def test_bad_arguments_are_refused():
    from protein_gibbs_sampler_amd import _lib
    import ctypes
    buf = ctypes.create_string_buffer(64)
    assert _lib.lib().pg_dbg_gemm_plan(32, 1280, 1280, BF16, 2, 0, 0, 0, buf, len(buf)) == _lib.PG_ERR_INVALID
    assert _lib.lib().pg_dbg_gemm_plan(32, 1280, 1280, BF16, 2, 0, 0, N_CU, None, 0) == _lib.PG_ERR_INVALID
