"""Kernel-level parity of the fused column QKV + attention kernel (csrc/gemm_colattn.hip) on the MI355X: gemm_colattn_kernel<KB, 4>
launched by itself through pg_dbg_colattn, in both operand flavours, at the shapes of tests/_colattn_reference.py (1, 2, 3 and 12
K-steps; a launch below one tile; ragged last tiles and tile groups; every KB), on its three operand families:

  * integer: element by element under the column attention's derived bound (tests/_attention_reference.py), the projection being
    exact by construction, so nothing is granted for it;
  * uniform: under the family's own, much tighter bound;
  * rowcode: exact -- the value says which column, head and feature a stored context element was computed for;
  * every family: the fused launch and the engine's two unfused launches agree bit for bit;
  * the 300 guard rows behind the live context rows keep their sentinel and every live row is overwritten;
  * what the operand's pad rows hold (0, 240, -240) does not change a bit of the context.

No element is excluded from any assertion.  PGIBBS_COLATTN_FRACTIONS=<file> appends the largest fraction of the bound per family and
flavour (the table in DESIGN.md)."""
import ctypes
import os

import numpy as np
import pytest

import _colattn_reference as cr
from protein_gibbs_sampler_amd import _lib

pytestmark = pytest.mark.gpu
PREC = {"bf16": _lib.PG_PREC_BF16, "f16": _lib.PG_PREC_F16}
GUARD = 300                  # context rows behind the live ones
SENTINEL = -1536.0           # representable in bf16 and fp16, 24 times beyond any context of the three families
FRACTIONS = {}               # (family, flavour) -> largest |err| / bound


def _run(fmt, shape, x, w, bias, fused, pad_fill=0.0):
    """pg_dbg_colattn -> (context [B][R][C][d], guard rows [GUARD][d], the recorded plan)"""
    B, R, C, H = shape
    d, M = H * 64, B * R * C
    ctx = np.full((M + GUARD, d), SENTINEL, np.float32)
    plan = ctypes.create_string_buffer(256)
    _lib.check(_lib.lib().pg_dbg_colattn(0, PREC[fmt], _lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(ctx), M + GUARD, B, R, C, H,
                                         int(fused), pad_fill, plan, 256))
    return ctx[:M].reshape(B, R, C, d), ctx[M:], plan.value.decode()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _note(family, fmt, frac):
    FRACTIONS[(family, fmt)] = max(FRACTIONS.get((family, fmt), 0.0), frac)
    path = os.environ.get("PGIBBS_COLATTN_FRACTIONS")
    if path:
        with open(path, "a") as f:
            f.write("%s %s\t%.4f\n" % (family, fmt, frac))


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("shape", cr.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_column_attention_kernel(shape, fmt):
    B, R, C, H = shape
    for family in cr.FAMILIES:
        x, w, bias, g = cr.operands(family, shape)
        qkv = cr.exact_qkv(fmt, x, w, bias, g)
        ref, bound = cr.expected(family, fmt, shape, qkv)
        got, guard, plan = _run(fmt, shape, x, w, bias, True)
        two, guard2, plan2 = _run(fmt, shape, x, w, bias, False)
        print("%s %s %s: fused plan %r, unfused plan %r" % (shape, fmt, family, plan, plan2))
        for name, ctx, rows in (("fused", got, guard), ("unfused", two, guard2)):
            assert (rows == SENTINEL).all(), (family, name, "a store behind the live context rows", np.argwhere(rows != SENTINEL)[:4])
            assert np.isfinite(ctx).all() and (ctx != SENTINEL).all(), (family, name, "a live context row was not written")
        err = np.abs(got - ref)
        frac = float((err / np.maximum(bound, 1e-300)).max()) if family != "rowcode" else float(err.max())
        print("%s %s %s: %s" % (shape, fmt, family, "%.3f of the bound" % frac if family != "rowcode" else "max |err| %g (exact)" % frac))
        if family == "rowcode":
            bad = np.argwhere(got != ref)
            assert not len(bad), (fmt, "first wrong (b, r, c, feature)", bad[:4].tolist(), [float(got[tuple(i)]) for i in bad[:4]],
                                  [float(ref[tuple(i)]) for i in bad[:4]])
        else:
            assert (err <= bound).all(), (family, fmt, frac, np.argwhere(err > bound)[:4].tolist())
            _note(family, fmt, frac)
        # the unfused path is held to the same expectation, so that a disagreement below names the path that is wrong
        assert (np.abs(two - ref) <= bound).all(), (family, fmt, "unfused")
        assert (_bits(got) == _bits(two)).all(), (family, fmt, "fused and unfused differ", np.argwhere(_bits(got) != _bits(two))[:4].tolist())
        # the launches of the unfused branch record their plans; the fused launcher records none
        assert plan == "" and plan2 != "", (plan, plan2)
        if family == "integer":
            for fill in (240.0, -240.0):
                again, rows, _ = _run(fmt, shape, x, w, bias, True, fill)
                assert (_bits(again) == _bits(got)).all(), (fmt, "pad rows of %g change the context" % fill)
                assert (rows == SENTINEL).all()

