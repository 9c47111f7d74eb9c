"""Where the expected strings of tests/test_attention_plan_cpu.py come from: the test's shapes, launched on the device.

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/attention_plan_sweep.py [--group G]     launch the group's shapes
    python tools/attention_plan_sweep.py --check OUT [--group G]      the trace against the test's expected strings
    python tools/attention_plan_sweep.py --compare OUT_A OUT_B        two builds: the same (kernel, grid, workgroup) sequence

A shape goes through pg_dbg_attention_hd (chains), pg_dbg_msa_attention (tied row attention, column attention = strided sequences) or,
with ESM-1's bias key, one forward of a synthetic one-layer ESM-1 model (12 heads).  What no entry point launches is skipped and
listed: refusals, a <pad> mask on strided sequences or in the strict row attention, a job-level order_bh.  The launching mode uses
nothing that an older build lacks, so it runs unchanged on the build before the plan functions.  A group other than `default` needs
its switch in the environment of the whole process (the switches are read once): the tool checks that it is set."""
import argparse
import csv
import glob
import os
import re
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_attention_plan_cpu as T  # noqa: E402

BF16, FP32, F16 = T.BF16, T.FP32, T.F16


GROUPS = dict({"default": ({}, T.CHAINS + T.HEAD32 + T.STRICT + T.ROWS)}, **T.SWITCHED)


def launchable(case):
    kind, prec, n, t_or_c, R, H, hd, pad, bias, row_step, order_bh = case
    if kind == 1:
        return not pad and not order_bh
    if row_step != 1:
        return not pad and not bias and hd == 64
    return n * H < 1 << 24 and (not bias or H == 12)


def _esm1(precision):
    from protein_gibbs_sampler_amd import models, weights
    cfg = weights.make_config(weights.ESM1_T6_CONFIG, n_layers=1, d_model=768, d_ffn=3072)
    sd = weights.synthetic_state_dict(cfg, seed=7, std=0.03, embed_std=0.05, ln_jitter=0.1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return models.ESM6(state_dict=sd, config=cfg, precision={BF16: "bf16", FP32: "fp32", F16: "fp16"}[precision]).model.to("cuda:0")


def launch(case, models):
    from protein_gibbs_sampler_amd import _lib
    L = _lib.lib()
    kind, prec, n, t_or_c, R, H, hd, pad, bias, row_step, order_bh = case
    if kind == 1 or row_step != 1:
        B, C, rows = (n, t_or_c, R) if kind == 1 else (1, n, t_or_c)
        which = (0 if kind == 1 else 1) + {BF16: 0, FP32: 2, F16: 4}[prec]
        qkv = np.zeros((B * rows * C, 3 * H * 64), dtype=np.float32)
        ctx = np.empty((B * rows * C, H * 64), dtype=np.float32)
        _lib.check(L.pg_dbg_msa_attention(0, which, _lib.ptr(qkv), _lib.ptr(ctx), B, rows, C, H, 0.125))
    elif bias:
        if prec not in models:
            models[prec] = _esm1(prec)
        tok = np.full((n, t_or_c), 5, dtype=np.int64)
        tok[:, 0] = 32
        if pad:
            tok[-1, -3:] = 1
        models[prec].forward_logits(tok)
    else:
        qkv = np.zeros((n * t_or_c, 3 * H * hd), dtype=np.float32)
        ctx = np.empty((n * t_or_c, H * hd), dtype=np.float32)
        tok = None
        if pad:
            tok = np.full((n, t_or_c), 5, dtype=np.int32)
            tok[-1, -3:] = 1
        _lib.check(L.pg_dbg_attention_hd(0, prec, _lib.ptr(qkv), _lib.ptr(ctx), n, t_or_c, H, hd, _lib.ptr(tok) if pad else None, 1))


def expected_launches(text, prec):
    """plan text -> [(kernel name as the trace demangles it, without blanks; workgroups; threads per workgroup)]"""
    ns = "pg::opf16::" if prec == F16 else "pg::opbf16::"
    b = lambda x: "true" if x else "false"      # noqa: E731
    w = text.replace(",", "").split()
    pad, bias = "pad" in w, "bias" in w
    wg = [int(x[:-2]) for x in w if re.fullmatch(r"\d+wg", x)]
    num = lambda p: next(int(x[len(p):]) for x in w if re.fullmatch(p + r"\d+", x))      # noqa: E731
    if w[0] == "whole":
        split = [x for x in w if re.fullmatch(r"\d+\+\d+wg", x)]
        grid = sum(int(v) for v in split[0][:-2].split("+")) if split else wg[0]
        return [(ns + "attention_kernel<%d,%s,%s,%s,%d>" % (num("kb"), b(pad), b(bias), b(split), num("hd")), grid, 256)]
    if w[0] == "long":
        return [(ns + "attention_long_kernel<18,2,%s,%s,%d>" % (b(pad), b(bias), num("hd")), wg[0], 256)]
    if w[0] == "split-f32":
        return [("pg::opbf16::attention_split_kernel<%d,%d,%s,%s,%d>" % (num("kb"), num("nqb"), b(bias), b(pad), num("hd")), wg[0], 256)]
    if w[0] == "row":
        k, nw = num("kb"), num("w")
        name = ns + "msa_row_attention_kernel<%d,%d,%%d>" % (k, nw)
        if num("rc") == 1:
            return [(name % 0, wg[0], nw * 64)]
        red = next(int(x[:-3]) for x in w if re.fullmatch(r"\d+x1w", x))
        return [(name % 1, wg[0], nw * 64), (name % 3, red, 64), (name % 2, wg[1], nw * 64)]
    if w[0] == "row-split-f32":
        return [("pg::opbf16::msa_row_scores_split_kernel<%d>" % num("kb"), wg[0], 256), ("pg::opbf16::msa_row_apply_split_kernel<%d>" % num("kb"), wg[1], 256)]
    raise ValueError(text)


def read_trace(out_dir):
    """the attention launches of a rocprofv3 kernel trace, in launch order: (kernel name without arguments and blanks, workgroups, threads)"""
    rows = []
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r["Kernel_Name"]
                if not re.search(r"attention_(long_|split_)?kernel|msa_row_\w+_kernel", name):
                    continue
                wgs = int(r.get("Workgroup_Size_X") or r["Workgroup_Size"])
                grid = int(r.get("Grid_Size_X") or r["Grid_Size"])
                name = re.sub(r"^void\s+", "", name).split("(")[0].replace(" ", "")
                rows.append((int(r["Start_Timestamp"]), name, grid // wgs, wgs))
    return [r[1:] for r in sorted(rows)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--group", default="default", choices=sorted(GROUPS), help="default: no switch; else a key of the test's SWITCHED")
    ap.add_argument("--check", metavar="OUT")
    ap.add_argument("--compare", nargs=2, metavar="OUT")
    a = ap.parse_args()
    if a.compare:
        x, y = read_trace(a.compare[0]), read_trace(a.compare[1])
        diff = [(i, p, q) for i, (p, q) in enumerate(zip(x, y)) if p != q]
        print("%d and %d attention launches, %d differ" % (len(x), len(y), len(diff)))
        for d in diff[:20]:
            print("  launch %d: %r != %r" % d)
        return 0 if x and len(x) == len(y) and not diff else 1
    switches, table = GROUPS[a.group]
    for k, v in switches.items():
        assert os.environ.get(k) == v, "group %s needs %s=%s in the environment" % (a.group, k, v)
    run = [(c, t) for c, t in table if launchable(c) and not t.startswith("error")]
    if a.check:
        want = [(c, e) for c, t in run for e in expected_launches(t, c[1])]
        got = read_trace(a.check)
        bad = 0
        for i, (c, e) in enumerate(want):
            g = got[i] if i < len(got) else None
            if g != e:
                bad += 1
                print("case %r: the test expects %r, the trace has %r" % (c, e, g))
        print("group %s: %d launches expected from %d cases, %d in the trace, %d disagree" % (a.group, len(want), len(run), len(got), bad))
        return 0 if not bad and len(got) == len(want) else 1
    models = {}
    for c, t in table:
        if (c, t) not in run:
            print("skipped (no entry point launches it): %r" % (c,))
            continue
        launch(c, models)
        print("launched %r" % (c,), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
