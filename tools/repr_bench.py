#!/usr/bin/env python3
"""One forward_representations call (the last layer, residue means only) next to one forward_logits call on the same batch, on one MI355X.

ESM-1b shape (33 x 1280, synthetic weights), `--batch` sequences of `--length` residues (64 x 258 tokens by default), bf16.  forward_logits
is the yardstick: it is the older entry, and the two calls run the same trunk; the representations call ends in the row kernel and the
pool kernel (csrc/repr.hip) and copies batch x d_model floats back, forward_logits in the LM head over every row and a copy of 33 floats
per token.  The two calls alternate for `--rounds` rounds after one warm-up round; the host clock is read around each call (both end in
a stream synchronisation).  A last, profiled call gives the two kernels' own time (the "repr_rows" / "repr_pool" profiling classes) and,
from the bytes they move, their achieved GB/s.  Medians, every round, the ratio and the GPU's name are printed as one JSON line and
written to `--out`.  The expectation -- not slower than forward_logits -- is recorded, not asserted.  Needs a GPU: there is no CPU path.
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--length", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--layers", type=int, default=33, help="fewer layers for a rehearsal")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "fp32"])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "repr_bench_mi355x.json"))
    args = ap.parse_args(argv)

    import torch
    from protein_gibbs_sampler_amd import models, weights
    if not torch.cuda.is_available():
        raise SystemExit("repr_bench: no GPU visible -- nothing is measured without one")
    cfg = weights.make_config(weights.ESM1B_CONFIG, n_layers=args.layers)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lm = models.ESM1b(state_dict=weights.synthetic_state_dict(cfg, seed=0), config=cfg, precision=args.precision).model.to("cuda:0")
    B, T, d, n = args.batch, args.length + 2, cfg["d_model"], cfg["n_layers"]
    rng = np.random.default_rng(1234)
    tok = np.concatenate([np.zeros((B, 1), np.int64), rng.integers(4, 24, (B, args.length)), np.full((B, 1), 2)], axis=1).astype(np.int32)
    pools = np.asarray([[[1, args.length]] * B], np.int32)
    calls = {"forward_logits": lambda: lm.forward_logits(tok),
             "forward_representations": lambda: lm.forward_representations(tok, [n], pools, per_token=False)}
    for fn in calls.values():
        fn()                                                    # warm-up: buffers, kernels, clocks
    ms = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, fn in calls.items():                             # same order every round
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    out = {"tool": "repr_bench", "device": torch.cuda.get_device_name(0), "precision": args.precision, "layers": n, "d_model": d,
           "batch": B, "tokens_per_sequence": T, "rounds": args.rounds}
    for k in calls:
        out[k + "_ms"] = round(statistics.median(ms[k]), 3)
        out[k + "_ms_rounds"] = [round(v, 3) for v in ms[k]]
    out["forward_representations_over_forward_logits"] = round(out["forward_representations_ms"] / out["forward_logits_ms"], 4)
    # the two kernels alone: one profiled call (the events are recorded around every launch of the call)
    lm.prof_enable(True)
    lm.prof_reset()
    calls["forward_representations"]()
    moved = {"repr_rows": 2 * B * T * d * 4,                                   # every row read (LayerNorm) and written once
             "repr_pool": B * args.length * d * 4 + B * d * 4}                 # the residue rows read, one mean per sequence written
    for cls, nbytes in moved.items():
        kernel_ms, launches = lm.prof_get(cls)
        out[cls + "_ms"] = round(kernel_ms, 4)
        out[cls + "_launches"] = launches
        out[cls + "_gb_per_s"] = round(nbytes / (kernel_ms * 1e-3) / 1e9, 1) if kernel_ms > 0 else None
    lm.prof_enable(False)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
