#!/usr/bin/env python3
"""One masked_marginals call next to one log_likelihood call on the same sequence, on one MI355X.

ESM-1b shape (33 x 1280, synthetic weights), one sequence of `--length` residues (default 256), every position masked in a copy of
its own (`--mask_distance` copies; default: one per position), `--batch_size` copies per forward (default: all of them in one
forward), so both calls run the same batched forwards over the same masked copies and differ only in the last kernel: the gather keeps one log-probability per position, the table kernel 20 and an entropy.
The two calls alternate for `--rounds` rounds after one warm-up round; the host clock is read around each call (both end in a
stream synchronisation).  Medians, every round, the ratio and the GPU's name are printed as one JSON line and written to `--out`.
The expectation -- equal within run-to-run noise -- is recorded, not asserted.  Needs a GPU: there is no CPU path.
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
    ap.add_argument("--length", type=int, default=256)
    ap.add_argument("--mask_distance", type=int, default=None, help="masked copies of the sequence (default: one per position)")
    ap.add_argument("--batch_size", type=int, default=None, help="masked copies per forward (default: all of them)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--layers", type=int, default=33, help="fewer layers for a rehearsal")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "fp32"])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "marginals_bench_mi355x.json"))
    args = ap.parse_args(argv)

    import torch
    from protein_gibbs_sampler_amd import esm_sampler, models, weights
    if not torch.cuda.is_available():
        raise SystemExit("marginals_bench: no GPU visible -- nothing is measured without one")
    cfg = weights.make_config(weights.ESM1B_CONFIG, n_layers=args.layers)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = models.ESM1b(state_dict=weights.synthetic_state_dict(cfg, seed=0), config=cfg, precision=args.precision)
    s = esm_sampler.ESM_sampler(model, device="cuda:0")
    seq = "".join(np.random.default_rng(1234).choice(list(esm_sampler.ESM_ALLOWED_AMINO_ACIDS), args.length))
    kw = dict(mask_distance=float("inf") if args.mask_distance is None else args.mask_distance)
    kw["batch_size"] = int(min(kw["mask_distance"], len(seq))) if args.batch_size is None else args.batch_size
    calls = {"log_likelihood": lambda: s.log_likelihood(seq, **kw), "masked_marginals": lambda: s.masked_marginals(seq, **kw)}
    for fn in calls.values():
        fn()                                                    # warm-up: buffers, kernels, clocks
    ms = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, fn in calls.items():                             # same order every round
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    _, ll = calls["log_likelihood"]()
    logp, _, toks = calls["masked_marginals"]()
    own = np.asarray([logp[i, toks.index(c)] for i, c in enumerate(seq)], dtype=np.float32)
    n = int(min(kw["mask_distance"], len(seq)))
    order = [p for i in range(n) for p in range(i, len(seq), n)]
    out = {"tool": "marginals_bench", "device": torch.cuda.get_device_name(0), "precision": args.precision, "layers": args.layers,
           "d_model": cfg["d_model"], "length": args.length, "masked_copies": n, "copies_per_forward": kw["batch_size"], "rounds": args.rounds,
           "same_bits_at_own_residue": bool(np.array_equal(own[order].view(np.uint32), np.asarray(ll, dtype=np.float32).view(np.uint32)))}
    for k in calls:
        out[k + "_ms"] = round(statistics.median(ms[k]), 3)
        out[k + "_ms_rounds"] = [round(v, 3) for v in ms[k]]
    out["masked_marginals_over_log_likelihood"] = round(out["masked_marginals_ms"] / out["log_likelihood_ms"], 4)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
