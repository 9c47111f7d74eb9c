#!/usr/bin/env python3
"""One predict_contacts call next to one forward_logits call on the same batch, on one MI355X.

ESM-1b shape (33 x 1280, synthetic weights and a seeded contact regression), `--batch` sequences of `--length` residues (64 x 258 tokens
by default), bf16.  forward_logits is the yardstick: the two calls run the same trunk; the contacts call adds, per layer, the
attention-probability kernel and the APC / regression fold (csrc/contact.hip) and copies batch x L x L floats back, forward_logits ends
in the LM head over every row.  The two calls alternate for `--rounds` rounds after one warm-up round; the host clock is read around
each call (both end in a stream synchronisation).  A last, profiled call gives the two new profiling classes' own time ("attn_probs",
"contact") and, from the bytes they move, their achieved GB/s.  Medians, every round, the ratio and the GPU's name are printed as one
JSON line and written to `--out`.  Recorded, not asserted.  Needs a GPU: there is no CPU path.
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
                                                  "contacts_bench_mi355x.json"))
    args = ap.parse_args(argv)

    import torch
    from protein_gibbs_sampler_amd import models, weights
    if not torch.cuda.is_available():
        raise SystemExit("contacts_bench: no GPU visible -- nothing is measured without one")
    cfg = weights.make_config(weights.ESM1B_CONFIG, n_layers=args.layers)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lm = models.ESM1b(state_dict=weights.synthetic_state_dict(cfg, seed=0), config=cfg, precision=args.precision).model.to("cuda:0")
    lm.set_contact_head(*weights.synthetic_contact_head(cfg, seed=0))
    B, T, H, n = args.batch, args.length + 2, cfg["n_heads"], cfg["n_layers"]
    W = T - 2
    rng = np.random.default_rng(1234)
    tok = np.concatenate([np.zeros((B, 1), np.int64), rng.integers(4, 24, (B, args.length)), np.full((B, 1), 2)], axis=1).astype(np.int32)
    calls = {"forward_logits": lambda: lm.forward_logits(tok), "predict_contacts": lambda: lm.predict_contacts(tok)}
    for fn in calls.values():
        fn()                                                    # warm-up: buffers, kernels, clocks
    ms = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, fn in calls.items():                             # same order every round
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    out = {"tool": "contacts_bench", "device": torch.cuda.get_device_name(0), "precision": args.precision, "layers": n, "heads": H,
           "batch": B, "tokens_per_sequence": T, "rounds": args.rounds, "map_bytes_per_layer": B * H * T * T * 4}
    for k in calls:
        out[k + "_ms"] = round(statistics.median(ms[k]), 3)
        out[k + "_ms_rounds"] = [round(v, 3) for v in ms[k]]
    out["predict_contacts_over_forward_logits"] = round(out["predict_contacts_ms"] / out["forward_logits_ms"], 4)
    # the two classes alone: one profiled call (the events are recorded around every launch of the call), all layers together
    lm.prof_enable(True)
    lm.prof_reset()
    calls["predict_contacts"]()
    item = 4 if args.precision == "fp32" else 2
    moved = {"attn_probs": n * (B * T * 2 * cfg["d_model"] * item + B * H * T * T * 4),      # q and k read, the maps written
             # the window of every map read twice by each of the two kernels (A and its transpose), the logits read and written
             "contact": n * (4 * B * H * W * W * 4 + 2 * B * W * W * 4)}
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
