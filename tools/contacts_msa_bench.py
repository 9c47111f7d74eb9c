#!/usr/bin/env python3
"""One predict_row_contacts call next to one forward_logits call on the same alignment batch, on one MI355X.

MSA-1b shape (12 x 768, synthetic weights and a seeded contact regression), bf16, two batches: 8 MSAs x depth 32 x 257 columns, and one
128 x 513 alignment.  forward_logits (pg_msa_forward_logits) is the yardstick: the two calls run the same trunk; the contacts call
adds, per block, the tied row-scores kernel and the row softmax (csrc/msa_contact.hip, profiling class "attn_probs") and the APC /
regression fold (csrc/contact.hip, class "contact") and copies B x L x L floats back, forward_logits ends in the LM head over every
row.  The two calls alternate for `--rounds` rounds after one warm-up round; the host clock is read around each call (both end in a
stream synchronisation).  A last, profiled call gives the two classes' own time.  Medians, every round, the ratio, where the added time
goes and the GPU's name are printed as one JSON line and written to `--out`.  Recorded, not asserted.  Needs a GPU: there is no CPU path.
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

SHAPES = [(8, 32, 257), (1, 128, 513)]


def measure(lm, tok, rounds):
    B, R, C = tok.shape
    H, n = lm.cfg["n_heads"], lm.cfg["n_layers"]
    calls = {"forward_logits": lambda: lm.forward_logits(tok), "predict_row_contacts": lambda: lm.predict_row_contacts(tok)}
    for fn in calls.values():
        fn()                                                    # warm-up: buffers, kernels, clocks
    ms = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():                             # same order every round
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    out = {"batch": B, "depth": R, "columns": C, "map_bytes_per_layer": B * H * C * C * 4}
    for k in calls:
        out[k + "_ms"] = round(statistics.median(ms[k]), 3)
        out[k + "_ms_rounds"] = [round(v, 3) for v in ms[k]]
    out["predict_row_contacts_over_forward_logits"] = round(out["predict_row_contacts_ms"] / out["forward_logits_ms"], 4)
    # the two classes alone: one profiled call (the events are recorded around every launch of the call), all blocks together
    lm.prof_enable(True)
    lm.prof_reset()
    calls["predict_row_contacts"]()
    for cls in ("attn_probs", "contact"):
        kernel_ms, launches = lm.prof_get(cls)
        out[cls + "_ms"] = round(kernel_ms, 4)
        out[cls + "_launches"] = launches
        out[cls + "_ms_per_layer"] = round(kernel_ms / n, 4)
    out["attn_probs_kernels"] = lm.prof_get_kernels("attn_probs")
    lm.prof_enable(False)
    out["added_ms"] = round(out["predict_row_contacts_ms"] - out["forward_logits_ms"], 3)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--layers", type=int, default=12, help="fewer layers for a rehearsal")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "fp32"])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "contacts_msa_bench_mi355x.json"))
    args = ap.parse_args(argv)

    import torch
    from protein_gibbs_sampler_amd import models, weights
    if not torch.cuda.is_available():
        raise SystemExit("contacts_msa_bench: no GPU visible -- nothing is measured without one")
    cfg = weights.make_config(weights.MSA1B_CONFIG, n_layers=args.layers)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lm = models.ESM_MSA1(state_dict=weights.synthetic_state_dict(cfg, seed=0), config=cfg, precision=args.precision).model.to("cuda:0")
    lm.set_row_contact_head(*weights.synthetic_contact_head(cfg, seed=0))
    rng = np.random.default_rng(1234)
    out = {"tool": "contacts_msa_bench", "device": torch.cuda.get_device_name(0), "precision": args.precision, "layers": cfg["n_layers"],
           "heads": cfg["n_heads"], "rounds": args.rounds, "shapes": []}
    for B, R, C in SHAPES:
        tok = rng.integers(4, 24, (B, R, C)).astype(np.int32)
        tok[..., 0] = 0
        out["shapes"].append(measure(lm, tok, args.rounds))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
