#!/usr/bin/env python3
"""Per-position symbol probabilities of the last sequence of an MSA under the ESM-MSA model, with the surface of the reference's
`pgen_msa_seq_probs.py` (src/pgen/pgen_msa_seq_probs.py:20-45 table, :49-62 flags).  That file no longer runs in
the reference (it calls ESM_MSA_sampler.probs_single, which the class lost, and DataFrame.append, which pandas removed), so the
table below follows its code and help text, not a recording.

Output: a tab separated table -- a header of the target row's residues; one row per symbol of `toks` with its probability at every
position (%.8g); then the rows `position` (1-based), `consensus` (the most probable symbol per column) and `different` (1 where the
consensus is not the target row's residue)."""
import argparse
import csv
import sys
import textwrap

import numpy as np

from . import models
from ._cli import RawAndDefaultsFormatter, add_engine_args, seed_everything
from .esm_msa_sampler import ESM_MSA_sampler
from .fasta_io import parse_fasta

model_map = {"esm_msa1": models.ESM_MSA1}
SUMMARY_ROWS = ("position", "consensus", "different")


def table_rows(probs, toks, target):
    """The table as lists of strings: header, len(toks) probability rows, then position / consensus / different."""
    probs = np.asarray(probs)
    if probs.shape != (len(toks), len(target)):
        raise ValueError("expected a [%d, %d] table, got %r" % (len(toks), len(target), probs.shape))
    consensus = [toks[i] for i in np.argmax(probs, axis=0)]
    rows = [[""] + list(target)]
    rows += [[tok] + ["%.8g" % v for v in probs[r]] for r, tok in enumerate(toks)]
    rows.append(["position"] + [str(i + 1) for i in range(len(target))])
    rows.append(["consensus"] + consensus)
    rows.append(["different"] + [str(int(c != t)) for c, t in zip(consensus, target)])
    return rows


def write_table(handle, probs, toks, target):
    csv.writer(handle, delimiter="\t", lineterminator="\n").writerows(table_rows(probs, toks, target))


def read_table(handle):
    """Inverse of write_table: dict(target, toks, probs float64 [len(toks), L], position, consensus, different)."""
    rows = list(csv.reader(handle, delimiter="\t"))
    body = {r[0]: r[1:] for r in rows[1:]}
    toks = [r[0] for r in rows[1:] if r[0] not in SUMMARY_ROWS]
    return dict(target="".join(rows[0][1:]), toks=toks, probs=np.asarray([[float(v) for v in body[t]] for t in toks]),
                position=[int(v) for v in body["position"]], consensus="".join(body["consensus"]),
                different=[int(v) for v in body["different"]])


def pgen_msa(msa, outpath, steps, device, model, sampler=None, batch_size=None, show_progress_bar=True):
    msa = parse_fasta(msa, clean="upper")
    if sampler is None:
        sampler = ESM_MSA_sampler(model_map[model](), device=device)
    if steps is None:
        steps = len(msa[-1])
    probs, toks = sampler.probs_single(msa, steps=steps, show_progress_bar=show_progress_bar, batch_size=batch_size)
    with open(outpath, "w", newline="") as handle:
        write_table(handle, probs, toks, msa[-1])


def build_parser():
    parser = argparse.ArgumentParser(description=textwrap.dedent("""Masked-marginal probabilities of every symbol at every position of the
        last sequence of an MSA, under the ESM-MSA model (MI355X engine)."""), formatter_class=RawAndDefaultsFormatter)
    parser.add_argument("--msa", default=None, required=True, help="calculate the probabilities for the last sequence in this MSA.")
    parser.add_argument("-o", default=None, required=True, help="a tab separated file to write the probability table to")
    parser.add_argument("--steps", type=int, default=None, help="Randomly assign the input positions to this many mask bins, and mask "
                        "and predict one bin at a time. Default: one bin per position.")
    parser.add_argument("--batch_size", type=int, default=None, help="mask bins per forward (default: all of them; the table does not "
                        "depend on it)")
    parser.add_argument("--device", type=str, default="gpu", help="gpu (cuda:0) or cuda:[int]")
    parser.add_argument("--model", type=str, default="esm_msa1", choices=sorted(model_map), help="which model to use")
    add_engine_args(parser)
    return parser


def cli(argv=None):
    args = build_parser().parse_args(argv)
    seed_everything(args.seed)
    sampler = ESM_MSA_sampler(model_map[args.model](checkpoint=args.checkpoint, precision=args.precision, synthetic=args.synthetic_weights),
                              device=args.device)
    pgen_msa(args.msa, args.o, args.steps, args.device, args.model, sampler=sampler, batch_size=args.batch_size)


if __name__ == "__main__":
    cli(sys.argv[1:])
