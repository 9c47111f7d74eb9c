#!/usr/bin/env python3
"""Masked-marginal substitution tables of FASTA sequences under an ESM masked LM (zero-shot variant scoring): every position is
masked, the model runs, and the log-probability of each of the 20 residues there is written.  Input and output flags as
likelihood_esm.py.

Output: a long-format table, one row per (sequence id, 1-based position): id, position, wt (the sequence's own residue), the 20
log-probabilities (columns named by residue, in the sampler's token order) and the entropy of the position's distribution in nats.
The score of a substitution is row[mutant] - row[wt]."""
import argparse
import csv
import sys
import textwrap

from ._cli import RawAndDefaultsFormatter, add_engine_args
from .esm_sampler import ESM_sampler
from .fasta_io import parse_fasta
from .likelihood_esm import model_map

FIXED_COLUMNS = ("id", "position", "wt")


def write_rows(writer, name, seq, logp, entropy):
    for i, wt in enumerate(seq):
        writer.writerow([name, str(i + 1), wt] + ["%.8g" % v for v in logp[i]] + ["%.8g" % entropy[i]])


def write_header(writer, toks):
    writer.writerow(list(FIXED_COLUMNS) + list(toks) + ["entropy"])


def read_table(handle, sep="\t"):
    """Inverse of the writer: (toks, {id: dict(seq, logp [L][20] floats, entropy [L] floats)}), positions in file order."""
    rows = list(csv.reader(handle, delimiter=sep))
    header = rows[0]
    if tuple(header[:3]) != FIXED_COLUMNS or header[-1] != "entropy":
        raise ValueError("not a substitution table: header %r" % (header,))
    toks = header[3:-1]
    out = {}
    for r in rows[1:]:
        rec = out.setdefault(r[0], dict(seq="", logp=[], entropy=[]))
        if int(r[1]) != len(rec["seq"]) + 1:
            raise ValueError("positions of %r are not consecutive at %r" % (r[0], r[1]))
        rec["seq"] += r[2]
        rec["logp"].append([float(v) for v in r[3:-1]])
        rec["entropy"].append(float(r[-1]))
    return toks, out


def main(input_h, output_h, masking_off, mask_distance, batch_size, normalise, csv_out, sampler):
    names, seqs = parse_fasta(input_h, return_names=True, clean="unalign")
    writer = csv.writer(output_h, delimiter="," if csv_out else "\t", lineterminator="\n")
    header_done = False
    tables = sampler.masked_marginals_batch(seqs, with_masking=not masking_off, mask_distance=mask_distance, batch_size=batch_size,
                                            normalise=normalise)
    for name, seq, (logp, entropy, toks) in zip(names, seqs, tables):
        if not header_done:
            write_header(writer, toks)
            header_done = True
        write_rows(writer, name, sampler.clean_seed_seq(seq), logp, entropy)
        output_h.flush()


def build_parser():
    parser = argparse.ArgumentParser(description=textwrap.dedent("""Masked-marginal log-probabilities of every residue at every position
    of the sequences of a fasta file, under an ESM BERT model.

    writes a tab separated output file with columns:
    sequence name, position, wild type, 20 log-probabilities, entropy
    """), formatter_class=RawAndDefaultsFormatter)
    parser.add_argument("-o", type=str, default=None, help="output table (default: stdout)")
    parser.add_argument("-i", default=None, help="A fasta file with sequences to score. Gaps and stop codons are removed first.")
    parser.add_argument("--batch_size", type=int, default=None, help="masked copies of a sequence per forward (default: the number of sequences in the input, as ESM_sampler.log_likelihood_batch counts it).")
    parser.add_argument("--device", type=str, default="gpu", help="gpu (cuda:0) or cuda:[int]")
    parser.add_argument("--masking_off", action="store_true", default=False, help="If set, no masking is done.")
    parser.add_argument("--mask_distance", type=int, default=None,
                        help="mask several positions per copy, (mask_distance - 1) unmasked positions apart. Default: one position at a time.")
    parser.add_argument("--model", type=str, default="esm1v", choices=sorted(model_map), help="Which model to use.")
    parser.add_argument("--normalise", type=str, default="vocab", choices=["vocab", "columns"],
                        help="vocab: log-softmax over the model's whole vocabulary (as likelihood_esm); columns: over the 20 residues only.")
    parser.add_argument("--csv", action="store_true", default=False, help="If set, then output will be a csv file.")
    add_engine_args(parser)
    return parser


def cli(argv=None):
    args = build_parser().parse_args(argv)
    mask_distance = float("inf") if args.mask_distance is None else args.mask_distance
    if mask_distance < 1:
        raise ValueError("mask distance must be an integer >= 1.")
    if args.masking_off and args.mask_distance is not None:
        raise ValueError("--masking_off and --mask_distance are both set, that doesn't make sense.")
    sampler = ESM_sampler(model_map[args.model](checkpoint=args.checkpoint, precision=args.precision, synthetic=args.synthetic_weights), device=args.device)
    input_handle = open(args.i) if args.i is not None else sys.stdin
    output_handle = open(args.o, "w", newline="") if args.o is not None else sys.stdout
    try:
        main(input_handle, output_handle, args.masking_off, mask_distance, args.batch_size, args.normalise, args.csv, sampler)
    finally:
        if args.i is not None:
            input_handle.close()
        if args.o is not None:
            output_handle.close()


if __name__ == "__main__":
    cli()
