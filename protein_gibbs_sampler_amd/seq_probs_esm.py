#!/usr/bin/env python3
"""Masked-marginal substitution tables of FASTA sequences under an ESM masked LM (zero-shot variant scoring): every position is
masked, the model runs, and the log-probability of each of the 20 residues there is written.  Input and output flags as
likelihood_esm.py.

Output: a long-format table, one row per (sequence id, 1-based position): id, position, wt (the sequence's own residue), the 20
log-probabilities (columns named by residue, in the sampler's token order) and the entropy of the position's distribution in nats.
The score of a substitution is row[mutant] - row[wt]."""
import argparse
import csv
import textwrap

from ._cli import RawAndDefaultsFormatter, add_engine_args, add_scoring_args, mask_distance_from, model_kwargs, open_io
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
    add_scoring_args(parser, "A fasta file with sequences to score. Gaps and stop codons are removed first.", None,
                     "masked copies of a sequence per forward (default: the number of sequences in the input, as "
                     "ESM_sampler.log_likelihood_batch counts it).", model_choices=model_map)
    parser.add_argument("--normalise", type=str, default="vocab", choices=["vocab", "columns"],
                        help="vocab: log-softmax over the model's whole vocabulary (as likelihood_esm); columns: over the 20 residues only.")
    add_engine_args(parser)
    return parser


def cli(argv=None):
    args = build_parser().parse_args(argv)
    mask_distance = mask_distance_from(args)
    sampler = ESM_sampler(model_map[args.model](**model_kwargs(args)), device=args.device)
    with open_io(args, newline="") as (input_handle, output_handle):
        main(input_handle, output_handle, args.masking_off, mask_distance, args.batch_size, args.normalise, args.csv, sampler)


if __name__ == "__main__":
    cli()
