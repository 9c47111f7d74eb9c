#!/usr/bin/env python3
"""Average log-likelihood of FASTA sequences under an ESM masked LM, with the surface of the reference's
`likelihood_esm.py` (/root/reference/src/pgen/likelihood_esm.py:15-57 loop and table format, :60-104 flags):
output is `id<sep>score` rows (tab or comma), optionally a second table with the ';'-joined per-position
log-likelihoods rounded to 3 decimals."""
import argparse
import textwrap

from . import models
from ._cli import RawAndDefaultsFormatter, add_engine_args, add_scoring_args, mask_distance_from, model_kwargs, open_io
from .esm_sampler import ESM_sampler
from .fasta_io import parse_fasta

POSITIONAL_SCORE_SEP = ";"
model_map = {"esm1b": models.ESM1b, "esm6": models.ESM6, "esm12": models.ESM12, "esm34": models.ESM34, "esm1v": models.ESM1v,
             **models.ESM2_MODELS}


def main(input_h, output_h, masking_off, device, model, batch_size, mask_distance, csv, score_name, positionwise=None, sampler=None):
    if sampler is None:
        sampler = ESM_sampler(model_map[model](), device=device)
    records = list(zip(*parse_fasta(input_h, return_names=True, clean="unalign")))
    sep = "," if csv else "\t"
    if score_name is None:
        score_name = model
    positionwise_h = open(positionwise, "w") if positionwise is not None else None
    try:
        print(f"id{sep}{score_name}", file=output_h)
        if positionwise_h is not None:
            print(f"id{sep}{score_name}", file=positionwise_h)
        for start in range(0, len(records), batch_size):
            chunk = records[start:start + batch_size]
            scores = sampler.log_likelihood_batch([seq for _, seq in chunk], with_masking=not masking_off,
                                                  mask_distance=mask_distance, batch_size=batch_size)
            for (name, _), (score, positional) in zip(chunk, scores):
                print(f"{name}{sep}{score}", file=output_h)
                if positionwise_h is not None:
                    print(f"{name}{sep}{POSITIONAL_SCORE_SEP.join(str(round(x, 3)) for x in positional)}", file=positionwise_h)
            output_h.flush()
            if positionwise_h is not None:
                positionwise_h.flush()
    finally:
        if positionwise_h is not None:
            positionwise_h.close()


def build_parser():
    parser = argparse.ArgumentParser(description=textwrap.dedent("""Calculates average log likelihood of a fasta ESM BERT model.

    writes a tab separated output file with columns:
    sequence name, score
    """), formatter_class=RawAndDefaultsFormatter)
    add_scoring_args(parser, "A fasta file with sequences to score. Gaps and stop codons are removed first.", 1,
                     "How many sequences to batch together.", model_choices=model_map)
    parser.add_argument("--score_name", type=str, default=None, help="name of the second column (default: the model name).")
    parser.add_argument("--positionwise", type=str, default=None, help="also write per-position log likelihoods (';' separated) to this file.")
    add_engine_args(parser)
    return parser


def cli(argv=None):
    args = build_parser().parse_args(argv)
    mask_distance = mask_distance_from(args)
    sampler = ESM_sampler(model_map[args.model](**model_kwargs(args)), device=args.device)
    with open_io(args) as (input_handle, output_handle):
        main(input_handle, output_handle, args.masking_off, args.device, args.model, args.batch_size, mask_distance, args.csv,
             args.score_name, args.positionwise, sampler=sampler)


if __name__ == "__main__":
    cli()
