#!/usr/bin/env python3
"""Embeddings of FASTA sequences under an ESM masked LM (fair-esm's scripts/extract.py): one `<id>.npz` per record in the output
directory, with arrays `mean_<layer>` [d] (the residues only), `per_tok_<layer>` [L, d] and `bos_<layer>` [d] for every requested
layer under the number it was asked by (-1 = the last layer, through the final LayerNorm).  Not in the reference."""
import argparse
import os
import re

import numpy as np

from . import models
from ._cli import RawAndDefaultsFormatter, add_engine_args, model_kwargs
from .esm_sampler import ESM_sampler
from .fasta_io import parse_fasta

model_map = {"esm1b": models.ESM1b, "esm6": models.ESM6, "esm12": models.ESM12, "esm34": models.ESM34, "esm1v": models.ESM1v,
             **models.ESM2_MODELS}
_SAFE_ID = re.compile(r"^[A-Za-z0-9_.\-|=+@]+$")


def record_file_names(names):
    """<id>.npz for every record name, in order.  ValueError naming the record when its id -- the name up to the first blank -- is
    empty, holds a character outside A-Z a-z 0-9 _ . - | = + @, starts with a dot, or was already used by an earlier record."""
    seen = {}
    out = []
    for number, name in enumerate(names, 1):
        ident = name.split()[0] if name.split() else ""
        if not _SAFE_ID.match(ident) or ident.startswith("."):
            raise ValueError("record %d (%r): the id %r is not a safe file name" % (number, name, ident))
        if ident in seen:
            raise ValueError("record %d (%r): the id %r was already used by record %d" % (number, name, ident, seen[ident]))
        seen[ident] = number
        out.append(ident + ".npz")
    return out


def write_record(path, result):
    """One embed_batch result {"mean": {layer: a}, ...} as the arrays mean_<layer>, per_tok_<layer>, bos_<layer> of an .npz file."""
    arrays = {"%s_%d" % (kind, layer): a for kind, by_layer in result.items() for layer, a in by_layer.items()}
    with open(path, "wb") as handle:
        np.savez(handle, **arrays)


def main(input_h, out_dir, repr_layers, include, batch_size, sampler):
    names, seqs = parse_fasta(input_h, return_names=True, clean="unalign", full_name=True)      # the whole header: an error names the record
    files = record_file_names(names)              # refused before anything runs or is written
    os.makedirs(out_dir, exist_ok=True)
    for file_name, result in zip(files, sampler.embed_batch(seqs, repr_layers, include, batch_size)):
        write_record(os.path.join(out_dir, file_name), result)
    return files


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=RawAndDefaultsFormatter)
    parser.add_argument("-i", required=True, help="A fasta file with the sequences to embed. Gaps and stop codons are removed first.")
    parser.add_argument("-o", required=True, help="output directory: one <id>.npz per record")
    parser.add_argument("--model", type=str, default="esm1v", choices=sorted(model_map), help="Which model to use.")
    parser.add_argument("--device", type=str, default="gpu", help="gpu (cuda:0) or cuda:[int]")
    parser.add_argument("--repr_layers", type=int, nargs="+", default=[-1], help="layers to return: 0 = the embedding output, "
                        "l = the stream after block l, negative numbers count from the end (-1 = the last layer).")
    parser.add_argument("--include", type=str, nargs="+", default=["mean"], choices=list(ESM_sampler.EMBED_KINDS),
                        help="mean = average over the residues, per_tok = every residue's row, bos = the first token's row.")
    parser.add_argument("--batch_size", type=int, default=None, help="sequences of equal length per forward (default: all of them); "
                        "the result does not depend on it.")
    add_engine_args(parser)
    return parser


def cli(argv=None):
    args = build_parser().parse_args(argv)
    sampler = ESM_sampler(model_map[args.model](**model_kwargs(args)), device=args.device)
    with open(args.i) as input_handle:
        main(input_handle, args.o, args.repr_layers, args.include, args.batch_size, sampler)


if __name__ == "__main__":
    cli()
