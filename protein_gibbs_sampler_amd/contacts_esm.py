#!/usr/bin/env python3
"""Contact maps of FASTA sequences under an ESM masked LM (fair-esm's model.predict_contacts): one `<id>.npz` per record in the output
directory, holding `contacts`, float32 [L, L]: the probability that residues i and j are in contact, from the model's attention maps
through the average product correction and its logistic regression head.  ESM-1b, ESM-1v and the ESM-2 sizes.  Not in the reference."""
import argparse
import os

import numpy as np

from . import models
from ._cli import RawAndDefaultsFormatter, add_engine_args, model_kwargs
from .embed_esm import record_file_names
from .esm_sampler import ESM_sampler
from .fasta_io import parse_fasta

model_map = {"esm1b": models.ESM1b, "esm1v": models.ESM1v, **models.ESM2_MODELS}


def write_record(path, contacts):
    with open(path, "wb") as handle:
        np.savez(handle, contacts=np.ascontiguousarray(contacts, dtype=np.float32))


def main(input_h, out_dir, batch_size, sampler, max_map_bytes=None):
    names, seqs = parse_fasta(input_h, return_names=True, clean="unalign", full_name=True)      # the whole header: an error names the record
    files = record_file_names(names)              # an unsafe or duplicate id is refused before anything runs or is written
    os.makedirs(out_dir, exist_ok=True)
    for file_name, contacts in zip(files, sampler.predict_contacts_batch(seqs, batch_size, max_map_bytes)):
        write_record(os.path.join(out_dir, file_name), contacts)
    return files


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=RawAndDefaultsFormatter)
    parser.add_argument("-i", required=True, help="A fasta file with the sequences. Gaps and stop codons are removed first.")
    parser.add_argument("-o", required=True, help="output directory: one <id>.npz per record")
    parser.add_argument("--model", type=str, default="esm1v", choices=sorted(model_map), help="Which model to use.")
    parser.add_argument("--device", type=str, default="gpu", help="gpu (cuda:0) or cuda:[int]")
    parser.add_argument("--batch_size", type=int, default=None, help="sequences of equal length per forward (default: all of them, "
                        "within the memory cap of the attention maps); the result does not depend on it.")
    add_engine_args(parser)
    return parser


def cli(argv=None):
    args = build_parser().parse_args(argv)
    sampler = ESM_sampler(model_map[args.model](**model_kwargs(args)), device=args.device)
    with open(args.i) as input_handle:
        main(input_handle, args.o, args.batch_size, sampler)


if __name__ == "__main__":
    cli()
