#!/usr/bin/env python3
"""Contact maps of alignments under the MSA Transformer (fair-esm's esm_msa1b return_contacts=True): every input file is one aligned
FASTA whose first record is the query sequence; one `<file stem>.npz` per alignment in the output directory, holding `contacts`,
float32 [L, L] over the alignment's L columns: the probability that residues i and j of the query are in contact, from the model's
tied row-attention maps through the average product correction and its logistic regression head.  Not in the reference."""
import argparse
import os

from . import models
from ._cli import RawAndDefaultsFormatter, add_engine_args, model_kwargs
from .contacts_esm import write_record
from .embed_esm import record_file_names
from .esm_msa_sampler import ESM_MSA_sampler
from .fasta_io import parse_fasta


def alignment_file_names(paths):
    """<file stem>.npz for every input path, in order; an unsafe stem or one used twice is refused (record_file_names)."""
    stems = [os.path.splitext(os.path.basename(path))[0] for path in paths]
    for number, (path, stem) in enumerate(zip(paths, stems), 1):
        if stem.split() != [stem]:                # record_file_names reads an id up to the first blank; a file stem is the whole name
            raise ValueError("file %d (%r): the stem %r is not a safe file name" % (number, path, stem))
    return record_file_names(stems)


def read_alignment(path, delete_insertions=False):
    """The rows of one aligned FASTA (lower case -> upper and '.' -> '-', or insertions deleted); ValueError naming the file when it
    is empty or its rows are not equally long."""
    with open(path) as handle:
        rows = parse_fasta(handle, clean="delete" if delete_insertions else "upper")
    if not rows:
        raise ValueError("%s: no sequences" % path)
    if any(len(row) != len(rows[0]) for row in rows):
        raise ValueError("%s: the rows are not equally long: not an alignment" % path)
    return rows


def main(paths, out_dir, batch_size, sampler, max_map_bytes=None, delete_insertions=False):
    files = alignment_file_names(paths)           # an unsafe or duplicate output name is refused before anything runs or is written
    msas = [read_alignment(path, delete_insertions) for path in paths]
    os.makedirs(out_dir, exist_ok=True)
    for file_name, contacts in zip(files, sampler.predict_contacts_batch(msas, batch_size, max_map_bytes)):
        write_record(os.path.join(out_dir, file_name), contacts)
    return files


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=RawAndDefaultsFormatter)
    parser.add_argument("-i", required=True, nargs="+", help="aligned fasta files, one alignment each; the first record is the query.")
    parser.add_argument("-o", required=True, help="output directory: one <file stem>.npz per alignment")
    parser.add_argument("--device", type=str, default="gpu", help="gpu (cuda:0) or cuda:[int]")
    parser.add_argument("--batch_size", type=int, default=None, help="alignments of equal depth and width per forward (default: all of "
                        "them, within the memory cap of the attention maps); the result does not depend on it.")
    parser.add_argument("--delete_insertions", action="store_true", default=False,
                        help="remove all lowercase and '.' characters from the rows. Default: lower -> upper and '.' -> '-'.")
    add_engine_args(parser)
    return parser


def cli(argv=None):
    args = build_parser().parse_args(argv)
    alignment_file_names(args.i)                  # before the model is loaded
    sampler = ESM_MSA_sampler(models.ESM_MSA1(**model_kwargs(args)), device=args.device)
    main(args.i, args.o, args.batch_size, sampler, delete_insertions=args.delete_insertions)


if __name__ == "__main__":
    cli()
