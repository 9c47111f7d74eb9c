"""Shared pieces of the command-line front ends (pgen_*.py, likelihood_*.py, seq_probs_esm.py)."""
import argparse
import ast
import contextlib
import sys


class RawAndDefaultsFormatter(argparse.ArgumentDefaultsHelpFormatter, argparse.RawTextHelpFormatter):
    pass


def parse_line_args(text):
    """The second TSV column: a Python dict literal of sampler keyword arguments.

    The reference passes this column to eval() (src/pgen/pgen_esm.py:25).  Here it is parsed as a literal
    (ast.literal_eval) with `inf` / `float('inf')` accepted, which covers every form in the reference's README and
    examples without executing arbitrary code -- a deliberate, documented deviation."""
    src = text.replace("float('inf')", "1e999").replace('float("inf")', "1e999")
    tree = ast.parse(src.strip(), mode="eval")
    for node in ast.walk(tree):
        if isinstance(node, ast.Name) and node.id in ("inf", "Infinity"):
            node.__class__ = ast.Constant
            node.value = float("inf")
            node.kind = None
    out = ast.literal_eval(tree)
    if not isinstance(out, dict):
        raise ValueError("sampler arguments must be a dict literal, got: " + text)
    return out


GUIDE_EPILOG = """Guided draws (not in the reference; see INTEGRATION.md): top_p (nucleus truncation, in (0, 1]),
temperature_schedule (one temperature per iteration, or 'kind:t_start:t_end' with kind linear or geometric),
position_bias ({position: {residue: bias}}), allowed_residues ({position: 'DE'}), forbidden_residues ('C', or {position: 'C'});
positions are token positions, as for indexes (residue 0 behind <cls> is position 1)."""


def add_guide_args(parser):
    """--top_p / --temperature_schedule / --forbid of the front ends that take sampler arguments as flags (guided draws)."""
    parser.add_argument("--top_p", type=float, default=None, help="nucleus truncation of the draw after burn-in: sample from the "
                        "smallest set of most probable residues whose probability reaches this value, in (0, 1] (default: off).")
    parser.add_argument("--temperature_schedule", type=str, default=None, metavar="kind:t0:t1",
                        help="anneal the sampling temperature from t0 to t1 over the iterations; kind is linear or geometric (default: off).")
    parser.add_argument("--forbid", type=str, default=None, metavar="RESIDUES", help="residues that are never drawn, at any position, "
                        "e.g. C (default: none).")


def guide_kwargs(args):
    """The sampler keyword arguments of the flags of add_guide_args that were given."""
    kw = {}
    if getattr(args, "top_p", None) is not None:
        kw["top_p"] = args.top_p
    if getattr(args, "temperature_schedule", None) is not None:
        kw["temperature_schedule"] = args.temperature_schedule
    if getattr(args, "forbid", None):
        kw["forbidden_residues"] = args.forbid
    return kw


def add_engine_args(parser):
    parser.add_argument("--checkpoint", default=None, help="fair-esm .pt checkpoint to load (default: torch hub cache; it is an "
                        "error if none is found)")
    parser.add_argument("--synthetic-weights", dest="synthetic_weights", action="store_true",
                        help="opt in to seeded random weights of the model's architecture when no checkpoint is available "
                             "(benchmarks / plumbing tests: the output is not biologically meaningful)")
    parser.add_argument("--precision", default="auto", choices=["auto", "bf16", "fp16", "fp32"],
                        help="auto = fp16 operands with a range guard (weights scanned, one probe forward, non-finite logits "
                             "detected per call: falls back to bf16 with one warning); bf16 = the benchmarked throughput mode; "
                             "fp16 = the same kernels with fp16 operands, no fallback (8x smaller logit error than bf16, ~3 %% "
                             "slower); fp32 = parity mode (split-bf16 GEMMs and attention, logits within 1e-3 of fp32)")
    parser.add_argument("--seed", type=int, default=None, help="seed random and torch (positions and token draws) for reproducible output")


def add_scoring_args(parser, input_help, batch_size_default, batch_size_help, mask_distance_default="one position at a time",
                     csv_help="If set, then output will be a csv file.", model_choices=None):
    """The flags the scoring front ends share (likelihood_esm, seq_probs_esm, likelihood_esm_msa)."""
    parser.add_argument("-o", type=str, default=None, help="output table (default: stdout)")
    parser.add_argument("-i", default=None, help=input_help)
    parser.add_argument("--batch_size", type=int, default=batch_size_default, help=batch_size_help)
    parser.add_argument("--device", type=str, default="gpu", help="gpu (cuda:0) or cuda:[int]")
    parser.add_argument("--masking_off", action="store_true", default=False, help="If set, no masking is done.")
    parser.add_argument("--mask_distance", type=int, default=None,
                        help="mask several positions per copy, (mask_distance - 1) unmasked positions apart. Default: %s." % mask_distance_default)
    if model_choices is not None:
        parser.add_argument("--model", type=str, default="esm1v", choices=sorted(model_choices), help="Which model to use.")
    parser.add_argument("--csv", action="store_true", default=False, help=csv_help)


def mask_distance_from(args, refuse_with_masking_off=True):
    """--mask_distance as the samplers take it (absent: one position per copy), with the front ends' two argument errors."""
    mask_distance = float("inf") if args.mask_distance is None else args.mask_distance
    if mask_distance < 1:
        raise ValueError("mask distance must be an integer >= 1.")
    if refuse_with_masking_off and args.masking_off and args.mask_distance is not None:
        raise ValueError("--masking_off and --mask_distance are both set, that doesn't make sense.")
    return mask_distance


def model_kwargs(args):
    """The engine flags as the keyword arguments of the models.* constructors."""
    return dict(checkpoint=args.checkpoint, precision=args.precision, synthetic=args.synthetic_weights)


@contextlib.contextmanager
def open_io(args, newline=None):
    """(input handle, output handle) of -i / -o, stdin / stdout where a flag is absent; files it opened are closed on exit."""
    input_handle = open(args.i) if args.i is not None else sys.stdin
    output_handle = open(args.o, "w", newline=newline) if args.o is not None else sys.stdout
    try:
        yield input_handle, output_handle
    finally:
        if args.i is not None:
            input_handle.close()
        if args.o is not None:
            output_handle.close()


def seed_everything(seed):
    if seed is not None:
        import random
        import torch
        random.seed(seed)
        torch.manual_seed(seed)
