"""Drop-in for `pgen.esm_sampler` (/root/reference/src/pgen/esm_sampler.py): same class, method names,
arguments, defaults, exceptions and messages; the per-iteration work runs on an MI355X.

What is kept verbatim in behaviour (citations = reference lines):
  * device grammar "cpu" | "gpu" | "cuda:N" and its three error messages            :66-78
  * seed cleaning / "<mask>" padding / list seeds drawn with random.choices           :95-126
  * num_positions / leader_length derivation and clamps, `indexes` rebinding (Q1)     :186-207
  * consumption order of the interpreter's RNG (choices per batch, sample per chain)  :112, :242-246
  * last-batch truncation, untokenize with "<mask>" left as text (Q6)                  :84-93, :236-239
What changes: the Python loops of :209-234 become one native call per batch
(`NativeMaskedLM.gibbs_run`), or -- for plug-in models that are not the HIP engine -- a device loop
whose mask scatter and draw are HIP kernels (`_gibbs.run_plugin_loop`).  The token draw uses the
engine's counter-based generator (pg_draw v1) keyed from torch's global RNG, since torch's serial
CPU multinomial stream cannot be reproduced by a data-parallel kernel (DESIGN.md "RNG contract").
"""
import ctypes
import math
import random
import re

import numpy as np
import torch
from tqdm import trange

from . import _gibbs, _lib, guides, sharding
from .engine import NativeMaskedLM

ESM_ALLOWED_AMINO_ACIDS = "ACDEFGHIKLMNPQRSTVWY"

_step_counter = [0]
_MUTATION = re.compile(r"^([A-Za-z])([0-9]+)([A-Za-z])$")


def parse_mutation(mutation):
    """"A24G" -> ("A", 23, "G"): wild-type residue, 0-based position (the text counts from 1), mutant residue."""
    m = _MUTATION.match(mutation.strip()) if isinstance(mutation, str) else None
    if not m or int(m.group(2)) < 1:
        raise ValueError("Invalid mutation %r: expected <wild type><1-based position><mutant>, such as 'A24G'" % (mutation,))
    wt, mut = m.group(1).upper(), m.group(3).upper()
    for aa in (wt, mut):
        if aa not in ESM_ALLOWED_AMINO_ACIDS:
            raise ValueError("Invalid mutation %r: %r is not one of %s" % (mutation, aa, ESM_ALLOWED_AMINO_ACIDS))
    return wt, int(m.group(2)) - 1, mut


def generate_step(out, gen_idx, temperature=None, top_k=0, sample=False, valid_idx=None, rng_seed=None, counter=None):
    """Generate a token id from out[gen_idx] (reference :8-45) on the GPU.

    out: logits [seq_len, vocab] (tensor or array); returns a 0-d int64 tensor like the reference.
    The draw is the HIP kernel behind pg_sample_writeback_device with P = 1.  `rng_seed`/`counter`
    pin the draw; by default a fresh counter value is used per call and the key comes from torch's
    global generator, so repeated calls are independent draws as in the reference.
    """
    if not torch.cuda.is_available():
        raise RuntimeError("generate_step needs an MI355X: the draw is a HIP kernel, there is no CPU implementation")
    dev = out.device if isinstance(out, torch.Tensor) and out.device.type == "cuda" else torch.device("cuda:0")
    logits = torch.as_tensor(out, dtype=torch.float32).to(dev).contiguous()
    if logits.dim() != 2:
        raise ValueError("out must be [seq_len, vocab]")
    width, V = logits.shape
    if valid_idx is None:
        valid_idx = list(range(V))
    if len(valid_idx) > 32:
        raise ValueError("at most 32 valid tokens are supported")
    if rng_seed is None:
        rng_seed = int(torch.randint(0, 2**62, (1,)).item())
    if counter is None:
        counter = _step_counter[0]
        _step_counter[0] += 1
    params = _lib.make_sample_params(False, 0, top_k, float("inf") if sample else 0, temperature, list(valid_idx), rng_seed,
                                     rng_stream=counter >> 32, row_id_base=counter & 0xFFFFFFFF)
    tok = torch.zeros((1, width), dtype=torch.int32, device=dev)
    idx = torch.tensor([[int(gen_idx) % width]], dtype=torch.int32, device=dev)
    picked = torch.empty((1, 1), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(_lib.lib().pg_sample_writeback_device(stream, ctypes.c_void_p(tok.data_ptr()), 1, width,
                                                         ctypes.c_void_p(logits.data_ptr()), V, ctypes.c_void_p(idx.data_ptr()),
                                                         None, 1, 1, ctypes.byref(params), 0,
                                                         ctypes.c_void_p(picked.data_ptr())))
    return torch.tensor(int(picked.item()))


class ESM_sampler():
    """adapted from bert-gen bert-babble.ipynb (via pgen.esm_sampler.ESM_sampler)"""

    def __init__(self, model, device="cpu"):
        """model: an object with attributes model, alphabet and batch_converter (reference :54-58)."""
        self.model = model
        self.model.model = self.model.model.eval()
        self.device, self.cuda = _gibbs.resolve_device(device)
        self.model.model.to(self.device)
        self.valid_aa_idx = sorted([self.model.alphabet.get_idx(tok) for tok in ESM_ALLOWED_AMINO_ACIDS])
        # key of the token-draw generator; None -> drawn from torch's global RNG once per generate()
        self.draw_seed = None
        self.rng_stream = 0
        # filled by generate(..., ) when self.record is True: per-batch dicts with tables / sampled logits / tokens
        self.record = False
        self.last_run = []
        # when torch.distributed is initialised with several ranks, generate() shards each batch over them
        self.shard_over_ranks = False    # opt-in (or PGIBBS_SHARD_OVER_RANKS=1): generate() splits every batch of ONE job over the torch.distributed ranks

    # ---- helpers with the reference's names ----------------------------------------------------
    def untokenize_batch(self, batch, bos, eos):
        start_offset = 1 if bos else 0
        end_offset = -1 if eos else 0
        if hasattr(batch, "numpy") and getattr(batch, "ndim", 0) == 2:       # a [B, T] token tensor: one table lookup per row
            arr = batch.numpy()
            return self.model.alphabet.decode_rows(arr[:, start_offset:arr.shape[1] + end_offset])
        if hasattr(batch, "tolist"):
            batch = batch.tolist()
        return ["".join([self.model.alphabet.get_tok(seq[i]) for i in range(0 + start_offset, len(seq) + end_offset)])
                for seq in batch]

    @staticmethod
    def clean_seed_seq(seed_to_clean):
        return _gibbs.clean_seed(seed_to_clean, ESM_ALLOWED_AMINO_ACIDS)

    def get_init_seq(self, seed_seq, max_len, batch_size=1):
        """Initial token batch: seeds right-padded with <mask> (reference :104-126).  A list of seeds consumes the
        interpreter's RNG once per batch (random.choices, :112) BEFORE any position draw."""
        if isinstance(seed_seq, list):
            seeds = random.choices(seed_seq, k=batch_size)
        elif isinstance(seed_seq, str):
            seeds = [seed_seq] * batch_size
        else:
            raise Exception("seed sequence should either be a string or list")
        rows = [(str(i), _gibbs.mask_padded(seed, max_len, ESM_ALLOWED_AMINO_ACIDS)) for i, seed in enumerate(seeds)]
        return self.model.batch_converter(rows)[2]

    def get_random_target_index(self, batch_size, indexes, num_positions):
        """== [random.sample(indexes, num_positions) for b in range(batch_size)] (reference :242-246),
        produced by the native CPython-exact generator on the interpreter's global RNG state."""
        from . import pyrandom
        return pyrandom.global_sample_table(list(indexes), num_positions, batch_size).tolist()

    def get_target_index_in_order(self, batch_size, indexes, next_i, num_positions):
        last_i, target = _gibbs.in_order_window(indexes, next_i, num_positions)
        return last_i, [target] * batch_size

    def mask_target_indexes(self, batch, target_indexes):
        """Reference :259-262.  Nested lists (as in the reference's unit test) are masked on the host; a
        device token tensor goes through the HIP scatter kernel."""
        mask_idx = self.model.alphabet.mask_idx
        if isinstance(batch, torch.Tensor) and batch.device.type == "cuda":
            table, _ = _gibbs.padded_positions(target_indexes)
            tok = batch.to(torch.int32).contiguous()
            d_table = torch.from_numpy(table).to(batch.device)
            with torch.cuda.device(batch.device):
                stream = ctypes.c_void_p(torch.cuda.current_stream(batch.device).cuda_stream)
                _lib.check(_lib.lib().pg_mask_scatter_device(stream, ctypes.c_void_p(tok.data_ptr()), tok.shape[0], tok.shape[1],
                                                             ctypes.c_void_p(d_table.data_ptr()), None, table.shape[0], table.shape[1],
                                                             mask_idx))
            batch.copy_(tok.to(batch.dtype))
            return
        for batch_index in range(len(target_indexes)):
            for kk in target_indexes[batch_index]:
                batch[batch_index][kk] = mask_idx

    def calculate_indexes(self, indexes, leader_length, max_len, rollover_from_start):
        return _gibbs.candidate_indexes(indexes, leader_length, max_len, rollover_from_start)

    def _require_gpu(self, what, why="there is no CPU implementation"):
        if not self.cuda:
            raise RuntimeError("ESM_sampler.%s needs device 'gpu'/'cuda:N' on an MI355X: %s" % (what, why))

    # ---- the sampler -----------------------------------------------------------------------------
    def generate(self, n_samples, seed_seq, batch_size=1, in_order=False, max_len=None, leader_length=0,
                 leader_length_percent=None, top_k=0, temperature=None, num_iters=10, burnin=float('inf'), mask=True,
                 num_positions=0, num_positions_percent=None, indexes=None, rollover_from_start=False,
                 show_progress_bar=True, top_p=None, temperature_schedule=None, position_bias=None, allowed_residues=None,
                 forbidden_residues=None):
        """generate sequences -- arguments exactly as pgen.esm_sampler.ESM_sampler.generate (reference :128-170), then the five
        of a guided draw, which the reference does not have (guides.DrawGuide; pg_draw v2): top_p in (0, 1],
        temperature_schedule (one temperature per iteration, or "kind:t_start:t_end"; at least num_iters long; `temperature` is
        then not used), position_bias, allowed_residues, forbidden_residues -- keyed by token position, as `indexes` is."""
        guide = guides.from_arguments(top_p, temperature_schedule, position_bias, allowed_residues, forbidden_residues)
        if isinstance(seed_seq, str):
            sequence_length = len(seed_seq)
        elif isinstance(seed_seq, list):
            sequence_length = max(len(seed) for seed in seed_seq)
        else:
            raise ValueError("Unknown seed sequence format, expecting str or list")

        sequences = []
        n_batches = math.ceil(n_samples / batch_size)
        if max_len is None:
            max_len = sequence_length
        num_positions, leader_length = _gibbs.derive_counts(max_len, num_positions, num_positions_percent, leader_length,
                                                            leader_length_percent)

        self._require_gpu("generate", "this package implements the Gibbs hot path as HIP kernels only and has no CPU implementation")
        draw_seed = _gibbs.draw_seed(self)
        self.last_run = []
        # several torch.distributed ranks (one per GPU): every batch is split contiguously over them
        ctx = _gibbs.shard_context(self, isinstance(self.model.model, NativeMaskedLM), lambda: (
            n_samples, seed_seq, batch_size, in_order, max_len, leader_length, top_k, temperature, num_iters, burnin, mask,
            num_positions, None if indexes is None else list(indexes), rollover_from_start, self.rng_stream,
            None if guide is None else guide.digest_parts()), "ESM_sampler.generate")
        if ctx is not None:
            draw_seed = sharding.broadcast_object(ctx, draw_seed)

        for batch_n in trange(n_batches, disable=(not show_progress_bar)):
            batch = self.get_init_seq(seed_seq, max_len, batch_size)

            indexes, last_i = self.calculate_indexes(indexes, leader_length, max_len, rollover_from_start)
            indexes = _gibbs.normalise_indexes(indexes, batch.shape[1])     # IndexError / negative wrap as batch[b][kk]
            if num_positions > len(indexes):
                num_positions = len(indexes)

            table, last_i = _gibbs.build_target_table(num_iters, (batch_size,), indexes, num_positions, in_order, last_i)
            params = _lib.make_sample_params(mask, self.model.alphabet.mask_idx, top_k, burnin, temperature, self.valid_aa_idx,
                                             draw_seed, rng_stream=self.rng_stream, row_id_base=batch_n * batch_size)
            batch = _gibbs.run_gibbs_batch(self, ctx, batch, table, params, batch_n * batch_size, 1, record_plugin=True,
                                           guide=guides.compile_for(self, guide, batch.shape[1], num_iters))

            strs = self.untokenize_batch(batch, self.model.alphabet.prepend_bos, self.model.alphabet.append_eos)
            if batch_n == (n_batches - 1):
                sequences += strs[0:n_samples - len(sequences)]
            else:
                sequences += strs
        return sequences

    # ---- masked log-likelihood (reference :277-363) ---------------------------------------------------
    def log_likelihood(self, seq, with_masking=True, verbose=False, mask_distance=float("inf"), batch_size=None):
        """(mean log-likelihood, per-position list) of one sequence -- see log_likelihood_batch."""
        return next(self.log_likelihood_batch([seq], with_masking, verbose, mask_distance, batch_size))

    def log_likelihood_batch(self, seq_list, with_masking=True, verbose=False, mask_distance=float("inf"), batch_size=None):
        """Same contract as pgen.esm_sampler.ESM_sampler.log_likelihood_batch: yields (float mean, list[float]).
        with_masking: min(mask_distance, len) copies of the sequence, copy i masked at every
        num_copies-th position starting at i; the log-probability of the original residue is read at the masked
        positions.  The forward, log-softmax and gather run on the GPU (pg_esm_forward_logprobs: the LM head is
        evaluated only at the scored rows)."""
        self._require_gpu("log_likelihood_batch")
        for job in self._masked_copy_jobs(seq_list, with_masking, mask_distance, batch_size):
            likelihood_sum = np.float32(0.0)
            likelihood_list = []
            for sl, first in job["chunks"]:
                nb = job["copies"][sl].shape[0]
                lp = _gibbs.score_positions(self.model.model, job["copies"][sl], np.arange(nb), job["idx"][sl], job["tgt"][sl], self.device)
                for i in range(nb):
                    # the reference appends in (copy, position) order; positions of one copy ascend (stride n)
                    for p in range(len(job["pos_of"][first + i])):
                        likelihood_sum = np.float32(likelihood_sum + lp[i, p])
                        likelihood_list.append(float(lp[i, p]))
            yield (float(likelihood_sum / np.float32(len(job["seq"]))), likelihood_list)

    def _masked_copy_jobs(self, seq_list, with_masking, mask_distance, batch_size):
        """What log_likelihood_batch and masked_marginals_batch run, one job per sequence: `copies` [n, T] (copy i masked at every
        n-th position starting at i, n = min(mask_distance, len); one unmasked copy without masking), `pos_of[i]` the token positions
        read from copy i, `idx` / `tgt` [n, P] the same positions (-1 padded) and the original tokens there, `chunks` the
        (slice, first copy) of every forward of `batch_size` copies, `start` the token position of residue 0."""
        n_batches = len(seq_list)
        if batch_size is None:
            batch_size = n_batches
        reformatted_seq = [(str(idx), self.clean_seed_seq(seq)) for idx, seq in enumerate(seq_list)]
        _, _, tokens = self.model.batch_converter(reformatted_seq)
        range_start = 1 if self.model.alphabet.prepend_bos else 0
        end_modifier = -1 if self.model.alphabet.append_eos else 0
        batch_range_end = [len(seq) + range_start for seq in seq_list]
        overall_range_end = tokens.shape[1] + end_modifier
        assert max(len(seq) for seq in seq_list) == len(range(range_start, overall_range_end))
        old_toks = tokens.numpy()
        mask_idx = self.model.alphabet.mask_idx
        for seq_idx in range(len(reformatted_seq)):
            original_string = reformatted_seq[seq_idx][1]
            end = batch_range_end[seq_idx]
            # tokens of THIS sequence alone (no padding reaches the model, as in the reference's masked path)
            _, _, one = self.model.batch_converter([(0, original_string)])
            if with_masking:
                copies, pos_of = _gibbs.strided_mask_copies(one, int(min(mask_distance, len(original_string))), range_start, end,
                                                            mask_idx)
                assert sum(len(p) for p in pos_of) == len(original_string)
            else:
                copies, pos_of = one, [list(range(range_start, end))]
            idx, tgt = _gibbs.padded_positions(pos_of, [old_toks[seq_idx]] * len(pos_of))
            yield dict(seq=seq_list[seq_idx], copies=copies, pos_of=pos_of, idx=idx, tgt=tgt,
                       chunks=list(_gibbs.chunks(len(pos_of), batch_size)), start=range_start)

    # ---- masked-marginal substitution tables (the zero-shot variant scoring ESM-1v was released for) ---------
    def masked_marginals(self, seq, with_masking=True, mask_distance=float("inf"), batch_size=None, normalise="vocab"):
        """(logp, entropy, toks) of one sequence -- see masked_marginals_batch."""
        return next(self.masked_marginals_batch([seq], with_masking, mask_distance, batch_size, normalise))

    def masked_marginals_batch(self, seq_list, with_masking=True, mask_distance=float("inf"), batch_size=None, normalise="vocab"):
        """For every sequence yields (logp float32 [L, 20], entropy float32 [L] in nats, toks): logp[i, c] = log-probability of
        residue toks[c] (the tokens of self.valid_aa_idx, in that order) at position i, read from the copy in which position i is
        masked.  The masked copies, position lists and `batch_size` chunks are log_likelihood_batch's, so the forwards are the same
        launches on the same data; only the last step keeps the row instead of one entry of it (pg_esm_forward_logprob_table).
        normalise "vocab": log_softmax over the model's whole vocabulary -- logp at a position's own residue is bit for bit what
        log_likelihood_batch lists there; "columns": over the 20 residues only (rows sum to 1)."""
        self._require_gpu("masked_marginals_batch")
        if normalise not in _lib.TABLE_NORMS:
            raise ValueError("normalise must be 'vocab' or 'columns', got %r" % (normalise,))
        toks = [self.model.alphabet.get_tok(i) for i in self.valid_aa_idx]
        for job in self._masked_copy_jobs(seq_list, with_masking, mask_distance, batch_size):
            L = len(job["seq"])
            logp = np.zeros((L, len(self.valid_aa_idx)), dtype=np.float32)
            entropy = np.zeros(L, dtype=np.float32)
            for sl, first in job["chunks"]:
                nb = job["copies"][sl].shape[0]
                tab, ent = _gibbs.score_table(self.model.model, job["copies"][sl], np.arange(nb), job["idx"][sl], self.valid_aa_idx,
                                              self.device, normalise, want_entropy=True)
                for i in range(nb):
                    pos = np.asarray(job["pos_of"][first + i], dtype=np.int64) - job["start"]
                    logp[pos] = tab[i, :len(pos)]
                    entropy[pos] = ent[i, :len(pos)]
            yield logp, entropy, toks

    # ---- sequence embeddings (fair-esm's repr_layers / scripts/extract.py) ------------------------------------
    EMBED_KINDS = ("mean", "per_tok", "bos")

    def embed(self, seq, repr_layers=(-1,), include=("mean",), batch_size=None):
        """The embeddings of one sequence -- see embed_batch."""
        return next(self.embed_batch([seq], repr_layers, include, batch_size))

    def embed_batch(self, seq_list, repr_layers=(-1,), include=("mean",), batch_size=None):
        """For every sequence, in order, yields a dict of the `include`d kinds, each {layer: float32 array} under the layer numbers as
        written in repr_layers (negative numbers count from the end, -1 = the last layer through emb_layer_norm_after):
        "mean" [d] over the residues only (not <cls> / <eos>), "per_tok" [L, d] the residue rows, "bos" [d] the first token's row.
        Sequences of equal length form one group and a group runs in chunks of batch_size (None: whole groups), so no padding
        reaches the model; every chunk is a shard of its group's job (set_job_items), so a sequence's result does not depend on
        batch_size.  The means are the engine's sequential fp32 means (pg_esm_forward_representations)."""
        self._require_gpu("embed_batch")
        include = tuple(include)
        if not include or any(kind not in self.EMBED_KINDS for kind in include):
            raise ValueError("include takes some of %r, got %r" % (self.EMBED_KINDS, include))
        lm = self.model.model
        if not isinstance(lm, NativeMaskedLM):
            raise TypeError("embed_batch needs the HIP engine (NativeMaskedLM); a plug-in model returns its own representations")
        layers = list(repr_layers)
        lm.normalise_layers(layers)                     # refuses before anything runs
        seqs = [self.clean_seed_seq(seq) for seq in seq_list]
        start = 1 if self.model.alphabet.prepend_bos else 0
        groups = {}
        for i, seq in enumerate(seqs):
            groups.setdefault(len(seq), []).append(i)
        kinds = [kind for kind in ("mean", "bos") if kind in include]      # the pools of a call, in this order
        done = {}
        for i, seq in enumerate(seqs):
            if i not in done:
                self._embed_group(lm, seqs, groups[len(seq)], layers, kinds, "per_tok" in include, start, batch_size, done)
            yield done.pop(i)

    def _embed_group(self, lm, seqs, members, layers, kinds, per_tok, start, batch_size, done):
        """embed_batch on one group of equally long sequences: done[i] = the result of sequence i for every member i."""
        L = len(seqs[members[0]])
        ranges = {"mean": (start, L), "bos": (0, 1)}
        for tok, first in self._group_chunks(lm, seqs, members, batch_size):
            pools = np.asarray([[ranges[kind]] * len(tok) for kind in kinds], dtype=np.int32) if kinds else None
            rows, means = lm.forward_representations(tok, layers, pools, per_token=per_tok)
            for b in range(len(tok)):
                out = {kind: {layer: means[k, p, b].copy() for k, layer in enumerate(layers)} for p, kind in enumerate(kinds)}
                if per_tok:
                    out["per_tok"] = {layer: rows[k, b, start:start + L].copy() for k, layer in enumerate(layers)}
                done[members[first + b]] = out

    def _group_chunks(self, lm, seqs, members, batch_size, max_items=None):
        """The grouping of embed_batch and predict_contacts_batch: the equally long sequences `members` as one token batch (no <pad>
        reaches the model), yielded as (tokens of a chunk, index of its first member) in chunks of batch_size (None: the whole group),
        cut further to max_items sequences when given.  Every chunk is a shard of the group's job (set_job_items while the generator
        runs), so a sequence's result does not depend on the chunking."""
        _, _, tokens = self.model.batch_converter([(str(i), seqs[i]) for i in members])
        tokens = tokens.numpy()
        size = len(members) if batch_size is None else batch_size
        if max_items is not None:
            size = max(1, min(size, max_items))
        lm.set_job_items(len(members))
        try:
            for sl, first in _gibbs.chunks(len(members), size):
                yield tokens[sl], first
        finally:
            lm.set_job_items(0)

    # ---- contact prediction (fair-esm's predict_contacts) ----------------------------------------------------
    CONTACT_MAP_BYTES = 1 << 30      # default cap on one call's staged attention maps (B * n_heads * T * T fp32)

    def predict_contacts(self, seq):
        """Contact probabilities of one sequence: float32 [L, L] over its residues -- see predict_contacts_batch."""
        return next(self.predict_contacts_batch([seq]))

    def predict_contacts_batch(self, seq_list, batch_size=None, max_map_bytes=None):
        """For every sequence, in order, yields its contact probabilities float32 [L, L] (residues only).  The grouping is
        embed_batch's (_group_chunks); a chunk is also cut so that the one layer of attention maps the engine stages for it,
        B * n_heads * T * T * 4 bytes, stays under max_map_bytes (default CONTACT_MAP_BYTES = 1 GiB; one sequence always runs).
        The result does not depend on batch_size or the cap."""
        self._require_gpu("predict_contacts_batch")
        lm = self.model.model
        if not isinstance(lm, NativeMaskedLM):
            raise TypeError("predict_contacts_batch needs the HIP engine (NativeMaskedLM)")
        predict = getattr(self.model, "predict_contacts", None) or lm.predict_contacts      # the holder's refusals (models.py) first
        cap = self.CONTACT_MAP_BYTES if max_map_bytes is None else int(max_map_bytes)
        if cap < 1:
            raise ValueError("max_map_bytes must be positive, got %r" % (max_map_bytes,))
        seqs = [self.clean_seed_seq(seq) for seq in seq_list]
        if any(len(seq) < 1 for seq in seqs):
            raise ValueError("predict_contacts_batch: an empty sequence has no contact map")
        groups = {}
        for i, seq in enumerate(seqs):
            groups.setdefault(len(seq), []).append(i)
        done = {}
        for i, seq in enumerate(seqs):
            if i not in done:
                members = groups[len(seq)]
                T = len(seq) + 2
                per_seq = lm.cfg["n_heads"] * T * T * 4
                for tok, first in self._group_chunks(lm, seqs, members, batch_size, max_items=max(1, cap // per_seq)):
                    maps = predict(tok)
                    for b in range(len(tok)):
                        done[members[first + b]] = maps[b].copy()
            yield done.pop(i)

    def score_mutations(self, seq, mutations, **kwargs):
        """Masked-marginal scores of point mutations such as "A24G" (wild type, 1-based position, mutant):
        logp[pos, mutant] - logp[pos, wild type], all from ONE masked_marginals table of `seq` (keyword arguments go to it).
        ValueError, naming the mutation, when its wild type is not the residue `seq` has there.  Returns a list of floats."""
        seq = self.clean_seed_seq(seq)
        parsed = []
        for mutation in mutations:
            wt, pos, mut = parse_mutation(mutation)
            if pos >= len(seq):
                raise ValueError("Mutation %r: position %d is beyond the sequence of %d residues" % (mutation, pos + 1, len(seq)))
            if seq[pos] != wt:
                raise ValueError("Mutation %r: the sequence has %r at position %d, not %r" % (mutation, seq[pos], pos + 1, wt))
            parsed.append((wt, pos, mut))
        if not parsed:
            return []
        logp, _, toks = self.masked_marginals(seq, **kwargs)
        col = {t: c for c, t in enumerate(toks)}
        return [float(logp[pos, col[mut]] - logp[pos, col[wt]]) for wt, pos, mut in parsed]
