"""Drop-in for `pgen.esm_msa_sampler` (/root/reference/src/pgen/esm_msa_sampler.py): same class, method
names, arguments, defaults and errors; per-iteration work on an MI355X.

Kept in behaviour (citations = reference lines): `partition` :13-31; device grammar :47-61; seed
cleaning with the 21-symbol alphabet :93-99; `<mask>` padding through the patched MSA batch converter
:78-90; `generate` bookkeeping (rounds, num_positions from sequence_length, `indexes` rebinding)
:189-218; RNG consumption order (one random.sample per (msa, row), :272-279; one random.shuffle per
pass, :129); `generate_single` masking row -1 while sampling `target_index` (quirk Q2, :133-145).
"""
import contextlib
import math

import numpy as np
import torch
from tqdm import tqdm, trange

from . import _gibbs, _lib, guides, sharding
from .engine import NativeMaskedLM
from .esm_sampler import generate_step  # noqa: F401  (same re-export as the reference, :6)

ESM_MSA_ALLOWED_AMINO_ACIDS = "-ACDEFGHIKLMNPQRSTVWY"
ESM_MSA_GAP_CHARACTERS = "-"


def partition(input_list, num_partitions):
    """Contiguous split into <= num_partitions near-equal parts, the first `remainder` parts one longer
    (reference :13-31; an empty input divides by zero there as well)."""
    if len(input_list) < num_partitions:
        num_partitions = len(input_list)
    num_per_partition = len(input_list) // num_partitions
    remainder = len(input_list) % num_partitions
    out, pos = [], 0
    for i in range(num_partitions):
        n = num_per_partition + (1 if i < remainder else 0)
        out.append(list(input_list[pos:pos + n]))
        pos += n
    return out


class ESM_MSA_sampler():
    """adapted from bert-gen bert-babble.ipynb (via pgen.esm_msa_sampler.ESM_MSA_sampler)"""

    def __init__(self, model, device="cpu"):
        self.model = model
        self.model.model = self.model.model.eval()
        self.device, self.cuda = _gibbs.resolve_device(device)
        self.model.model.to(self.device)
        self.valid_aa_idx = sorted([self.model.alphabet.get_idx(tok) for tok in ESM_MSA_ALLOWED_AMINO_ACIDS])
        self.toks = [self.model.alphabet.get_tok(idx) for idx in self.valid_aa_idx]
        self.draw_seed = None
        self.rng_stream = 0
        self.record = False
        self.last_run = []
        self.shard_over_ranks = False    # opt-in (or PGIBBS_SHARD_OVER_RANKS=1): generate() / generate_single_batch() split ONE job's MSAs over the torch.distributed ranks

    def untokenize_batch(self, batch):
        if hasattr(batch, "numpy") and getattr(batch, "ndim", 0) == 3:       # a [B, R, C] token tensor: one table lookup per row
            arr = batch.numpy()
            return self.model.alphabet.decode_rows(arr[:, :, 1:].reshape(-1, arr.shape[2] - 1))
        if hasattr(batch, "tolist"):
            batch = batch.tolist()
        out_batch = list()
        for msa in batch:
            out_batch += ["".join([self.model.alphabet.get_tok(itm) for itm in seq[1:]]) for seq in msa]
        return out_batch

    def get_init_msa(self, seed_msa, max_len, batch_size=1):
        """[B, R, C] tokens: every row <mask>-padded to max_len, the MSA repeated batch_size times (reference :78-90)."""
        rows = [(str(i), _gibbs.mask_padded(seq, max_len, ESM_MSA_ALLOWED_AMINO_ACIDS)) for i, seq in enumerate(seed_msa)]
        return self.model.batch_converter([rows] * batch_size)[2]

    def clean_seed_seq(self, seq):
        return _gibbs.clean_seed(seq, ESM_MSA_ALLOWED_AMINO_ACIDS)

    def _require_gpu(self, what):
        if not self.cuda:
            raise RuntimeError("ESM_MSA_sampler.%s needs device 'gpu'/'cuda:N' on an MI355X: the Gibbs hot path is "
                               "implemented as HIP kernels only, there is no CPU implementation" % what)

    # ---- single-row resampling (reference :101-147) -------------------------------------------
    def generate_single(self, seed_msa, steps=10, passes=3, burn_in=1, target_index=0, k=1, exclude_positions=None, top_p=None,
                        temperature_schedule=None, position_bias=None, allowed_residues=None, forbidden_residues=None):
        return self.generate_single_batch([seed_msa], steps=steps, passes=passes, burn_in=burn_in, target_index=target_index, k=k,
                                          exclude_positions=[exclude_positions], _shard=False, top_p=top_p,
                                          temperature_schedule=temperature_schedule, position_bias=position_bias,
                                          allowed_residues=allowed_residues, forbidden_residues=forbidden_residues)[0]

    def generate_single_batch(self, seed_msas, steps=10, passes=3, burn_in=1, target_index=0, k=1, exclude_positions=None,
                              max_batch=4, _shard=None, top_p=None, temperature_schedule=None, position_bias=None,
                              allowed_residues=None, forbidden_residues=None):
        """== [self.generate_single(m, steps, passes, burn_in, target_index, k, ex) for m, ex in zip(seed_msas, exclude_positions)]
        -- the loop of pgen_msa_revised over templates and sequences per template (reference pgen_msa_revised.py:107-115) --
        with MSAs of equal shape resampled together, up to `max_batch` per native call (BASELINE config 5: batches of templates),
        and, when sharding over torch.distributed ranks is switched on, contiguous blocks of the list on different GPUs.

        Same interpreter-RNG consumption as the serial calls (one random.shuffle per MSA and pass, MSA-major), one torch seed per
        MSA in list order, and the same strings: each MSA's arithmetic is independent of its batch mates (pgibbs.h
        pg_msa_gibbs_single_batch_run).  exclude_positions: None or one list (or None) per MSA.

        top_p, temperature_schedule, position_bias, allowed_residues, forbidden_residues (not in the reference; guides.DrawGuide):
        a guided draw of the sampled row, keyed by token column (residue 0 is column 1); the schedule is indexed by the step
        number (passes * steps of them) and top_p is ignored in burn-in passes, as k is."""
        guide = guides.from_arguments(top_p, temperature_schedule, position_bias, allowed_residues, forbidden_residues)
        n = len(seed_msas)
        if exclude_positions is None:
            exclude_positions = [None] * n
        if len(exclude_positions) != n:
            raise ValueError("exclude_positions: expected one list (or None) per MSA")
        self._require_gpu("generate_single")
        from . import pyrandom
        native = isinstance(self.model.model, NativeMaskedLM)
        ctx = _gibbs.shard_context(self, native, lambda: (seed_msas, steps, passes, burn_in, target_index, k, exclude_positions,
                                                          self.rng_stream, None if guide is None else guide.digest_parts()),
                                     "ESM_MSA_sampler.generate_single_batch", shard=_shard)

        # every MSA's step lists, decided up front in the serial order (selection never depends on the logits)
        jobs = []
        for seed_msa, excl in zip(seed_msas, exclude_positions):
            excl = set(i + 1 for i in (excl or []))                    # shift for the <cls> column
            sequence_length = len(seed_msa[0])
            positions = [x for x in range(1, sequence_length + 1) if x not in excl]
            batch = self.get_init_msa(seed_msa, len(seed_msa[0]), 1)
            R = batch.shape[1]
            if not -R <= target_index < R:
                raise IndexError("index %d is out of bounds for dimension 0 with size %d" % (target_index, R))
            steps_all, flags = [], []
            for pass_num in range(passes):
                pyrandom.global_shuffle(positions)
                for step in partition(positions, steps):
                    steps_all.append(list(step))
                    flags.append(1 if pass_num < burn_in else 0)
            jobs.append(dict(batch=batch, steps=steps_all, flags=flags, tr=target_index % R, seed=_gibbs.draw_seed(self)))
        if ctx is not None:
            seeds = sharding.broadcast_object(ctx, [j["seed"] for j in jobs])      # rank 0's torch draws
            for j, sd in zip(jobs, seeds):
                j["seed"] = sd
        self.last_run = [None] * n
        mask_idx = self.model.alphabet.mask_idx

        def table_of(job, P):
            return _gibbs.padded_positions(job["steps"], min_width=P)[0]

        lo, hi = (0, n) if ctx is None else sharding.shard_range(n, ctx.world, ctx.rank)
        if native:
            # equal-shape MSAs of this rank's block go through the engine together
            groups = {}
            for j in range(lo, hi):
                job = jobs[j]
                key = (tuple(job["batch"].shape), len(job["steps"]), tuple(job["flags"]), job["tr"])
                groups.setdefault(key, []).append(j)
            for key, members in groups.items():
                for sl, _ in _gibbs.chunks(len(members), max_batch):
                    chunk = members[sl]
                    P = max((len(st) for j in chunk for st in jobs[j]["steps"]), default=0)
                    table = np.stack([table_of(jobs[j], P) for j in chunk], axis=1)         # [n_steps, b, P]
                    tok = np.ascontiguousarray(np.concatenate([jobs[j]["batch"].numpy() for j in chunk]), dtype=np.int32)
                    R = tok.shape[1]
                    params = [_lib.make_sample_params(True, mask_idx, k, 0, None, self.valid_aa_idx, jobs[j]["seed"],
                                                      rng_stream=self.rng_stream, row_id_base=jobs[j]["tr"]) for j in chunk]
                    compiled = guides.compile_for(self, guide, tok.shape[2], table.shape[0])
                    with (self.model.model.draw_guide(compiled) if compiled is not None else contextlib.nullcontext()):
                        lg, st = self.model.model.gibbs_single_batch_run(tok, R - 1, key[3], table, list(key[2]), params,
                                                                         want_logits=self.record, want_tokens=self.record)
                    for i, j in enumerate(chunk):
                        jobs[j]["batch"] = torch.from_numpy(tok[i:i + 1].astype(np.int64))
                        if self.record:
                            self.last_run[j] = dict(table=table[:, i:i + 1], sampled_logits=lg[:, i], sampled_tokens=st[:, i],
                                                    tokens=tok[i:i + 1].copy())
        else:
            for job in jobs:
                R = job["batch"].shape[1]
                P = max((len(st) for st in job["steps"]), default=0)
                params = _lib.make_sample_params(True, mask_idx, k, 0, None, self.valid_aa_idx, job["seed"],
                                                 rng_stream=self.rng_stream, row_id_base=job["tr"])
                job["batch"] = _gibbs.run_plugin_loop(self.model.model, job["batch"], table_of(job, P)[:, None, :], params, self.device,
                                                      row_map=[job["tr"]], mask_row_map=[R - 1], sample_flags=job["flags"],
                                                      guide=guides.compile_for(self, guide, job["batch"].shape[2], len(job["steps"])))
        if ctx is not None:
            # the one collective: the resampled rows, padded to the widest alignment, blocks in rank order
            width = max(j["batch"].shape[2] for j in jobs)
            mine = np.full((hi - lo, width), -1, dtype=np.int32)
            for i, j in enumerate(range(lo, hi)):
                row = jobs[j]["batch"][0, jobs[j]["tr"]].numpy()
                mine[i, :len(row)] = row
            full = sharding.gather_blocks(ctx, mine, n, self.device)
            self.last_run = []                    # per-draw records are refused together with sharding (above)
            return ["".join(self.model.alphabet.get_tok(int(v)) for v in full[j, 1:jobs[j]["batch"].shape[2]]) for j in range(n)]
        if not self.record:
            self.last_run = []
        # == untokenize_batch(batch)[target_index] (reference :147) without spelling out the other rows of the alignment
        return [self.untokenize_batch(job["batch"][:, job["tr"]:job["tr"] + 1])[0] for job in jobs]

    # ---- whole-MSA resampling (reference :151-253) ------------------------------------------------
    def generate(self, n_samples, seed_msa, batch_size=1, in_order=False, max_len=None, leader_length=0,
                 leader_length_percent=None, top_k=0, temperature=None, num_iters=10, burnin=float('inf'),
                 mask=True, num_positions=0, num_positions_percent=None, indexes=None, rollover_from_start=False,
                 show_progress_bar=True, top_p=None, temperature_schedule=None, position_bias=None, allowed_residues=None,
                 forbidden_residues=None):
        """Arguments as pgen.esm_msa_sampler.ESM_MSA_sampler.generate, then the five of a guided draw, which the reference does not
        have (guides.DrawGuide; pg_draw v2): one table per token column (residue 0 is column 1), applied to every row of every MSA;
        temperature_schedule needs at least num_iters entries and replaces `temperature`."""
        guide = guides.from_arguments(top_p, temperature_schedule, position_bias, allowed_residues, forbidden_residues)
        num_sequences = len(seed_msa)
        sequence_length = len(seed_msa[0])
        sequences = []
        n_generation_rounds = math.ceil(n_samples / num_sequences / batch_size)
        num_positions, leader_length = _gibbs.derive_counts(sequence_length, num_positions, num_positions_percent,
                                                            leader_length, leader_length_percent)
        if max_len is None:
            max_len = sequence_length
        self._require_gpu("generate")
        draw_seed = _gibbs.draw_seed(self)
        self.last_run = []
        ctx = _gibbs.shard_context(self, isinstance(self.model.model, NativeMaskedLM), lambda: (
            n_samples, seed_msa, batch_size, in_order, max_len, leader_length, top_k, temperature, num_iters, burnin, mask,
            num_positions, None if indexes is None else list(indexes), rollover_from_start, self.rng_stream,
            None if guide is None else guide.digest_parts()), "ESM_MSA_sampler.generate")
        if ctx is not None:
            draw_seed = sharding.broadcast_object(ctx, draw_seed)

        for generation_round in trange(n_generation_rounds, disable=(not show_progress_bar)):
            batch = self.get_init_msa(seed_msa, max_len, batch_size)        # [B, R, C]
            indexes, last_i = self.calculate_indexes(indexes, leader_length, max_len, rollover_from_start)
            indexes = _gibbs.normalise_indexes(indexes, batch.shape[2])
            if num_positions > len(indexes):
                num_positions = len(indexes)
            table, last_i = _gibbs.build_target_table(num_iters, (batch_size, num_sequences), indexes, num_positions,
                                                      in_order, last_i)
            params = _lib.make_sample_params(mask, self.model.alphabet.mask_idx, top_k, burnin, temperature,
                                             self.valid_aa_idx, draw_seed, rng_stream=self.rng_stream,
                                             row_id_base=generation_round * batch_size * num_sequences)
            # a plug-in run is not recorded here (ESM_sampler.generate records it): the one difference between the two callers
            batch = _gibbs.run_gibbs_batch(self, ctx, batch, table, params, generation_round * batch_size * num_sequences, num_sequences,
                                           record_plugin=False, guide=guides.compile_for(self, guide, batch.shape[2], num_iters))
            strs = self.untokenize_batch(batch)
            if generation_round == (n_generation_rounds - 1):
                sequences += strs[0:n_samples - len(sequences)]
            else:
                sequences += strs
        return sequences

    # ---- index helpers with the reference's names (:255-304) ---------------------------------------
    def mask_target_indexes(self, batch, target_indexes):
        for batch_index in range(len(batch)):
            for sequence_index in range(len(batch[batch_index])):
                for kk in target_indexes[batch_index][sequence_index]:
                    batch[batch_index][sequence_index][kk] = self.model.alphabet.mask_idx

    def mask_target_indexes_single(self, batch, target_indexes, seq_index):
        for batch_index in range(len(batch)):
            for kk in target_indexes:
                batch[batch_index][seq_index][kk] = self.model.alphabet.mask_idx

    def get_target_indexes_all_positions(self, batch_size, indexes, num_sequences):
        return [[indexes] * num_sequences for _ in range(batch_size)]

    def get_random_target_index(self, batch_size, indexes, num_positions, num_sequences):
        from . import pyrandom
        t = pyrandom.global_sample_table(list(indexes), num_positions, batch_size * num_sequences)
        return t.reshape(batch_size, num_sequences, num_positions).tolist()

    def get_target_index_in_order(self, batch_size, indexes, next_i, num_positions, num_sequences):
        last_i, per_seq = _gibbs.in_order_window(indexes, next_i, num_positions)
        return last_i, [[per_seq] * num_sequences for _ in range(batch_size)]

    def calculate_indexes(self, indexes, leader_length, max_len, rollover_from_start):
        indexes, last_i = _gibbs.candidate_indexes(indexes, leader_length, max_len, rollover_from_start)
        return (list(indexes) if isinstance(indexes, range) else indexes), last_i     # the MSA sampler hands out a list (:296)

    # ---- masked log-likelihood of one MSA row (reference :306-432) --------------------------------------
    def log_likelihood(self, msa, target_index=0, with_masking=True, verbose=False, count_gaps=False,
                       mask_distance=float("inf")):
        return next(self.log_likelihood_batch([msa], target_index, with_masking, verbose, count_gaps, mask_distance))

    def log_likelihood_batch(self, msa_list, target_index=0, with_masking=True, verbose=False, count_gaps=False,
                             mask_distance=float("inf"), batch_size=1):
        """Same contract as pgen.esm_msa_sampler.ESM_MSA_sampler.log_likelihood_batch: yields (float mean, list[float])
        for the row `target_index` of every MSA; gap positions of the target row are skipped unless count_gaps.
        with_masking: every MSA is scored on its own strided-mask copies (no padding reaches the model, as in the reference,
        :365-405).  Unmasked: the reference converts the WHOLE list into one tensor padded to the deepest / widest MSA and scores
        `batch_size` of them per forward (:341, :416-431) -- so a shallower MSA of a ragged list is scored with <pad> rows and
        columns around it under fair-esm's padding semantics (and its tied row attention's 1/sqrt(R) from the padded depth); the
        same here, through the engine's <pad> handling."""
        self._require_gpu("log_likelihood_batch")
        for group in self._scoring_groups(msa_list, target_index, with_masking, count_gaps, mask_distance, batch_size):
            lps = [_gibbs.score_positions(self.model.model, tokens, row_of, idx, tgt, self.device)
                   for tokens, row_of, idx, tgt in group["calls"]]
            for item in group["items"]:
                likelihood_sum = np.float32(0.0)
                likelihood_list = []
                for call, sel, pos in item["rows"]:
                    for p_ in range(len(pos)):
                        likelihood_sum = np.float32(likelihood_sum + lps[call][sel, p_])
                        likelihood_list.append(float(lps[call][sel, p_]))
                if with_masking:
                    assert len(likelihood_list) == item["denom"]
                if item["denom"] == 0:                   # all-gap target row with count_gaps=False: the reference's 0.0 / 0
                    raise ZeroDivisionError("float division by zero")
                yield (float(likelihood_sum / np.float32(item["denom"])), likelihood_list)

    def _scoring_groups(self, msa_list, target_index, with_masking, count_gaps, mask_distance, batch_size):
        """What log_likelihood_batch and masked_marginals_batch run, as groups of forwards: `calls` = the (tokens, row_of, idx, tgt)
        of every forward of the group -- idx / tgt [n_sel, P]: scored token positions (-1 padded) and the original tokens there --
        and `items` = the MSAs those forwards score completely, each with `denom` (its scored positions) and `rows` = (call, selected
        row, token positions) in the order the reference appends them.  Unmasked: one group per `batch_size` MSAs of the padded
        list; masked: one group per MSA, its strided-mask copies in chunks of `batch_size`."""
        gap_tokens = {self.model.alphabet.get_idx(x) for x in ESM_MSA_GAP_CHARACTERS}
        if batch_size is None:
            batch_size = len(msa_list)
        range_start = 1 if self.model.alphabet.prepend_bos else 0
        mask_idx = self.model.alphabet.mask_idx
        if not with_masking:
            if not msa_list:
                return
            reformatted = [[(str(i), self.clean_seed_seq(seq)) for i, seq in enumerate(msa)] for msa in msa_list]
            _, _, tokens = self.model.batch_converter(reformatted)          # [n, R_max, C_max], <pad> around the smaller MSAs
            n, R, C = tokens.shape
            # the reference's own shape check (:353): the widest target row fills the padded width
            assert max(len(msa[target_index]) for msa in msa_list) == C - range_start
            # Row scored per MSA.  target_index >= 0: row target_index, as the reference.  target_index < 0 counts from the END OF
            # EACH MSA (as the masked path below and generate_single do).  On a list of equal depths that is the reference's
            # tokens[:, target_index]; on a ragged list the reference reads that row of the PADDED tensor -- a <pad> row for every
            # shallower MSA, whose "likelihoods" are those of <pad> tokens -- a deliberate deviation.
            rows_of = [target_index if target_index >= 0 else len(msa) + target_index for msa in msa_list]
            for sl, batch_start in _gibbs.chunks(n, batch_size):
                chunk = tokens[sl]
                nb = chunk.shape[0]
                pos_of, orig = [], []
                for i in range(nb):
                    msa = msa_list[batch_start + i]
                    o = chunk[i, rows_of[batch_start + i]].numpy()
                    end = len(msa[target_index]) + range_start
                    pos_of.append([p_ for p_ in range(range_start, end) if count_gaps or int(o[p_]) not in gap_tokens])
                    orig.append(o)
                idx, tgt = _gibbs.padded_positions(pos_of, orig, min_width=1)
                row_of = np.arange(nb) * R + np.asarray(rows_of[batch_start:batch_start + nb])
                items = []
                for i in range(nb):
                    msa = msa_list[batch_start + i]
                    denom = len(msa[target_index]) - (0 if count_gaps else sum(msa[target_index].count(g) for g in ESM_MSA_GAP_CHARACTERS))
                    items.append(dict(denom=denom, rows=[(0, i, pos_of[i])], start=range_start))
                yield dict(calls=[(chunk, row_of, idx, tgt)], items=items)
            return
        for msa in msa_list:
            reformatted = [(str(i), self.clean_seed_seq(seq)) for i, seq in enumerate(msa)]
            _, _, one = self.model.batch_converter(reformatted)            # [1, R, C]
            R = one.shape[1]
            tr = target_index % R
            seq_len = len(msa[target_index])
            assert seq_len == one.shape[2] - range_start              # the reference's shape check (:353-355)
            denom = seq_len - (0 if count_gaps else sum(msa[target_index].count(g) for g in ESM_MSA_GAP_CHARACTERS))
            end = seq_len + range_start
            orig = one[0, tr].numpy()
            copies, pos_all = _gibbs.strided_mask_copies(one, int(min(mask_distance, seq_len)), range_start, end, mask_idx, row=tr)
            pos_of = [[p for p in pos if count_gaps or int(orig[p]) not in gap_tokens] for pos in pos_all]
            idx, tgt = _gibbs.padded_positions(pos_of, [orig] * len(pos_of), min_width=1)
            calls, rows = [], []
            for sl, batch_start in _gibbs.chunks(len(pos_of), batch_size):
                nb = copies[sl].shape[0]
                row_of = np.arange(nb) * R + tr
                rows += [(len(calls), i, pos_of[batch_start + i]) for i in range(nb)]
                calls.append((copies[sl], row_of, idx[sl], tgt[sl]))
            yield dict(calls=calls, items=[dict(denom=denom, rows=rows, start=range_start)])

    # ---- contact prediction (fair-esm's MSATransformer.predict_contacts) ---------------------------------
    CONTACT_MAP_BYTES = 1 << 30      # default cap on one call's staged row-attention maps (B * n_heads * C * C fp32)

    def predict_contacts(self, msa):
        """Contact probabilities of one alignment's query sequence (row 0): float32 [L, L] -- see predict_contacts_batch."""
        return next(self.predict_contacts_batch([msa]))

    def predict_contacts_batch(self, msa_list, batch_size=None, max_map_bytes=None):
        """For every MSA (a list of aligned rows, as log_likelihood_batch takes them; row 0 is the query), in order, yields the
        contact probabilities float32 [L, L] over its L columns, from the tied row-attention maps.  MSAs of equal depth and width are
        run together, batch_size at a time (None: the whole group); an MSA is NEVER padded to another's shape -- <pad> rows and
        columns change the tied map and its 1/sqrt(R) --, so a contact map is each alignment's own.  A chunk is also cut so that the
        one block of maps the engine stages for it, B * n_heads * C * C * 4 bytes, stays under max_map_bytes (default
        CONTACT_MAP_BYTES = 1 GiB; one MSA always runs).  The result does not depend on batch_size or the cap."""
        self._require_gpu("predict_contacts_batch")
        lm = self.model.model
        if not isinstance(lm, NativeMaskedLM):
            raise TypeError("predict_contacts_batch needs the HIP engine (NativeMaskedLM)")
        predict = getattr(self.model, "predict_row_contacts", None) or lm.predict_row_contacts      # the holder's refusals (models.py) first
        cap = self.CONTACT_MAP_BYTES if max_map_bytes is None else int(max_map_bytes)
        if cap < 1:
            raise ValueError("max_map_bytes must be positive, got %r" % (max_map_bytes,))
        rows = [[(str(r), self.clean_seed_seq(seq)) for r, seq in enumerate(msa)] for msa in msa_list]
        for i, msa in enumerate(rows):
            if not msa or len(msa[0][1]) < 1:
                raise ValueError("predict_contacts_batch: alignment %d is empty: it has no contact map" % i)
            if any(len(seq) != len(msa[0][1]) for _, seq in msa):
                raise ValueError("predict_contacts_batch: the rows of alignment %d are not equally long" % i)
        groups = {}
        for i, msa in enumerate(rows):
            groups.setdefault((len(msa), len(msa[0][1])), []).append(i)
        done = {}
        for i, msa in enumerate(rows):
            if i not in done:
                members = groups[len(msa), len(msa[0][1])]
                C = len(msa[0][1]) + 1
                size = max(1, cap // (lm.cfg["n_heads"] * C * C * 4))
                if batch_size is not None:
                    size = max(1, min(size, batch_size))
                _, _, tokens = self.model.batch_converter([rows[m] for m in members])      # [n, R, C]: one shape, no <pad>
                tokens = tokens.numpy()
                lm.set_job_items(len(members))      # every chunk is a shard of the group's job: its maps do not depend on the chunking
                try:
                    for sl, first in _gibbs.chunks(len(members), size):
                        maps = predict(tokens[sl])
                        for b in range(len(maps)):
                            done[members[first + b]] = maps[b].copy()
                finally:
                    lm.set_job_items(0)
            yield done.pop(i)

    # ---- masked-marginal substitution tables ------------------------------------------------------------
    def masked_marginals_batch(self, msa_list, target_index=0, with_masking=True, count_gaps=False, mask_distance=float("inf"),
                               batch_size=1, normalise="vocab"):
        """The twin of log_likelihood_batch that keeps the whole row: for the row `target_index` of every MSA yields
        (logp float32 [n, 21], entropy float32 [n] in nats, positions, toks) -- one table row per scored position, `positions`
        their 0-based residue indices in ascending order (gap positions of the target row are left out unless count_gaps), columns
        = self.toks (the 21 symbols of self.valid_aa_idx, in that order).  Same copies and the same forwards as
        log_likelihood_batch; normalise "vocab" (logp at a position's own symbol is bit for bit what log_likelihood_batch lists
        there) or "columns" (over the 21 symbols only)."""
        self._require_gpu("masked_marginals_batch")
        if normalise not in _lib.TABLE_NORMS:
            raise ValueError("normalise must be 'vocab' or 'columns', got %r" % (normalise,))
        for group in self._scoring_groups(msa_list, target_index, with_masking, count_gaps, mask_distance, batch_size):
            tabs = [_gibbs.score_table(self.model.model, tokens, row_of, idx, self.valid_aa_idx, self.device, normalise, want_entropy=True)
                    for tokens, row_of, idx, _ in group["calls"]]
            for item in group["items"]:
                where = sorted((p_, call, sel, j) for call, sel, pos in item["rows"] for j, p_ in enumerate(pos))
                logp = np.zeros((len(where), len(self.valid_aa_idx)), dtype=np.float32)
                entropy = np.zeros(len(where), dtype=np.float32)
                for k, (_, call, sel, j) in enumerate(where):
                    logp[k] = tabs[call][0][sel, j]
                    entropy[k] = tabs[call][1][sel, j]
                yield logp, entropy, [w[0] - item["start"] for w in where], list(self.toks)

    def _probs_single_bins(self, sequence_length, steps):
        """The mask bins of probs_single: the target row's token positions 1 .. L shuffled with random.shuffle on the interpreter's
        global RNG (CPython-exact, consuming it as generate_single's one pass does) and split by `partition`; None = one per position."""
        from . import pyrandom
        positions = list(range(1, sequence_length + 1))
        pyrandom.global_shuffle(positions)
        return partition(positions, sequence_length if steps is None else steps)

    def probs_single(self, msa, steps=None, target_index=-1, show_progress_bar=True, batch_size=None):
        """The call the reference's pgen_msa_seq_probs.py:31 makes (its ESM_MSA_sampler no longer has the method): the probability
        of every symbol at every position of row `target_index`, by masking.  The row's positions are shuffled and split into
        `steps` bins (None: one bin per position) as generate_single does; for each bin the row is masked at the bin's positions,
        the model runs, and the distribution generate_step would draw from there (softmax over the 21 valid symbols, no
        temperature, no top-k) is read at those positions.  Bins never see each other's results, so all bins of a call are ONE
        batched job of `steps` alignments, run `batch_size` at a time (None: all at once; the result does not depend on it).
        Returns (probs float32 [len(toks), L], toks)."""
        self._require_gpu("probs_single")
        sequence_length = len(msa[0])
        reformatted = [(str(i), self.clean_seed_seq(seq)) for i, seq in enumerate(msa)]
        _, _, one = self.model.batch_converter(reformatted)               # [1, R, C]
        R = one.shape[1]
        if not -R <= target_index < R:
            raise IndexError("index %d is out of bounds for dimension 0 with size %d" % (target_index, R))
        bins = self._probs_single_bins(sequence_length, steps)
        tr = target_index % R
        n = len(bins)
        copies = _gibbs.masked_copies(one, bins, self.model.alphabet.mask_idx, row=tr)
        idx, _ = _gibbs.padded_positions(bins)
        probs = np.zeros((len(self.toks), sequence_length), dtype=np.float32)
        native = isinstance(self.model.model, NativeMaskedLM)
        if native:
            # every chunk is a shard of the one n-alignment job: kernel choices that change a summation order are taken on the
            # job's size, so the table does not depend on batch_size (pgibbs.h pg_engine_set_job_items)
            self.model.model.set_job_items(n)
        try:
            for sl, b0 in tqdm(list(_gibbs.chunks(n, n if batch_size is None else batch_size)), disable=(not show_progress_bar)):
                nb = copies[sl].shape[0]
                tab, _ = _gibbs.score_table(self.model.model, copies[sl], np.arange(nb) * R + tr, idx[sl], self.valid_aa_idx,
                                            self.device, "columns")
                for i in range(nb):
                    b = np.asarray(bins[b0 + i], dtype=np.int64)
                    probs[:, b - 1] = np.exp(tab[i, :len(b)]).T
        finally:
            if native:
                self.model.model.set_job_items(0)
        return probs, list(self.toks)
