"""Host-side pieces shared by ESM_sampler and ESM_MSA_sampler: target-position tables, masked copies, the
one-batch runner of generate() and the device loop and scoring calls for plug-in (non-engine) models.
Everything that touches tokens or logits per position is a HIP kernel behind the C ABI; this file only
prepares index tables and sequences the calls.
"""
import contextlib
import ctypes
import re

import numpy as np
import torch

from . import _lib, sharding
from . import pyrandom as _pyr
from .engine import NativeMaskedLM

SHADOW_BIT = 1 << 30   # include/pgibbs.h: sampled but not written (a later duplicate in the same row wins)


def resolve_device(device):
    """The reference's device grammar (esm_sampler.py:66-78, esm_msa_sampler.py:47-61): "cpu" | "gpu" | "cuda:N", with
    its three error messages.  Returns (device string, uses_gpu)."""
    if device == "gpu":
        device = "cuda:0"
    if re.match("^cuda:[0-9]+$", device):
        if not torch.cuda.is_available():
            raise Exception("gpu requested, but No Cuda devices found")
        if int(device.split(":")[1]) >= torch.cuda.device_count():
            raise Exception("Invalid cuda device number: " + device)
        return device, True
    if device != "cpu":
        raise Exception("Invalid device: " + device)
    return device, False


def clean_seed(seq, allowed):
    """clean_seed_seq of both samplers (esm_sampler.py:95-102, esm_msa_sampler.py:93-99)."""
    seq = seq.upper()
    bad = set(seq) - set(allowed)
    if bad:
        raise Exception("Invalid input character: " + ",".join(bad))
    return seq


def mask_padded(seq, max_len, allowed):
    """A cleaned seed right-padded with the literal "<mask>" up to max_len residues (esm_sampler.py:115,120)."""
    return clean_seed(seq, allowed) + "<mask>" * (max_len - len(seq))


def candidate_indexes(indexes, leader_length, max_len, rollover_from_start):
    """calculate_indexes (esm_sampler.py:264-274, esm_msa_sampler.py:294-304): 1-based token positions after the leader
    (position 0 is <cls>), or the caller's `indexes` untouched; last_i = where an in-order sweep starts."""
    if indexes is not None:
        return indexes, -1
    indexes = range(1, max_len + 1)
    if rollover_from_start:
        return indexes, -1
    return indexes[leader_length:], leader_length - 1


def derive_counts(length, num_positions, num_positions_percent, leader_length, leader_length_percent):
    """num_positions / leader_length from their *_percent forms, clamped at 0 (esm_sampler.py:189-197)."""
    if num_positions_percent is not None:
        num_positions = int(length * (num_positions_percent / 100))
    if leader_length_percent is not None:
        leader_length = int(length * (leader_length_percent / 100))
    return max(num_positions, 0), max(leader_length, 0)


def in_order_window(indexes, next_i, num_positions):
    """get_target_index_in_order (/root/reference/src/pgen/esm_sampler.py:248-257)."""
    out = []
    n = len(indexes)
    for _ in range(num_positions):
        next_i = (next_i + 1) % n
        out.append(indexes[next_i])
    return next_i, out


def normalise_indexes(indexes, width):
    """Candidate positions as the reference's `batch[b][kk]` would resolve them (esm_sampler.py:234,262): a torch row of
    `width` tokens accepts -width <= kk < width, negative values counting from the end; anything else is the IndexError
    torch raises there.  `range` objects (the default candidates) are returned untouched."""
    if isinstance(indexes, range):
        if len(indexes) and (indexes[0] < -width or indexes[-1] >= width or indexes[0] < 0):
            indexes = list(indexes)
        else:
            return indexes
    out = []
    for kk in indexes:
        k = int(kk)
        if k < -width or k >= width:
            raise IndexError("index %d is out of bounds for dimension 0 with size %d" % (k, width))
        out.append(k + width if k < 0 else k)
    return out


def mark_shadowed(table, indexes):
    """Sequential write-back semantics for duplicate positions inside one row's target list."""
    if len(set(indexes)) == len(indexes):
        return table
    flat = table.reshape(-1, table.shape[-1])
    for row in flat:
        seen = set()
        for p in range(len(row) - 1, -1, -1):
            v = int(row[p])
            if v < 0:
                continue
            if v in seen:
                row[p] = v | SHADOW_BIT
            seen.add(v)
    return table


def build_target_table(n_iters, n_rows_shape, indexes, num_positions, in_order, last_i):
    """All target positions of one batch, for every iteration, as int32 [n_iters, *n_rows_shape, P].

    Mirrors the per-iteration branch of generate() (esm_sampler.py:210-218, esm_msa_sampler.py:222-231):
    random -> one random.sample per row in row-major order, iteration-major (exactly the order the
    reference consumes the interpreter's RNG); in order -> one shared cyclic window per iteration;
    num_positions == 0 -> every candidate position every iteration.
    Returns (table, last_i).
    """
    indexes = list(indexes)
    n_rows = int(np.prod(n_rows_shape)) if len(n_rows_shape) else 1
    if num_positions > 0:
        P = num_positions
        if in_order:
            table = np.empty((n_iters, n_rows, P), dtype=np.int32)
            for it in range(n_iters):
                last_i, win = in_order_window(indexes, last_i, P)
                table[it, :, :] = np.asarray(win, dtype=np.int32)[None, :]
        else:
            table = _pyr.global_sample_table(indexes, P, n_iters * n_rows).reshape(n_iters, n_rows, P)
    else:
        P = len(indexes)
        table = np.broadcast_to(np.asarray(indexes, dtype=np.int32), (n_iters, n_rows, P)).copy()
    table = mark_shadowed(table, indexes)
    return table.reshape((n_iters,) + tuple(n_rows_shape) + (P,)), last_i


def padded_positions(pos_of, tokens_at=None, min_width=0):
    """A ragged list of position lists as one table: idx int32 [n, P], -1 padded, P = the longest list (at least min_width),
    and -- when tokens_at gives the token row each list points into -- tgt int32 [n, P], the tokens found there (else None)."""
    P = max(max((len(pos) for pos in pos_of), default=0), min_width)
    idx = np.full((len(pos_of), P), -1, dtype=np.int32)
    tgt = None if tokens_at is None else np.zeros((len(pos_of), P), dtype=np.int32)
    for i, pos in enumerate(pos_of):
        idx[i, :len(pos)] = pos
        if tgt is not None:
            tgt[i, :len(pos)] = tokens_at[i][pos]
    return idx, tgt


def masked_copies(one, bins, mask_idx, row=None):
    """len(bins) copies of the token tensor `one` ([1, T], or [1, R, C] with `row` the alignment row that is masked), copy i
    masked at the positions bins[i]."""
    copies = one.repeat(len(bins), *([1] * (one.dim() - 1)))
    for i, pos in enumerate(bins):
        if row is None:
            copies[i, pos] = mask_idx
        else:
            copies[i, row, pos] = mask_idx
    return copies


def strided_mask_copies(one, n, start, end, mask_idx, row=None):
    """The masked-likelihood copies of both samplers (esm_sampler.py:300-317): n copies, copy i masked at start + i,
    start + i + n, ... below `end`.  Returns (copies, pos_all) with pos_all[i] the positions masked in copy i."""
    pos_all = [list(range(start + i, end, n)) for i in range(n)]
    return masked_copies(one, pos_all, mask_idx, row), pos_all


def chunks(n, batch_size):
    """(slice, first index) of every run of max(1, batch_size) items out of n."""
    step = max(1, batch_size)
    for b0 in range(0, n, step):
        yield slice(b0, b0 + step), b0


def draw_seed(sampler):
    """Key of the token-draw generator: the sampler's pinned `draw_seed`, else one draw from torch's global RNG."""
    return sampler.draw_seed if sampler.draw_seed is not None else int(torch.randint(0, 2**62, (1,)).item())


def shard_context(sampler, native, digest_parts, what, shard=None):
    """The prologue of a job that may be split over torch.distributed ranks: a DistContext when the model is the
    engine, sharding is switched on (`shard`, default: the sampler's opt-in) and there are several ranks, else None.  With a
    context: record=True is refused, every rank must have been handed the same job (digest_parts() -> the arguments that
    define it, evaluated only here) and all ranks continue from rank 0's interpreter RNG state."""
    if shard is None:
        shard = sharding.sharding_requested(sampler.shard_over_ranks)
    ctx = sharding.dist_context() if (native and shard) else None
    if ctx is not None:
        if sampler.record:
            raise ValueError("record=True is not supported together with shard_over_ranks (per-draw logits stay on their rank)")
        sharding.check_same_job(ctx, sharding.job_digest(*digest_parts()), what)
        sharding.sync_host_rng(ctx)
    return ctx


def _dptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _current_stream_ptr(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def run_plugin_loop(model_callable, tokens_i64, table, params, device, row_map=None, mask_row_map=None,
                    sample_flags=None, guide=None):
    """Gibbs loop for a plug-in model whose forward is not the HIP engine (any callable
    tokens[int64, device] -> {"logits": float tensor}): mask scatter and draw/write-back are the HIP kernels
    `pg_mask_scatter_device` / `pg_sample_writeback_device`; the token buffer stays on the device.

    tokens_i64: torch int64 tensor [..rows.., width] (any device); table int32 [n_iters, n_sel, P];
    row_map: optional int32 [n_sel] token-row sampled for each selected row (generate_single);
    mask_row_map: token-row masked for each selected row (defaults to row_map; generate_single masks row -1);
    sample_flags: optional per-iteration override of `sample` (generate_single's pass_num < burn_in);
    guide: optional guides.CompiledGuide -- the draw is then `pg_sample_writeback_guided_device` (pg_draw v2) on device copies
    of its tables, iteration `it` reading temperature `it` of a schedule.
    Returns the final tokens as a torch int64 CPU tensor of the input shape.
    """
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X visible: the Gibbs hot path has no CPU implementation in this package")
    L = _lib.lib()
    dev = torch.device(device)
    shape = tuple(tokens_i64.shape)
    width = shape[-1]
    n_rows = int(np.prod(shape[:-1]))
    tok = tokens_i64.to(device=dev, dtype=torch.int32).contiguous()
    n_iters, n_sel, P = table.shape
    d_table = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
    d_rowmap = torch.from_numpy(np.ascontiguousarray(row_map, dtype=np.int32)).to(dev) if row_map is not None else None
    rm_ptr = _dptr(d_rowmap) if d_rowmap is not None else None
    d_mrowmap = (torch.from_numpy(np.ascontiguousarray(mask_row_map, dtype=np.int32)).to(dev)
                 if mask_row_map is not None else None)
    mrm_ptr = _dptr(d_mrowmap) if d_mrowmap is not None else rm_ptr
    if guide is not None and guide.empty:
        guide = None
    if guide is not None:
        if guide.temperatures is not None and len(guide.temperatures) < n_iters:
            raise ValueError("temperature_schedule has %d entries, the call runs %d iterations" % (len(guide.temperatures), n_iters))
        d_bias = torch.from_numpy(guide.bias).to(dev) if guide.bias is not None else None
        d_temps = torch.from_numpy(guide.temperatures).to(dev) if guide.temperatures is not None else None
        guide_args = (_dptr(d_bias) if d_bias is not None else None, 0 if d_bias is None else d_bias.shape[0],
                      _dptr(d_temps) if d_temps is not None else None, 0 if d_temps is None else d_temps.shape[0],
                      float("nan") if guide.top_p is None else guide.top_p)
    with torch.cuda.device(dev):
        for it in range(n_iters):
            stream = _current_stream_ptr(dev)
            idx_ptr = _dptr(d_table[it])
            if params.mask and P > 0:
                _lib.check(L.pg_mask_scatter_device(stream, _dptr(tok), n_rows, width, idx_ptr, mrm_ptr, n_sel, P, params.mask_idx))
            out = model_callable(tok.to(torch.int64).reshape(shape))["logits"]
            if P == 0:
                continue
            out = out.to(device=dev, dtype=torch.float32).contiguous()
            V = out.shape[-1]
            if sample_flags is not None:
                params.burnin = _lib.INT32_MAX if sample_flags[it] else 0
            if guide is not None:
                _lib.check(L.pg_sample_writeback_guided_device(stream, _dptr(tok), n_rows, width, _dptr(out), V, idx_ptr, rm_ptr, n_sel,
                                                               P, ctypes.byref(params), it, None, *guide_args))
            else:
                _lib.check(L.pg_sample_writeback_device(stream, _dptr(tok), n_rows, width, _dptr(out), V, idx_ptr, rm_ptr, n_sel, P,
                                                        ctypes.byref(params), it, None))
        torch.cuda.synchronize(dev)
    return tok.to(device="cpu", dtype=torch.int64).reshape(shape)


def run_gibbs_batch(sampler, ctx, batch, table, params, row_id_base, rows_per_item, record_plugin=False, guide=None):
    """One batch of either generate(): `batch` (torch int64 [B, T] or [B, R, C]) through every iteration of `table`
    (int32 [iters, B, P] / [iters, B, R, P]); returns the final tokens as a torch int64 tensor of the same shape.
    Engine models: one native call -- or, with a DistContext `ctx`, this rank's block of the batch (announced to the engine as
    a shard of a B-item job) and one gather; row_id_base / rows_per_item are the Philox row id of the batch's first row and
    the ids one item consumes.  Plug-in models: the device loop over the table flattened to [iters, rows, P].
    sampler.record appends the run to sampler.last_run; a plug-in run only when the caller asks for it (record_plugin).
    guide (guides.CompiledGuide or None): the draws are pg_draw v2 under it -- set on the engine around the native call and cleared
    after it whatever happens, or handed to the plug-in loop."""
    lm = sampler.model.model
    if not isinstance(lm, NativeMaskedLM):
        flat = table.reshape(table.shape[0], int(np.prod(table.shape[1:-1])), table.shape[-1]) if table.ndim > 3 else table
        batch = run_plugin_loop(lm, batch, flat, params, sampler.device, guide=guide)
        if sampler.record and record_plugin:
            sampler.last_run.append(dict(table=table, tokens=batch.numpy().copy()))
        return batch
    tok = np.ascontiguousarray(batch.numpy(), dtype=np.int32)
    with (lm.draw_guide(guide) if guide is not None else contextlib.nullcontext()):      # unguided: the engine object is not touched
        if ctx is not None:
            def run_block(ltok, ltable, base):
                params.row_id_base = base & 0xFFFFFFFF
                lm.set_job_items(batch.shape[0])      # shard of a batch.shape[0]-item job
                try:
                    lm.gibbs_run(ltok, ltable, params)
                finally:
                    lm.set_job_items(0)
            tok = sharding.run_sharded(ctx, tok, table, row_id_base, rows_per_item, run_block, sampler.device, guard=lm)
        else:
            lg, st = lm.gibbs_run(tok, table, params, want_logits=sampler.record, want_tokens=sampler.record)
            if sampler.record:
                sampler.last_run.append(dict(table=table, sampled_logits=lg, sampled_tokens=st, tokens=tok.copy()))
    return torch.from_numpy(tok.astype(np.int64))


@contextlib.contextmanager
def _plugin_logits(model_callable, tokens_i64, device, no_gpu, *arrays):
    """The plug-in side of score_positions / score_table: the caller's forward on `device`, its logits as one contiguous fp32
    tensor, and device copies of the int32 `arrays`.  Yields (stream, logits, (n_rows, width, V), device copies) for the
    caller's one kernel launch and synchronizes after it.  Without a GPU: RuntimeError(no_gpu)."""
    if not torch.cuda.is_available():
        raise RuntimeError(no_gpu)
    dev = torch.device(device)
    with torch.cuda.device(dev):
        out = model_callable(tokens_i64.to(dev))["logits"].to(device=dev, dtype=torch.float32).contiguous()
        width, V = out.shape[-2], out.shape[-1]
        yield _current_stream_ptr(dev), out, (out.numel() // (width * V), width, V), [torch.from_numpy(a).to(dev) for a in arrays]
        torch.cuda.synchronize(dev)


def _int32(*arrays):
    return [np.ascontiguousarray(a, dtype=np.int32) for a in arrays]


def _host_tokens(tokens):
    return tokens.numpy() if hasattr(tokens, "numpy") else tokens


def score_positions(model_callable, tokens_i64, row_of, idx, targets, device):
    """log_softmax(logits)[target] at (token row row_of[s], position idx[s][p]); idx < 0 -> 0.
    Engine models: one native call (LM head only at the scored rows).  Plug-in models: the caller's forward, then the
    HIP gather kernel `pg_logprob_gather_device` on its device-resident logits."""
    row_of, idx, targets = _int32(row_of, idx, targets)
    if isinstance(model_callable, NativeMaskedLM):
        return model_callable.forward_logprobs(_host_tokens(tokens_i64), row_of, idx, targets)
    no_gpu = "no MI355X visible: log-likelihood scoring has no CPU implementation in this package"
    with _plugin_logits(model_callable, tokens_i64, device, no_gpu, idx, row_of, targets) as (stream, out, dims, (d_idx, d_row, d_tgt)):
        res = torch.zeros(idx.shape, dtype=torch.float32, device=out.device)
        _lib.check(_lib.lib().pg_logprob_gather_device(stream, _dptr(out), *dims, _dptr(d_idx), _dptr(d_row), _dptr(d_tgt),
                                                       idx.shape[0], idx.shape[1], _dptr(res)))
    return res.cpu().numpy()


def score_table(model_callable, tokens_i64, row_of, idx, cols, device, normalise="vocab", want_entropy=False):
    """The table form of score_positions: out[s, p, c] = log-probability of token cols[c] at (token row row_of[s], position
    idx[s][p]), normalised over the vocabulary ("vocab") or over the selected columns ("columns"); idx < 0 -> zeros.  Returns
    (out float32 [n_sel, P, n_cols], entropy float32 [n_sel, P] or None).
    Engine models: one native call.  Plug-in models: the caller's forward, then the HIP table kernel `pg_logprob_table_device` on
    its device-resident logits."""
    if normalise not in _lib.TABLE_NORMS:
        raise ValueError("normalise must be 'vocab' or 'columns', got %r" % (normalise,))
    row_of, idx, cols = _int32(row_of, idx, cols)
    cols = cols.reshape(-1)
    if isinstance(model_callable, NativeMaskedLM):
        return model_callable.forward_logprob_table(_host_tokens(tokens_i64), row_of, idx, cols, normalise, want_entropy)
    no_gpu = "no MI355X visible: masked-marginal tables have no CPU implementation in this package"
    with _plugin_logits(model_callable, tokens_i64, device, no_gpu, idx, row_of, cols) as (stream, out, dims, (d_idx, d_row, d_cols)):
        if len(cols) and (cols.min() < 0 or cols.max() >= dims[2]):
            raise ValueError("score_table: a column lies outside the model's vocabulary of %d" % dims[2])
        res = torch.zeros(idx.shape + (len(cols),), dtype=torch.float32, device=out.device)
        ent = torch.zeros(idx.shape, dtype=torch.float32, device=out.device) if want_entropy else None
        _lib.check(_lib.lib().pg_logprob_table_device(stream, _dptr(out), *dims, _dptr(d_idx), _dptr(d_row), idx.shape[0], idx.shape[1],
                                                      _dptr(d_cols), len(cols), _lib.TABLE_NORMS[normalise], _dptr(res),
                                                      _dptr(ent) if want_entropy else None))
    return res.cpu().numpy(), (ent.cpu().numpy() if want_entropy else None)
