"""What the ESM-2 GPU suites (test_gpu_esm2.py and its _150m, _3b, _15b, _8m siblings) share: token batches, the 16-bit roundings,
the wrapper call, the oracle's replay of every draw, the single-chain job, the sharded job and the child processes that rerun one
of them under another environment.  A child imports the CALLING test module by name and calls a function of it, so every suite
keeps its own model and its own `_single_chain_child` / `_shard_child` / `_refuse_valu_child` entry."""
import ctypes
import hashlib
import json
import os
import random
import subprocess
import sys
import warnings

import numpy as np

from oracle import draw as odraw
from protein_gibbs_sampler_amd import _lib, esm_sampler

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SEED25 = "MEPAATGQEAEECAHSGRGEAWEEV"
PREC = {"fp32": _lib.PG_PREC_FP32, "bf16": _lib.PG_PREC_BF16, "fp16": _lib.PG_PREC_F16}


def tokens(rng, B, T, mask_every=7):
    tok = np.concatenate([np.zeros((B, 1), np.int64), rng.integers(4, 24, (B, T - 2)), np.full((B, 1), 2)], axis=1) if T >= 2 \
        else np.zeros((B, 1), np.int64)
    tok[:, 2:T - 1:mask_every] = 32
    return tok


def round_bf16(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + (((u >> 16) & 1) + np.uint32(0x7fff))) & np.uint32(0xffff0000)).view(np.float32)


def round_f16(x):
    return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


def model(cls, cfg, sd, precision):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return cls(state_dict=sd, config=cfg, precision=precision)


def replay_draws(s, run, B, P, iters, top_k, burnin, temperature, draw_seed):
    for it in range(iters):
        rows = run["sampled_logits"][it].reshape(-1, 33)
        assert np.isfinite(rows).all()
        toks = odraw.draw_rows(rows, s.valid_aa_idx, top_k, it < burnin, temperature, np.repeat(np.arange(B), P), it,
                               np.tile(np.arange(P), B), 0, draw_seed)
        assert (toks == run["sampled_tokens"][it].reshape(-1)).all(), "draw differs from the oracle"


def child(module_name, call, timeout=300, **env):
    """`module_name`.`call`() in a fresh process under `env` (the switches are read once per process) -> its output lines"""
    code = "import sys; sys.path[:0] = [%r, %r]; import %s as t; t.%s()" % (ROOT, HERE, module_name, call)
    proc = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert proc.returncode == 0, proc.stderr[-2000:]
    return proc.stdout.splitlines()


# ---- one chain: the hipGraph path ---------------------------------------------------------------------------------------------------
def single_chain_generate(s, record):
    s.draw_seed, s.record = 21, record
    random.seed(4)
    return s.generate(1, SEED25, batch_size=1, num_iters=12, num_positions=3, top_k=0, temperature=1.0, burnin=float("inf"), show_progress_bar=False)


def single_chain_run(wrapped):
    """One chain of 25 residues (27 token rows: weight-streaming GEMMs), 12 iterations, not recorded: the hipGraph path when on."""
    s = esm_sampler.ESM_sampler(wrapped, device="cuda:0")
    return s, single_chain_generate(s, False)


def single_chain_child(run):
    _, out = run()
    print("CHILD_TOKENS " + json.dumps(out))


def check_single_chain(run, module_name, timeout=300):
    """the graph was captured and replayed; the same job in a fresh child process with graphs off (PGIBBS_GRAPH is read once per
    process) gives the same sequence; and recorded (eager loop, logits emitted): same sequence, every draw replayed by the oracle"""
    s, out = run()
    lm = s.model.model
    assert lm.get_stat("graph_captures") == 1 and lm.get_stat("graph_replays") > 0
    line = [l for l in child(module_name, "_single_chain_child", timeout=timeout, PGIBBS_GRAPH="0") if l.startswith("CHILD_TOKENS ")][-1]
    assert json.loads(line[len("CHILD_TOKENS "):]) == out
    again = single_chain_generate(s, True)
    assert again == out
    replay_draws(s, s.last_run[0], 1, 3, 12, 0, float("inf"), 1.0, 21)


# ---- a job and its shards -----------------------------------------------------------------------------------------------------------
def shard_tokens(B, L, seed=1234):
    rng = np.random.default_rng(seed)
    return np.concatenate([np.zeros((B, 1), np.int64), rng.integers(4, 24, (B, L)), np.full((B, 1), 2)], axis=1).astype(np.int32)


def shard_runner(s, tok_all, P, iters):
    """-> run(lo, hi): chains lo .. hi - 1 of the job `tok_all` as a shard that knows the job's size (pg_engine_set_job_items), on
    the device: (tokens after the run, logits of every draw)"""
    import torch

    from protein_gibbs_sampler_amd import pyrandom, sharding
    lm = s.model.model
    B, T = tok_all.shape
    L = T - 2
    L_ = _lib.lib()

    def run(lo, hi):
        r = pyrandom.NativePyRandom()
        r.seed(0)
        table = sharding.local_slice(sharding.global_position_table(r, list(range(1, L + 1)), P, iters, B), lo, hi)
        params = _lib.make_sample_params(True, 32, 0, float("inf"), 1.0, s.valid_aa_idx, rng_seed=0, row_id_base=lo)
        d_tok = torch.from_numpy(tok_all[lo:hi].copy()).cuda()
        d_idx = torch.from_numpy(table).cuda()
        d_lg = torch.empty((iters, hi - lo, P, 33), dtype=torch.float32, device="cuda")
        lm.set_job_items(B)
        try:
            _lib.check(L_.pg_esm_gibbs_run_device(lm.handle, ctypes.c_void_p(d_tok.data_ptr()), hi - lo, T,
                                                  ctypes.c_void_p(d_idx.data_ptr()), iters, P, ctypes.byref(params),
                                                  ctypes.c_void_p(d_lg.data_ptr()), None))
            lm.synchronize()
        finally:
            lm.set_job_items(0)
        return d_tok.cpu().numpy(), d_lg.cpu().numpy()

    return run


def shard_job(wrapped, worlds, B=64):
    """A B-chain job of config 2's chain length, whole and as contiguous shards that know the job's size: a digest of (tokens,
    logits) of the whole job, after checking every world against it bit for bit."""
    from protein_gibbs_sampler_amd import sharding
    s = esm_sampler.ESM_sampler(wrapped, device="cuda:0")
    tok_all = shard_tokens(B, 256)
    run = shard_runner(s, tok_all, 5, 2)
    whole, whole_lg = run(0, B)
    assert (whole != tok_all).any() and np.isfinite(whole_lg).all()
    for world in worlds:
        parts = [run(*sharding.shard_range(B, world, g)) for g in range(world)]
        assert (np.concatenate([p[1] for p in parts], axis=1) == whole_lg).all(), "world=%d: sampled-position logits differ" % world
        assert (np.concatenate([p[0] for p in parts]) == whole).all(), "world=%d" % world
    return hashlib.sha256(whole.tobytes() + whole_lg.tobytes()).hexdigest()


def refuse_valu_child(hd):
    """the strict attention entry at heads of `hd` under PGIBBS_ATTN_F32=valu: prints the refusal"""
    x = np.zeros((1, 16, 3 * 2 * hd), np.float32)
    y = np.zeros((1, 16, 2 * hd), np.float32)
    rc = _lib.lib().pg_dbg_attention_hd(0, _lib.PG_PREC_FP32, _lib.ptr(x), _lib.ptr(y), 1, 16, 2, hd, None, -1)
    assert rc != 0
    try:
        _lib.check(rc)
    except Exception as e:      # noqa: BLE001
        print("CHILD_REFUSED " + str(e))
