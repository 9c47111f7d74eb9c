"""What the ESM-2 GPU suites share.  First the tools every size's own file (test_gpu_esm2.py and its _150m, _3b, _15b, _8m, _35m siblings)
uses: token batches, the 16-bit roundings, the wrapper call, the oracle's replay of every draw, the job of a shard, a child process.
Then the test bodies that are the same at every size, each taking a --model name whose row of tests/_esm2_sizes.py holds what differs:
tests/test_gpu_esm2_sizes.py parametrises over that table the ones that are one item per size, and each size's own file runs the ones
with many cases (its T, H, precision and shape lists are its decorators).  A child process (the switches are read once per process) imports
this module and calls `_single_chain_child` / `_shard_child` with the name."""
import ctypes
import hashlib
import json
import os
import random
import subprocess
import sys
import warnings

import numpy as np
import pytest

import _esm2_reference as ref
from _esm2_sizes import FWD_BATCHES, HF_FIXTURES, SIZES
from oracle import draw as odraw
from protein_gibbs_sampler_amd import _lib, esm_sampler, models, weights

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


def child(module_name, call, *args, timeout=300, **env):
    """`module_name`.`call`(*args) in a fresh process under `env` (the switches are read once per process) -> its output lines"""
    code = "import sys; sys.path[:0] = [%r, %r]; import %s as t; t.%s(*%r)" % (ROOT, HERE, module_name, call, args)
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
    """A B-chain job of config 2's chain length, whole and as contiguous shards that know the job's size (pg_engine_set_job_items): a
    digest of (tokens, logits) of the whole job, after checking every world against it bit for bit."""
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


# ==== the bodies that run at every size ================================================================================================
_CASES = {}


def case(size, n_layers=None, d=None, seed=7, **over):
    """-> (configuration, synthetic weights, reference configuration) of a cut of `size`: the row's default case unless said otherwise,
    d_ffn = 4 d unless said otherwise.  One case per size stays cached, so that consecutive tests on the same model (3B: 236 M weights)
    draw its weights once."""
    row = SIZES[size]
    n_layers, d = n_layers or row["case"]["n_layers"], d or row["case"]["d"]
    over.setdefault("d_ffn", 4 * d)
    key = json.dumps([n_layers, d, seed, over], sort_keys=True)
    if _CASES.get(size, (None,))[0] != key:
        cfg = weights.make_config(row["base"], n_layers=n_layers, d_model=d, **over)
        assert cfg["n_heads"] * row["hd"] == d
        sd = weights.synthetic_state_dict(cfg, seed=seed, std=row["case"]["std"], embed_std=row["case"]["embed_std"], ln_jitter=0.1)
        _CASES[size] = (key, (cfg, sd, ref.Esm2Config.of(cfg)))
    return _CASES[size][1]


def size_model(size, cfg, sd, precision):
    return model(SIZES[size]["wrapper"], cfg, sd, precision)


# ---- the attention and rotation kernels of a width -------------------------------------------------------------------------------------
def check_attention_hd(size, T, H, precision):
    """Each shape without and with <pad> keys (the PADMASK forms); row 1's tail is padding."""
    hd, q_draw = SIZES[size]["hd"], SIZES[size]["attention"]["q_draw"]
    B = 2
    rng = np.random.default_rng(T * 7 + H)
    qkv = rng.standard_normal((B, T, 3, H, hd)).astype(np.float32)
    qkv[:, :, 0] *= np.float32(q_draw)
    rnd = {"fp32": lambda a: a, "bf16": round_bf16, "fp16": round_f16}[precision]
    x = np.ascontiguousarray(rnd(qkv).reshape(B, T, 3 * H * hd))
    tok = np.full((B, T), 5, dtype=np.int32)
    tok[1, max(1, T - 1 - T // 3):] = 1
    L = _lib.lib()
    for key_tok in (None, tok):
        got = np.zeros((B, T, H * hd), np.float32)
        _lib.check(L.pg_dbg_attention_hd(0, PREC[precision], _lib.ptr(x), _lib.ptr(got), B, T, H, hd,
                                         _lib.ptr(key_tok) if key_tok is not None else None, 1))
        want = ref.softmax_attention(x, B, T, H, hd, None if key_tok is None else key_tok == 1)
        err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
        print("\n[attention hd%d T=%d H=%d %s pad=%d] relative error %.3e" % (hd, T, H, precision, key_tok is not None, err))
        # strict: split-bf16 products and a context returned as a (hi, lo) bf16 pair, 16-17 mantissa bits: the bound of the head-64
        # strict kernel's test (first measured value at head 32: 1.3e-5 at T = 16); 16-bit modes: P and the context are rounded to the
        # operand type (bf16: the bound the head-64 kernel is held to on inputs drawn the same way; fp16 has three more mantissa bits)
        tol = {"fp32": 6e-5, "bf16": 2.5e-2, "fp16": 4e-3}[precision]
        assert np.isfinite(got).all() and err < tol, (T, H, precision, key_tok is not None, err)


def check_attention_hd_at_64_is_pg_dbg_attention():
    B, T, H = 2, 70, 3
    x = np.random.default_rng(3).standard_normal((B, T, 3 * H * 64)).astype(np.float32) * np.float32(0.5)
    L = _lib.lib()
    for prec in PREC.values():
        a, b = np.zeros((B, T, H * 64), np.float32), np.zeros((B, T, H * 64), np.float32)
        _lib.check(L.pg_dbg_attention(0, prec, _lib.ptr(x), _lib.ptr(a), B, T, H))
        _lib.check(L.pg_dbg_attention_hd(0, prec, _lib.ptr(x), _lib.ptr(b), B, T, H, 64, None, -1))
        assert np.array_equal(a, b)
    assert L.pg_dbg_attention_hd(0, _lib.PG_PREC_BF16, _lib.ptr(x), _lib.ptr(a), B, T, H, 48, None, -1) != 0


def check_rope_hd(size, T, H):
    hd = SIZES[size]["hd"]
    B = 2 if T < 600 else 1
    rng = np.random.default_rng(T * 31 + H)
    x = (rng.standard_normal((B * T, 3 * H * hd)) * 2.0).astype(np.float32)
    L = _lib.lib()
    d2 = 2 * H * hd
    got = x.copy()
    _lib.check(L.pg_dbg_rope_hd(0, _lib.PG_PREC_FP32, _lib.ptr(got), B, T, H, hd))
    want = ref.rotate_qkv_rows(x, B, T, H, hd)
    assert np.array_equal(got, want)                                            # strict mode: the host fp32 loop, bit for bit (v included)
    assert np.array_equal(got[:, d2:], x[:, d2:]) and np.array_equal(got[0, :d2], x[0, :d2])
    if T > 1:
        assert not np.array_equal(got[1, :d2], x[1, :d2])
    # 16-bit modes: round16(rotate_fp32(round16(x))) within one ulp of the 16-bit type
    for prec, rnd, mant in ((_lib.PG_PREC_BF16, round_bf16, 7), (_lib.PG_PREC_F16, round_f16, 10)):
        got = x.copy()
        _lib.check(L.pg_dbg_rope_hd(0, prec, _lib.ptr(got), B, T, H, hd))
        x16 = rnd(x)
        want = rnd(ref.rotate_qkv_rows(x16, B, T, H, hd))
        assert np.array_equal(got[:, d2:], x16[:, d2:])                          # v: the input's 16-bit value, untouched
        ulp16 = np.spacing(np.maximum(np.abs(want[:, :d2]), np.float32(2.0 ** -14))) * np.float32(2.0 ** (23 - mant))
        assert (np.abs(got[:, :d2] - want[:, :d2]) <= ulp16).all()


def check_rope_hd_refuses_one_head_too_many(size):
    hd, most = SIZES[size]["hd"], SIZES[size]["max_heads"]
    x = np.zeros((2, 3 * (most + 1) * hd), np.float32)
    assert _lib.lib().pg_dbg_rope_hd(0, _lib.PG_PREC_BF16, _lib.ptr(x), 1, 2, most + 1, hd) != 0


# ---- forward ------------------------------------------------------------------------------------------------------------------------
def padded_batch(rng):
    """three rows of 40, 23 and 9 tokens, right-padded to 40"""
    tok = np.full((3, 40), 1, dtype=np.int64)
    lens = (40, 23, 9)
    for b, n in enumerate(lens):
        tok[b, :n] = tokens(rng, 1, n, mask_every=5)[0]
    return tok, lens


def check_forward(size, shape, precision):
    """The engine against the numpy reference over FWD_BATCHES, then on a right-padded batch: <pad> keys are masked and positions are
    token indices, so a padded row equals the row run alone.  fp32: 1e-3 absolute; 16-bit modes: the row's bound, absolute or per
    unit of the batch's logit std."""
    row = SIZES[size]
    fwd = row["forward"]
    cfg, sd, rcfg = case(size, **fwd["shapes"][shape])
    if fwd.get("full_size"):
        assert (cfg["d_model"], cfg["n_layers"], cfg["n_heads"], cfg["d_ffn"]) == row["shape"]
    lm = size_model(size, cfg, sd, precision).model.to("cuda:0")
    per_std = fwd["per_std"] and precision != "fp32"
    bound = lambda std: 1e-3 if precision == "fp32" else fwd["tol"][precision] * (std if per_std else 1.0)
    name = "ESM-2 %s%s, %s" % (shape + ", " if shape else "", row["label"], precision)
    rng = np.random.default_rng(5)
    worst, std = 0.0, 1.0
    for B, T in FWD_BATCHES:
        tok = tokens(rng, B, T)
        want = ref.esm2_forward(sd, rcfg, tok)
        got = lm.forward_logits(tok)
        assert got.shape == want.shape == (B, T, 33)
        std = float(want.std())
        err = np.abs(got - want).max()
        worst = max(worst, err / (std if per_std else 1.0))
        print("\n[%s, T=%d] max|engine - reference| = %.3e (logit std %.2f)" % (name, T, err, std))
        assert err < bound(std), (T, err, std)
    tok, lens = padded_batch(rng)
    got = lm.forward_logits(tok)
    want = ref.esm2_forward(sd, rcfg, tok)
    for b, n in enumerate(lens):
        err = np.abs(got[b, :n] - want[b, :n]).max()
        assert err < bound(float(want.std())), (b, err)
        alone = lm.forward_logits(tok[b:b + 1, :n])
        assert np.abs(alone[0] - got[b, :n]).max() < (2e-4 if precision == "fp32" else 0.08)
    print("\n[%s] max|engine - reference| over %d sequence lengths = %.3e %s (logit std %.2f)"
          % (name, len(FWD_BATCHES), worst, "per unit of logit std" if per_std else "absolute", std))


def check_huggingface_logits(name):
    size, shape, tok_shape = HF_FIXTURES[name]
    z = np.load(os.path.join(HERE, "golden", "esm2_hf_%s.npz" % name))
    cfg = weights.make_config(SIZES[size]["base"], **json.loads(str(z["cfg"])))
    assert (cfg["d_model"], cfg["n_heads"], cfg["n_layers"]) == shape and z["tokens"].shape == tok_shape
    sd = weights.synthetic_state_dict(cfg, seed=int(z["seed"]), std=float(z["std"]), embed_std=float(z["embed_std"]),
                                      ln_jitter=float(z["ln_jitter"]))
    for precision, tol in (("fp32", 1e-3), ("fp16", 0.04)):
        got = size_model(size, cfg, sd, precision).model.to("cuda:0").forward_logits(z["tokens"])
        err = np.abs(got - z["logits"]).max()
        print("\n[ESM-2 %d x %d against HuggingFace, %s] max|engine - HF| = %.3e" % (cfg["n_layers"], cfg["d_model"], precision, err))
        assert err < tol, precision


def check_full_size_strict_logits(size):
    """the released shape, two chains, strict mode against the fp32 reference"""
    row = SIZES[size]
    full = row["full"]
    cfg = dict(row["base"])
    assert (cfg["d_model"], cfg["n_layers"], cfg["n_heads"], cfg["d_ffn"]) == row["shape"]
    sd = weights.synthetic_state_dict(cfg, seed=0, std=full["std"], embed_std=full["embed_std"], ln_jitter=0.1)
    lm = size_model(size, cfg, sd, "fp32").model.to("cuda:0")
    tok = tokens(np.random.default_rng(3), 2, full["T"], mask_every=9)
    got = lm.forward_logits(tok)
    want = ref.esm2_forward(sd, ref.Esm2Config.of(cfg), tok)
    err = np.abs(got - want).max()
    print("\n[ESM-2 %d x %d, fp32] std %g embed_std %g: max|engine - reference| = %.3e (logit std %.2f)"
          % (cfg["n_layers"], cfg["d_model"], full["std"], full["embed_std"], err, want.std()))
    lo, hi = full.get("logit_std", (0.0, np.inf))
    assert lo < want.std() < hi
    assert err < 1e-3


def check_auto_precision(size):
    """precision="auto" (fp16 behind the range guard) resolves and runs; where the row says so, synthetic=True builds the full
    configuration and it runs"""
    row = SIZES[size]
    cfg, sd, rcfg = case(size, **row["auto"]["case"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = row["wrapper"](state_dict=sd, config=cfg)                            # precision="auto"
    lm = m.model.to("cuda:0")
    tok = tokens(np.random.default_rng(1), 2, 30)
    want = ref.esm2_forward(sd, rcfg, tok)
    assert np.abs(lm.forward_logits(tok) - want).max() < 0.05 * max(1.0, float(want.std()))
    if row["auto"]["full_synthetic"] and not weights.find_cached_checkpoint(row["file"] + ".pt"):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            full = row["wrapper"](synthetic=True)
        assert (full.cfg["d_model"], full.cfg["n_layers"], full.cfg["n_heads"], full.cfg["d_ffn"]) == row["shape"]
        out = full.model.to("cuda:0").forward_logits(tok)
        assert out.shape == (2, 30, 33) and np.isfinite(out).all()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
OTHER_ARCHS = {"ESM-1b": ("ESM1B_CONFIG", "ESM1b"), "ESM-MSA-1b": ("MSA1B_CONFIG", "ESM_MSA1"), "ESM-1": ("ESM1_T6_CONFIG", "ESM6")}


def check_other_architectures_refuse_the_width(size, arch):
    base, cls = OTHER_ARCHS[arch]
    cfg = weights.make_config(getattr(weights, base), n_layers=1, d_ffn=512, max_positions=40, **SIZES[size]["other_archs"])
    sd = weights.synthetic_state_dict(cfg, seed=1)
    m = model(getattr(models, cls), cfg, sd, "bf16")
    with pytest.raises(Exception, match=r"%s with heads of %d.*64" % (arch, SIZES[size]["hd"])):
        m.model.to("cuda:0")


# ---- the sampler --------------------------------------------------------------------------------------------------------------------
def check_sampler(size):
    """positions bit-exact with random.sample, every draw replayed by the oracle, iteration 0's logits and the log-likelihoods (one
    position masked at a time, and unmasked) against the reference, the substitution tables against the likelihoods"""
    row = SIZES[size]
    cfg, sd, rcfg = case(size, **row["sampler"])
    s = esm_sampler.ESM_sampler(size_model(size, cfg, sd, "fp32"), device="cuda:0")
    assert s.get_init_seq("AA", 5, 1).tolist() == [[0, 5, 5, 32, 32, 32, 2]]
    s.draw_seed, s.record = 11, True
    random.seed(2)
    out = s.generate(4, SEED25, batch_size=4, num_iters=3, num_positions=5, top_k=3, burnin=2, temperature=0.9, show_progress_bar=False)
    assert len(out) == 4 and all(len(x) == 25 for x in out)
    run = s.last_run[0]
    random.seed(2)
    table = np.asarray([[random.sample(range(1, 26), 5) for _ in range(4)] for _ in range(3)])
    assert (run["table"] == table).all(), "position selection is not bit-exact with random.sample"
    replay_draws(s, run, 4, 5, 3, 3, 2, 0.9, 11)
    # iteration 0's logits are those of the seed masked at the chosen positions
    tok = s.get_init_seq(SEED25, 25, 4).numpy()
    for b in range(4):
        tok[b, table[0, b]] = 32
    want = ref.esm2_forward(sd, rcfg, tok)
    for b in range(4):
        assert np.abs(run["sampled_logits"][0][b] - want[b, table[0, b]]).max() < 1e-3
    # log-likelihoods: one position masked at a time (the copies as one reference batch), and unmasked, against the reference's log-softmax
    seq = row["seq"]
    ll, per = s.log_likelihood(seq)
    tok = s.get_init_seq(seq, len(seq), 1).numpy()
    batch = np.repeat(tok, len(seq), axis=0)
    batch[np.arange(len(seq)), np.arange(1, len(seq) + 1)] = 32
    lg = ref.esm2_forward(sd, rcfg, batch)
    masked = [ref.log_softmax(lg[i, i + 1])[tok[0, i + 1]] for i in range(len(seq))]
    assert np.abs(np.asarray(per) - np.asarray(masked)).max() < 2e-3 and abs(ll - np.mean(masked)) < 1e-3
    ll0, per0 = s.log_likelihood(seq, with_masking=False)
    lp = ref.log_softmax(ref.esm2_forward(sd, rcfg, tok)[0])
    plain = [lp[i, tok[0, i]] for i in range(1, len(seq) + 1)]
    assert np.abs(np.asarray(per0) - np.asarray(plain)).max() < 2e-3 and abs(ll0 - np.mean(plain)) < 1e-3
    # the substitution table read at the sequence's own residues is the likelihood's list, bit for bit
    seqs = [seq, seq[:20], SEED25]
    lls = list(s.log_likelihood_batch(seqs))
    for sq, (ll_b, per_b), (logp, entropy, toks) in zip(seqs, lls, s.masked_marginals_batch(seqs)):
        own = np.asarray([logp[i, toks.index(c)] for i, c in enumerate(sq)], dtype=np.float32)
        assert np.array_equal(own, np.asarray(per_b, dtype=np.float32)) and np.isfinite(entropy).all()
    assert np.array_equal(np.asarray(lls[0][1], dtype=np.float32), np.asarray(per, dtype=np.float32))


# ---- one chain: the hipGraph path ---------------------------------------------------------------------------------------------------
def _single_chain_run(size):
    cfg, sd, _ = case(size, **SIZES[size]["single_chain"])
    return single_chain_run(size_model(size, cfg, sd, "bf16"))


def _single_chain_child(size):
    _, out = _single_chain_run(size)
    print("CHILD_TOKENS " + json.dumps(out))


def check_single_chain(size):
    """the graph was captured and replayed; the same job in a fresh child process with graphs off (PGIBBS_GRAPH is read once per
    process) gives the same sequence; and recorded (eager loop, logits emitted): same sequence, every draw replayed by the oracle"""
    s, out = _single_chain_run(size)
    lm = s.model.model
    assert lm.get_stat("graph_captures") == 1 and lm.get_stat("graph_replays") > 0
    lines = child(__name__, "_single_chain_child", size, timeout=SIZES[size].get("child_timeout", 300), PGIBBS_GRAPH="0")
    line = [l for l in lines if l.startswith("CHILD_TOKENS ")][-1]
    assert json.loads(line[len("CHILD_TOKENS "):]) == out
    again = single_chain_generate(s, True)
    assert again == out
    replay_draws(s, s.last_run[0], 1, 3, 12, 0, float("inf"), 1.0, 21)


# ---- a job and its shards, at a size ------------------------------------------------------------------------------------------------
def _shard_job(size, worlds):
    sh = SIZES[size]["shards"]
    cfg, sd, _ = case(size, **sh["case"])
    return shard_job(size_model(size, cfg, sd, "bf16"), worlds, B=sh["B"])


def _shard_child(size):
    print("CHILD_DIGEST " + _shard_job(size, (2,)))


def check_shards(size):
    """A job of config 2's chain length run whole and as the row's worlds of contiguous shards: tokens and the logits of every draw, bit
    for bit; where the row says so, a child process with PGIBBS_ATTN_SPLIT=0 gives the same bits"""
    sh = SIZES[size]["shards"]
    digest = _shard_job(size, sh["worlds"])
    assert digest
    if sh["split_child"]:
        line = [l for l in child(__name__, "_shard_child", size, PGIBBS_ATTN_SPLIT="0") if l.startswith("CHILD_DIGEST ")][-1]
        assert line.split()[1] == digest
