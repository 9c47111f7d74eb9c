"""Sequence representations on the GPU (pg_esm_forward_representations, csrc/repr.hip): the two kernels alone through pg_repr_dbg_rows,
bit for bit against pg_dbg_layernorm and the float32 sequential mean; the engine's layers against the fp32 references (the oracle's
return_layers for ESM-1b, oracle.esm1_forward's trunk steps for ESM-1, tests/_repr_reference.py for the ESM-2 sizes) and against
HuggingFace's recorded hidden states; and the structure of the call: subsets of layers, pools, the persistent launch, batch sizes,
and what a representations call leaves behind for the calls after it."""
import functools
import json
import os
import warnings

import numpy as np
import pytest

import _esm2_gpu_common as C
import _repr_reference as rr
from _esm2_sizes import FWD_TOL_PER_STD, SIZES
from oracle import esm1_forward as E1
from oracle import esm_forward as E
from protein_gibbs_sampler_amd import _lib, esm_sampler, models, weights

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PRECISIONS = ["fp32", "bf16", "fp16"]
BATCHES = [(1, 8), (3, 27), (3, 34), (2, 130)]
STRICT_LOGIT_TOL = 1e-3
# max |engine - reference| / std(reference layer) over layers 0 .. n - 1, every model and batch below, per precision mode: the first
# measured run on an MI355X (against the fp32 references, never against a rerun of the engine); the tests hold 2.5 x these.
# Measured 4.75e-5 (strict; worst: ESM-2 heads of 16, layer 2), 2.40e-2 (bf16; ESM-2 heads of 128, layer 2), 2.99e-3 (fp16; ESM-2 heads of
# 24, layer 2).  Layer n, not bounded here, measured 6.0e-5 / 3.1e-2 / 3.5e-3; its logits through the fp32 head at most 7.2e-5 / 2.6e-2 /
# 3.1e-3 of the logit std, against the forward tests' 1e-3 absolute / 0.05 / 0.008
REPR_MEASURED = {"fp32": 4.8e-5, "bf16": 2.4e-2, "fp16": 3.0e-3}
REPR_BOUND = {p: 2.5 * v for p, v in REPR_MEASURED.items()}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ==== the kernels alone ====================================================================================================================
def _dbg_rows(x, d_live, gamma=None, beta=None, tokens=None, pad_idx=1, B=0, T=0, pools=None):
    M, d = x.shape
    rows = np.full((M, d_live), np.float32(np.nan))
    means = np.full((pools.shape[0], B, d_live), np.float32(np.nan)) if pools is not None else None
    p = lambda a: _lib.ptr(a) if a is not None else None
    _lib.check(_lib.lib().pg_repr_dbg_rows(0, p(x), M, d, d_live, p(gamma), p(beta), 1e-5, p(tokens), pad_idx, p(rows), B, T, p(pools),
                                           pools.shape[0] if pools is not None else 0, p(means)))
    return rows, means


@pytest.mark.parametrize("d,d_live", [(64, 64), (320, 320), (640, 480), (1280, 1280), (2560, 2560), (5120, 5120)])
def test_row_and_pool_kernels_bit_for_bit(d, d_live):
    """With LayerNorm: pg_dbg_layernorm's bits on the live columns; without: a copy; <pad> rows zeros; the pooled values the float32
    sequential mean -- no tolerance anywhere.  T 1 ... 130 (several rows per wave, several workgroups), B 1 and 3, two pools at once
    with counts 0, 1 and T - 2."""
    rng = np.random.default_rng(d + d_live)
    g = (1 + 0.1 * rng.standard_normal(d_live)).astype(np.float32)
    b = (0.1 * rng.standard_normal(d_live)).astype(np.float32)
    for T in (1, 3, 33, 130):
        for B in (1, 3):
            M = B * T
            x = (rng.standard_normal((M, d)) * 3).astype(np.float32)
            x[:, d_live:] = 0                                                      # an embedded model's structural zeros
            tok = rng.integers(4, 24, M).astype(np.int32)
            if M > 1:
                tok[rng.choice(M, max(1, M // 5), replace=False)] = 1
            live = np.ascontiguousarray(x[:, :d_live])
            pools = np.zeros((2, B, 2), np.int32)
            for s in range(B):
                pools[0, s] = (1, T - 2) if T > 2 else (0, T)
                pools[1, s] = (T - 1, 1) if s % 2 == 0 else (T // 2, 0)
            # a copy
            rows, means = _dbg_rows(x, d_live, tokens=tok, B=B, T=T, pools=pools)
            want = np.where((tok == 1)[:, None], np.float32(0), live)
            assert np.array_equal(_bits(rows), _bits(want)), (T, B)
            assert np.array_equal(_bits(means), _bits(rr.pooled(rows.reshape(B, T, d_live), pools))), (T, B)
            assert not means[1, 1::2].any()
            # without tokens nothing is zeroed
            rows, _ = _dbg_rows(x, d_live)
            assert np.array_equal(_bits(rows), _bits(live))
            # LayerNorm
            ln = np.zeros_like(live)
            _lib.check(_lib.lib().pg_dbg_layernorm(0, _lib.ptr(live), _lib.ptr(g), _lib.ptr(b), _lib.ptr(ln), M, d_live, 1e-5))
            rows, means = _dbg_rows(x, d_live, g, b, tokens=tok, B=B, T=T, pools=pools)
            want = np.where((tok == 1)[:, None], np.float32(0), ln)
            assert np.array_equal(_bits(rows), _bits(want)), (T, B)
            assert np.array_equal(_bits(means), _bits(rr.pooled(rows.reshape(B, T, d_live), pools))), (T, B)


# ==== the engine against the fp32 references ===============================================================================================
def _esm1_layers(sd, ocfg, tok):
    """oracle.esm1_forward's trunk, step by step: the n + 1 states; ESM-1 has no final LayerNorm, layer n is the raw stream."""
    x, pad = E1.esm1_embed(sd, ocfg, tok)
    states = [x]
    for i in range(ocfg.n_layers):
        p = "layers.%d." % i
        h = E1.layer_norm(x, sd[p + "self_attn_layer_norm.weight"], sd[p + "self_attn_layer_norm.bias"], 1e-12)
        x = x + E1.mha_bias_kv(sd, p + "self_attn.", ocfg, h, pad)
        h = E1.layer_norm(x, sd[p + "final_layer_norm.weight"], sd[p + "final_layer_norm.bias"], 1e-12)
        h = E1.gelu(E1.linear(h, sd[p + "fc1.weight"], sd[p + "fc1.bias"]))
        x = (x + E1.linear(h, sd[p + "fc2.weight"], sd[p + "fc2.bias"])).astype(np.float32)
        states.append(x)
    return states


def _esm1b_layers(sd, ocfg, tok):
    x, states = E.esm1b_trunk(sd, ocfg, tok, return_layers=True)
    states[-1] = x
    return states


def _esm1_tokens(rng, B, T, mask_every=7):
    tok = np.concatenate([np.full((B, 1), 32), rng.integers(4, 24, (B, T - 1))], axis=1)
    tok[:, 2:T:mask_every] = 33
    return tok


@functools.lru_cache(maxsize=None)
def _family(name):
    """-> dict(cfg, sd, wrapper, layers(tok) -> the reference's n + 1 states, head(x) -> the reference's logits of layer n, tokens, ends
    = the tokens around the residues)"""
    if name == "esm1b":      # 3 x 1024: a width the persistent single-chain launch takes at (1, 8)
        cfg = weights.make_config(weights.ESM1B_CONFIG, d_model=1024, n_layers=3, n_heads=16, d_ffn=4096, max_positions=160)
        sd = weights.synthetic_state_dict(cfg, seed=5, std=0.03, embed_std=0.3, ln_jitter=0.1)
        ocfg = E.EsmConfig(d_model=1024, n_layers=3, n_heads=16, d_ffn=4096, max_pos=160)
        return dict(cfg=cfg, sd=sd, wrapper=models.ESM1b, layers=lambda t: _esm1b_layers(sd, ocfg, t), head=lambda x: E.lm_head(sd, x),
                    tokens=C.tokens, ends=(1, 1))
    if name == "esm1":
        cfg = weights.make_config(weights.ESM1_T6_CONFIG, n_layers=3, d_model=256, d_ffn=1024)
        sd = weights.synthetic_state_dict(cfg, seed=7, std=0.03, embed_std=0.05, ln_jitter=0.1)
        ocfg = E1.Esm1Config(d_model=256, n_layers=3, n_heads=4, d_ffn=1024)
        return dict(cfg=cfg, sd=sd, wrapper=models.ESM6, layers=lambda t: _esm1_layers(sd, ocfg, t), head=lambda x: E1.esm1_head(sd, x),
                    tokens=_esm1_tokens, ends=(1, 0))
    over = {"esm2": dict(n_layers=3, d=256), "esm2_150m": dict(n_layers=3, d=256), "esm2_8m": dict(n_layers=3), "esm2_15b": dict(n_layers=3),
            "esm2_35m": dict(n_layers=3, d=480)}[name]
    cfg, sd, rcfg = C.case(name, **over)
    sd = dict(sd)
    return dict(cfg=cfg, sd=sd, wrapper=SIZES[name]["wrapper"], layers=lambda t: rr.esm2_layers(sd, rcfg, t),
                head=lambda x: rr.esm2_lm_head(sd, rcfg, x), tokens=C.tokens, ends=(1, 1))


FAMILIES = ["esm1b", "esm1", "esm2", "esm2_8m", "esm2_150m", "esm2_15b", "esm2_35m"]


def _lm(name, precision):
    f = _family(name)
    return C.model(f["wrapper"], f["cfg"], f["sd"], precision).model.to("cuda:0")


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The token batches of a family and the reference's states on them: computed once, shared by the precision modes, never changed.
    The last batch is the ragged one, in tests/_esm2_gpu_common.padded_batch's shape (rows of 40, 23 and 9 tokens right-padded to 40)."""
    f = _family(name)
    rng = np.random.default_rng(5)
    out = []
    for B, T in BATCHES:
        tok = f["tokens"](rng, B, T)
        out.append((tok, [T] * B, f["layers"](tok)))
    tok = np.full((3, 40), 1, dtype=np.int64)
    lens = [40, 23, 9]
    for b, n in enumerate(lens):
        tok[b, :n] = f["tokens"](rng, 1, n, mask_every=5)[0]
    out.append((tok, lens, f["layers"](tok)))
    for _, _, states in out:
        for s in states:
            s.setflags(write=False)
    return out


def _rms(a):
    return float(np.sqrt(np.mean(np.square(a, dtype=np.float64))))


@functools.lru_cache(maxsize=None)
def _measure(name, precision):
    """One engine of (family, mode) over every batch, all layers at once with the per-residue mean: the figures the tests assert on."""
    f = _family(name)
    n = f["cfg"]["n_layers"]
    d = f["cfg"]["d_model"]
    lm = _lm(name, precision)
    lo, hi = f["ends"]
    fig = dict(logit=[], dev=[], ratio=[], sq_n=0.0, count_n=0, pad_zero=True, pool_bits=True, mean_dev=0.0)
    for tok, lens, ref in _reference(name):
        B, T = tok.shape
        pools = np.asarray([[[lo, ln - lo - hi] for ln in lens]], np.int32)
        rows, means = lm.forward_representations(tok, list(range(n + 1)), pools)
        assert rows.shape == (n + 1, B, T, d) and means.shape == (n + 1, 1, B, d) and rows.dtype == means.dtype == np.float32
        assert np.isfinite(rows).all()
        real = np.arange(T)[None, :] < np.asarray(lens)[:, None]
        fig["pad_zero"] &= not rows[:, ~real].any()
        fig["pool_bits"] &= all(np.array_equal(_bits(means[l]), _bits(rr.pooled(rows[l], pools))) for l in range(n + 1))
        want = f["head"](ref[n][real])
        std = float(want.std())
        fig["logit"].append((float(np.abs(f["head"](rows[n][real]) - want).max()), std))
        fig["dev"].append([float(np.abs(rows[l][real] - ref[l][real]).max() / ref[l][real].std()) for l in range(n + 1)])
        ratio = []
        for l in range(n + 1):
            own = _rms(rows[l][real] - ref[l][real])
            other = min(_rms(rows[l][real] - ref[k][real]) for k in (l - 1, l + 1) if 0 <= k <= n)
            ratio.append(own / other)
        fig["ratio"].append(ratio)
        fig["sq_n"] += float(np.sum(np.square(rows[n][real] - ref[n][real], dtype=np.float64)))
        fig["count_n"] += int(real.sum()) * d
        for l in range(n):      # the mean of the reference's real residues: an error of the mean is at most the largest error of a row
            for b, ln in enumerate(lens):
                want_mean = ref[l][b, lo:ln - hi].astype(np.float64).mean(axis=0)
                fig["mean_dev"] = max(fig["mean_dev"], float(np.abs(means[l, 0, b] - want_mean).max() / ref[l][real].std()))
    fig["rms_n"] = (fig["sq_n"] / fig["count_n"]) ** 0.5
    print("\n[representations %s %s] layer-n logits max|err| / logit std per batch %s; max|engine - reference| / std per layer, worst batch %s; "
          "rms(own layer) / rms(neighbouring layer), worst %.3g; rms at layer n %.3e"
          % (name, precision, ["%.3g" % (e / s) for e, s in fig["logit"]], ["%.3g" % max(b[l] for b in fig["dev"]) for l in range(n + 1)],
             max(max(r) for r in fig["ratio"]), fig["rms_n"]))
    return fig


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", FAMILIES)
def test_layers_against_the_fp32_reference(name, precision):
    """Every batch of BATCHES and the right-padded ragged batch.  Layer n, pushed through the REFERENCE's fp32 LM head, gives logits
    within the bound the forward tests hold that mode to.  Every layer is much nearer its own reference layer than either
    neighbouring one (a tap one block off cannot pass: neighbouring reference layers of these models are at least 0.24 std apart).  Layers below n
    stay within 2.5 x the first measured max|engine - reference| / std.  <pad> rows are zeros and the mean covers the real
    residues only."""
    fig = _measure(name, precision)
    n = _family(name)["cfg"]["n_layers"]
    for i, (err, std) in enumerate(fig["logit"]):
        assert err < (STRICT_LOGIT_TOL if precision == "fp32" else FWD_TOL_PER_STD[precision] * std), (i, err, std)
    for i, ratio in enumerate(fig["ratio"]):
        assert all(r < 0.1 for r in ratio), (i, ratio)
    assert fig["pad_zero"] and fig["pool_bits"]
    for i, dev in enumerate(fig["dev"]):
        assert max(dev[:n]) < REPR_BOUND[precision], (i, dev)
    assert fig["mean_dev"] < REPR_BOUND[precision]


@pytest.mark.parametrize("name", FAMILIES)
def test_layer_n_is_nearer_the_reference_in_the_finer_modes(name):
    errs = [_measure(name, p)["rms_n"] for p in ("fp32", "fp16", "bf16")]
    assert errs[0] < errs[1] < errs[2], errs


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("name", ["esm_hf_repr", "esm2_hf_repr"])
def test_huggingface_hidden_states(name, precision):
    """HuggingFace's output_hidden_states on 3 x 128 (tests/golden/make_golden_representations.py): the recorded rows and residue means
    of all n + 1 layers, held to the bounds of the reference tests."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    recipe = json.loads(str(z["cfg"]))
    kw = dict(seed=int(z["seed"]), std=float(z["std"]), embed_std=float(z["embed_std"]), ln_jitter=float(z["ln_jitter"]))
    if name == "esm2_hf_repr":
        cfg = weights.make_config(weights.ESM2_T33_CONFIG, **recipe)
        sd = weights.synthetic_state_dict(cfg, **kw)
        rcfg = C.ref.Esm2Config.of(cfg)
        wrapper, head = models.ESM2, lambda x: rr.esm2_lm_head(sd, rcfg, x)
    else:
        cfg = weights.make_config(weights.ESM1B_CONFIG, d_model=recipe["d_model"], n_layers=recipe["n_layers"], d_ffn=recipe["d_ffn"],
                                  max_positions=recipe["max_pos"])
        sd = E.synthetic_esm_weights(E.EsmConfig(**recipe), **kw)
        wrapper, head = models.ESM1b, lambda x: E.lm_head(sd, x)
    n = cfg["n_layers"]
    tok = z["tokens"]
    B, T = tok.shape
    lm = C.model(wrapper, cfg, sd, precision).model.to("cuda:0")
    pools = np.asarray([[[1, T - 2]] * B], np.int32)
    rows, means = lm.forward_representations(tok, list(range(n + 1)), pools)
    got = rows.reshape(n + 1, B * T, -1)[:, z["rows"]]
    assert got.shape == z["per_token"].shape and means[:, 0].shape == z["means"].shape
    for l in range(n):
        std = z["per_token"][l].std()
        dev, mdev = np.abs(got[l] - z["per_token"][l]).max() / std, np.abs(means[l, 0] - z["means"][l]).max() / std
        print("\n[%s %s] layer %d: max|engine - HF| / std = %.3e (means %.3e)" % (name, precision, l, dev, mdev))
        assert dev < REPR_BOUND[precision] and mdev < REPR_BOUND[precision], (l, dev, mdev)
    want = head(z["per_token"][n])
    err = np.abs(head(got[n]) - want).max()
    print("\n[%s %s] layer n through the fp32 head: max|logit err| = %.3e (logit std %.2f)" % (name, precision, err, want.std()))
    assert err < (STRICT_LOGIT_TOL if precision == "fp32" else FWD_TOL_PER_STD[precision] * want.std())


# ==== structure: bit for bit ===============================================================================================================
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["esm1b", "esm2_35m"])
def test_subsets_pools_and_the_calls_around(name, precision):
    f = _family(name)
    n = f["cfg"]["n_layers"]
    lm = _lm(name, precision)
    rng = np.random.default_rng(11)
    for B, T in [(1, 8), (3, 27)]:
        tok = f["tokens"](rng, B, T)
        before = lm.forward_logits(tok)
        pools = np.asarray([[[1, T - 2]] * B, [[0, 1]] * B, [[2, 0]] * B], np.int32)
        rows, means = lm.forward_representations(tok, list(range(n + 1)), pools)
        # a layer asked for alone is that layer of the request for all of them -- (1, 8) on ESM-1b in the 16-bit modes: layer n alone
        # (and with layer 0) comes out of the persistent single-chain launch, next to an intermediate layer out of the per-layer launches
        for l in range(n + 1):
            alone, m_alone = lm.forward_representations(tok, [l], pools)
            assert np.array_equal(_bits(alone[0]), _bits(rows[l])) and np.array_equal(_bits(m_alone[0]), _bits(means[l])), (B, T, l)
        ends, _ = lm.forward_representations(tok, [0, n])
        inner, _ = lm.forward_representations(tok, [1, n])
        assert np.array_equal(_bits(ends[1]), _bits(rows[n])) and np.array_equal(_bits(inner[1]), _bits(rows[n]))
        assert np.array_equal(_bits(ends[0]), _bits(rows[0])) and np.array_equal(_bits(inner[0]), _bits(rows[1]))
        # the caller's order, and negative numbers
        swapped, _ = lm.forward_representations(tok, [-1, 0])
        assert np.array_equal(_bits(swapped[0]), _bits(rows[n])) and np.array_equal(_bits(swapped[1]), _bits(rows[0]))
        # pools: the float32 sequential mean of the same call's rows; "bos" is row 0; a count of 0 is zeros; pools alone
        for l in range(n + 1):
            assert np.array_equal(_bits(means[l]), _bits(rr.pooled(rows[l], pools)))
            assert np.array_equal(_bits(means[l, 1]), _bits(rows[l][:, 0])) and not means[l, 2].any()
        none, only = lm.forward_representations(tok, [n], pools, per_token=False)
        assert none is None and np.array_equal(_bits(only[0]), _bits(means[n]))
        # fair-esm's call shape
        out = lm(tok, repr_layers=[0, n])
        assert sorted(out) == ["logits", "representations"] and sorted(out["representations"]) == [0, n]
        assert np.array_equal(_bits(out["representations"][0].numpy()), _bits(rows[0]))
        assert np.array_equal(_bits(out["representations"][n].numpy()), _bits(rows[n]))
        assert sorted(lm(tok)) == ["logits"] and np.array_equal(_bits(out["logits"].numpy()), _bits(lm(tok)["logits"].numpy()))
        # and the logits after all of this are the logits before it
        assert np.array_equal(_bits(lm.forward_logits(tok)), _bits(before))
    assert rows.shape[-1] == f["cfg"]["d_model"] == (480 if name == "esm2_35m" else 1024)


def test_engine_refusals_that_need_an_engine():
    lm = _lm("esm1", "bf16")
    tok = _esm1_tokens(np.random.default_rng(0), 2, 9).astype(np.int32)
    lay = np.asarray([0, 4], np.int32)
    out = np.zeros((2, 2, 9, 256), np.float32)
    L = _lib.lib()
    assert L.pg_esm_forward_representations(lm.handle, _lib.ptr(tok), 2, 9, _lib.ptr(lay), 2, None, 0, _lib.ptr(out), None) == _lib.PG_ERR_INVALID
    assert "layer 4 is outside 0 .. 3" in L.pg_last_error().decode()
    bad = tok.copy()
    bad[1, 3] = 35
    lay[1] = 3
    assert L.pg_esm_forward_representations(lm.handle, _lib.ptr(bad), 2, 9, _lib.ptr(lay), 2, None, 0, _lib.ptr(out), None) == _lib.PG_ERR_INVALID
    assert "token 35 at flat index 12" in L.pg_last_error().decode()
    from oracle.msa_forward import MsaConfig, synthetic_msa_weights
    ck = dict(d_model=128, n_layers=2, n_heads=2, d_ffn=256, max_pos=64, max_rows=16)
    cfg = weights.make_config(weights.MSA1B_CONFIG, d_model=128, n_layers=2, n_heads=2, d_ffn=256, max_positions=64, max_msa_rows=16)
    msa = C.model(models.ESM_MSA1, cfg, synthetic_msa_weights(MsaConfig(**ck), seed=1), "bf16").model.to("cuda:0")
    assert L.pg_esm_forward_representations(msa.handle, _lib.ptr(tok), 2, 9, _lib.ptr(lay), 2, None, 0, _lib.ptr(out), None) == _lib.PG_ERR_INVALID
    assert "the MSA engine has no representations entry" in L.pg_last_error().decode()
    with pytest.raises(ValueError, match="MSA engine"):
        msa.forward_representations(tok[None], [0])


def test_embed_batch_does_not_depend_on_batch_size():
    f = _family("esm2_35m")
    s = esm_sampler.ESM_sampler(C.model(f["wrapper"], f["cfg"], f["sd"], "bf16"), device="cuda:0")
    seqs = ["ACDEFGH", "M", "KLMNPQR", "ACDEFGHIKLMNPQRSTVWYACDEFGHIKL", "WYVTSRQ"]
    kinds = ("mean", "per_tok", "bos")
    runs = [list(s.embed_batch(seqs, repr_layers=(-1, 1), include=kinds, batch_size=bs)) for bs in (1, 2, None)]
    for seq, a, b, c in zip(seqs, *runs):
        for kind in kinds:
            for layer in (-1, 1):
                assert a[kind][layer].shape == ((len(seq), 480) if kind == "per_tok" else (480,))
                assert np.array_equal(_bits(a[kind][layer]), _bits(b[kind][layer])) and np.array_equal(_bits(a[kind][layer]), _bits(c[kind][layer]))
        assert np.array_equal(_bits(a["mean"][1]), _bits(rr.sequential_mean(a["per_tok"][1], 0, len(seq))))
    # the residues only, and a sequence's own rows: sequence 0 alone
    tok = s.model.batch_converter([("0", seqs[0])])[2].numpy()
    rows, _ = s.model.model.forward_representations(tok, [1])
    assert np.array_equal(_bits(runs[0][0]["per_tok"][1]), _bits(rows[0, 0, 1:-1])) and np.array_equal(_bits(runs[0][0]["bos"][1]), _bits(rows[0, 0, 0]))
    assert s.embed(seqs[3], repr_layers=[0])["mean"][0].shape == (480,)


def test_generate_is_unchanged_by_a_representations_call_in_between():
    """A seeded 12-iteration single-chain generate (the hipGraph path) twice on one engine, with and without a representations call
    between the two runs: the same tokens."""
    cfg, sd, _ = C.case("esm2", n_layers=3, d=256, seed=13)
    outs = {}
    for between in (False, True):
        s, first = C.single_chain_run(C.size_model("esm2", cfg, sd, "bf16"))
        lm = s.model.model
        if between:
            tok = C.tokens(np.random.default_rng(2), 3, 27)
            rows, _ = lm.forward_representations(tok, [0, 2, 3])
            assert np.isfinite(rows).all()
        outs[between] = (first, C.single_chain_generate(s, False))
        assert lm.get_stat("graph_replays") > 0
    assert outs[True] == outs[False] and outs[True][0] == outs[True][1]


def test_auto_precision_falls_back_to_bf16_on_an_overflow_at_an_intermediate_layer(monkeypatch):
    """tests/test_gpu_fp16_mode.py's recipe: fc1 weights of block 2 that fit fp16 but drive GELU(fc1) past 65504, the probe off.  The
    fp16 engine's layers 2 and 3 are not finite, the entry answers PG_ERR_RANGE and the wrapper runs the call on the bf16 engine."""
    monkeypatch.setenv("PGIBBS_F16_PROBE", "0")
    cfg = weights.make_config(weights.ESM1B_CONFIG, d_model=256, n_layers=3, d_ffn=512, max_positions=128)
    sd = {k: v.copy() for k, v in weights.synthetic_state_dict(cfg, seed=21, std=0.05, embed_std=0.3, ln_jitter=0.1).items()}
    sd["layers.1.fc1.weight"] *= np.float32(1e5)
    assert np.abs(sd["layers.1.fc1.weight"]).max() < 65504
    tok = C.tokens(np.random.default_rng(2), 3, 42)
    pools = np.asarray([[[1, 40]] * 3], np.int32)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        lm = models.ESM1b(state_dict=sd, config=cfg).model.to("cuda:0")
        early, _ = lm.forward_representations(tok, [0, 1])                     # below the overflow: fp16 values, no fallback
    assert lm.precision_name == "fp16" and lm.fallbacks == 0 and np.isfinite(early).all()
    with pytest.warns(UserWarning, match="run again with bf16 operands"):
        rows, means = lm.forward_representations(tok, [1, 2, 3], pools)
    assert lm.fallbacks == 1 and np.isfinite(rows).all() and np.isfinite(means).all()
    bf = models.ESM1b(state_dict=sd, config=cfg, precision="bf16").model.to("cuda:0")
    want, want_means = bf.forward_representations(tok, [1, 2, 3], pools)
    assert np.array_equal(_bits(rows), _bits(want)) and np.array_equal(_bits(means), _bits(want_means))
    with pytest.raises(_lib.PgError) as err:
        models.ESM1b(state_dict=sd, config=cfg, precision="fp16").model.to("cuda:0").forward_representations(tok, [3], pools, per_token=False)
    assert err.value.code == _lib.PG_ERR_RANGE
