"""Sequence representations without a GPU: the two C entries are declared and bound and refuse on the host, the layer numbers are
normalised as fair-esm's, ESM_sampler.embed_batch groups, chunks and ranges as documented (against a recording stand-in for the engine),
the embed_esm front end parses, writes and refuses file names, and the float32 references of tests/_repr_reference.py agree with
tests/_esm2_reference.py."""
import io
import os
import re

import numpy as np
import pytest
import torch

import _esm2_reference as r2
import _repr_reference as rr
from _fake_engine import fake_engine_model
from protein_gibbs_sampler_amd import _lib, embed_esm, esm_sampler, weights
from protein_gibbs_sampler_amd.alphabet import Alphabet
from protein_gibbs_sampler_amd.engine import NativeMaskedLM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "pg_esm_forward_representations"


# ---- the C entries ----------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "pgibbs.h")).read()
    bound = {n: a for n, _, a in _lib.SIGNATURES}
    for name, n_args in ((ENTRY, 10), ("pg_repr_dbg_rows", 16)):
        decl = re.search(r"PG_API int %s\(([^;]*)\);" % name, hdr)
        assert decl and len(decl.group(1).split(",")) == n_args == len(bound[name])
        assert hasattr(_lib.lib(), name)


def _refused(rc, message):
    assert rc == _lib.PG_ERR_INVALID
    assert message in _lib.lib().pg_last_error().decode(), _lib.lib().pg_last_error()


def _call(h=None, tok=True, B=2, T=5, layers=(0, 2), n_req=None, pools=None, n_pools=0, per_token=True, pooled=False):
    tokens = np.full((max(B, 1), max(T, 1)), 5, np.int32)
    lay = np.asarray(layers, np.int32)
    pl = np.asarray(pools, np.int32) if pools is not None else None
    rows = np.zeros(len(lay) * tokens.size * 8, np.float32)
    means = np.zeros(len(lay) * max(n_pools, 1) * max(B, 1) * 8, np.float32)
    return _lib.lib().pg_esm_forward_representations(
        h, _lib.ptr(tokens) if tok else None, B, T, _lib.ptr(lay) if layers is not None and len(lay) else None,
        len(lay) if n_req is None else n_req, _lib.ptr(pl) if pl is not None else None, n_pools, _lib.ptr(rows) if per_token else None,
        _lib.ptr(means) if pooled else None)


def test_every_host_refusal_has_its_message_and_needs_no_device():
    """In the order pgibbs.h states; none of them looks for a device or into the (null) engine."""
    _refused(_call(tok=False), ENTRY + ": null argument")
    _refused(_call(layers=()), ENTRY + ": null argument")
    _refused(_call(n_req=0), "no layer requested")
    _refused(_call(layers=(-1, 2)), "layer -1 is outside")
    _refused(_call(layers=(2, 2)), "strictly ascending")
    _refused(_call(layers=(2, 1)), "strictly ascending")
    _refused(_call(per_token=False), "neither per-token nor pooled output")
    _refused(_call(pooled=True), "pooled output requested without pools")
    whole = [[[0, 5], [0, 5]]]
    _refused(_call(pools=[[[0, 5], [1, 5]]], n_pools=1, pooled=True), "pool 0 of sequence 1 leaves the token row [0, 5]")
    _refused(_call(pools=[[[0, 5], [-1, 2]]], n_pools=1, pooled=True), "leaves the token row")
    _refused(_call(pools=[[[0, 5], [2, -1]]], n_pools=1, pooled=True), "pool 0 of sequence 1 has a negative count")
    _refused(_call(pools=whole, n_pools=1, pooled=True), ENTRY + ": null engine")
    _refused(_call(), ENTRY + ": null engine")


def test_kernel_entry_refuses_on_the_host_and_needs_a_device():
    L = _lib.lib()
    x = np.zeros((6, 64), np.float32)
    g = np.ones(64, np.float32)
    tok = np.zeros(6, np.int32)
    out, means = np.zeros((6, 64), np.float32), np.zeros((1, 2, 64), np.float32)
    pools = np.asarray([[[0, 3], [1, 2]]], np.int32)

    def call(x_=x, M=6, d=64, d_live=64, gamma=g, beta=g, rows=out, B=2, T=3, pl=pools, n_pools=1, pm=means):
        p = lambda a: _lib.ptr(a) if a is not None else None
        return L.pg_repr_dbg_rows(0, p(x_), M, d, d_live, p(gamma), p(beta), 1e-5, p(tok), 1, p(rows), B, T, p(pl), n_pools, p(pm))
    _refused(call(x_=None), "pg_repr_dbg_rows: bad argument")
    _refused(call(rows=None), "pg_repr_dbg_rows: bad argument")
    _refused(call(M=0), "pg_repr_dbg_rows: bad argument")
    _refused(call(d=66), "no width of the row kernels")
    _refused(call(d=2816), "no width of the row kernels")
    _refused(call(d_live=68), "no width of the row kernels")
    _refused(call(beta=None), "gamma and beta come together")
    _refused(call(pm=None), "pools and pooled_out come together")
    _refused(call(T=4), "pooling needs M = B * T")
    _refused(call(pl=np.asarray([[[0, 3], [2, 2]]], np.int32)), "leaves the token row")
    if L.pg_device_count() == 0:
        assert call() == _lib.PG_ERR_NO_DEVICE
        assert call(gamma=None, beta=None, pl=None, pm=None) == _lib.PG_ERR_NO_DEVICE


# ---- layer numbers ----------------------------------------------------------------------------------------------------------------------
def _host_lm(n_layers=3):
    cfg = weights.make_config(weights.ESM2_T33_CONFIG, d_model=128, n_layers=n_layers, d_ffn=256, max_positions=64)
    return NativeMaskedLM(cfg, {}, precision="bf16")


def test_negative_layers_count_from_the_end():
    lm = _host_lm(3)
    assert lm.normalise_layers([-1]) == [3] and lm.normalise_layers((0, -1, -3)) == [0, 3, 1]
    assert lm.normalise_layers([3, 0, -2]) == [3, 0, 2]
    assert lm.normalise_layers([-4]) == [0]
    for bad in ([4], [-5], [1.5]):
        with pytest.raises(ValueError, match="outside"):
            lm.normalise_layers(bad)
    for twice in ([-1, 3], [0, -4], [2, 2]):
        with pytest.raises(ValueError, match="twice"):
            lm.normalise_layers(twice)
    with pytest.raises(ValueError, match="no representation layer"):
        lm.normalise_layers([])
    # refused before the engine is asked for: this object is not resident anywhere
    with pytest.raises(ValueError, match="twice"):
        lm.forward_representations(np.zeros((1, 4), np.int32), (-1, 3))
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        lm.forward_representations(np.zeros((1, 4), np.int32), (-1,))


# ---- embed_batch against a recording stand-in ----------------------------------------------------------------------------------------------
D = 8


def _standin(arch="ESM-1b"):
    """fake_engine_model's plug-in with a recording forward_representations: row t of sequence b at layer l holds
    token * 100 + t + l / 10 in every feature, so what comes back says which token rows were read."""
    plug = fake_engine_model(False)
    if arch == "ESM-1":
        plug.alphabet = Alphabet(True, False, arch="ESM-1")
        plug.batch_converter = plug.alphabet.get_batch_converter()
    lm = plug.model
    lm.cfg = {"n_layers": 4, "d_model": D, "arch": _lib.PG_ARCH_ESM1 if arch == "ESM-1" else _lib.PG_ARCH_ESM1B}

    def forward_representations(tokens, layers, pools=None, per_token=True):
        want = lm.normalise_layers(layers)
        tok = np.asarray(tokens)
        lm.trace.append(("forward_representations", tok.copy(), tuple(layers), None if pools is None else np.asarray(pools).copy(), per_token))
        rows = np.stack([(tok * 100 + np.arange(tok.shape[1])[None, :] + l / 10.0)[..., None].repeat(D, -1) for l in want]).astype(np.float32)
        means = None
        if pools is not None:
            means = np.stack([rr.pooled(rows[k], pools) for k in range(len(want))])
        return (rows if per_token else None), means
    lm.forward_representations = forward_representations
    return plug


@pytest.fixture
def gpu_named(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)


SEQS = ["ACDEFGH", "M", "KLMNPQR", "ACDEFGHIKLMNPQRSTVWYACDEFGHIKL"]       # lengths 7, 1, 7, 30


@pytest.mark.parametrize("arch", ["ESM-1b", "ESM-1"])
@pytest.mark.parametrize("batch_size", [1, 2, None])
def test_embed_batch_groups_chunks_and_ranges(gpu_named, arch, batch_size):
    plug = _standin(arch)
    s = esm_sampler.ESM_sampler(plug, device="gpu")
    eos = 1 if plug.alphabet.append_eos else 0
    assert (arch == "ESM-1") == (eos == 0)
    out = list(s.embed_batch(SEQS, repr_layers=(-1, 0), include=("mean", "per_tok", "bos"), batch_size=batch_size))
    lm = plug.model
    calls = [t for t in lm.trace if t[0] == "forward_representations"]
    # one group per length, in order of first appearance, each in chunks of batch_size; no <pad> reaches the model
    sizes = {1: [1, 1, 1, 1], 2: [2, 1, 1], None: [2, 1, 1]}[batch_size]
    assert [c[1].shape[0] for c in calls] == sizes
    assert [c[1].shape[1] for c in calls] == [{1: [9, 9, 3, 32], 2: [9, 3, 32], None: [9, 3, 32]}[batch_size][i] - (1 - eos) for i in range(len(calls))]
    assert all((c[1] != plug.alphabet.padding_idx).all() for c in calls)
    assert lm.job_items == [2, 0, 1, 0, 1, 0]                                # every group a job of its size, reset after it
    for c in calls:
        nb, T = c[1].shape
        L = T - 1 - eos
        assert c[2] == (-1, 0) and c[4] is True
        assert c[3].tolist() == [[[1, L]] * nb, [[0, 1]] * nb]                 # "mean": the residues only; "bos": the first token
    cls = plug.alphabet.cls_idx
    for seq, res in zip(SEQS, out):
        assert set(res) == {"mean", "per_tok", "bos"} and all(set(v) == {-1, 0} for v in res.values())
        tok = np.asarray([plug.alphabet.get_idx(c) for c in seq])
        for layer, l in ((-1, 4), (0, 0)):
            rows = (tok * 100 + np.arange(1, len(seq) + 1) + l / 10.0).astype(np.float32)
            assert res["per_tok"][layer].shape == (len(seq), D) and np.array_equal(res["per_tok"][layer][:, 0], rows)
            assert np.array_equal(res["mean"][layer], rr.sequential_mean(rows[:, None].repeat(D, 1), 0, len(seq)))
            assert np.array_equal(res["bos"][layer], np.full(D, cls * 100 + l / 10.0, np.float32))
    # only what was asked for: no per-token rows are requested from the engine for a mean alone
    lm.trace.clear()
    res = s.embed("ACD")
    assert set(res) == {"mean"} and set(res["mean"]) == {-1}
    (call,) = [t for t in lm.trace if t[0] == "forward_representations"]
    assert call[4] is False and call[3].tolist() == [[[1, 3]]]


def test_embed_batch_refusals(gpu_named):
    s = esm_sampler.ESM_sampler(_standin(), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        next(s.embed_batch(["ACD"]))
    s = esm_sampler.ESM_sampler(_standin(), device="gpu")
    with pytest.raises(ValueError, match="include"):
        next(s.embed_batch(["ACD"], include=("mean", "contacts")))
    with pytest.raises(ValueError, match="twice"):
        next(s.embed_batch(["ACD"], repr_layers=(-1, 4)))


# ---- the front end ------------------------------------------------------------------------------------------------------------------------
def test_cli_parser():
    args = embed_esm.build_parser().parse_args(["-i", "in.fasta", "-o", "out"])
    assert (args.repr_layers, args.include, args.batch_size, args.model, args.precision) == ([-1], ["mean"], None, "esm1v", "auto")
    args = embed_esm.build_parser().parse_args(["-i", "a", "-o", "b", "--model", "esm2_35m", "--repr_layers", "0", "-1", "6", "--include",
                                                "mean", "per_tok", "bos", "--batch_size", "4", "--precision", "bf16", "--synthetic-weights"])
    assert (args.repr_layers, args.include, args.batch_size, args.model) == ([0, -1, 6], ["mean", "per_tok", "bos"], 4, "esm2_35m")
    assert args.synthetic_weights and args.precision == "bf16"
    with pytest.raises(SystemExit):
        embed_esm.build_parser().parse_args(["-i", "a", "-o", "b", "--include", "contacts"])
    with pytest.raises(SystemExit):
        embed_esm.build_parser().parse_args(["-o", "b"])


def test_cli_writes_one_file_per_record(gpu_named, tmp_path):
    s = esm_sampler.ESM_sampler(_standin(), device="gpu")
    fasta = ">sp|P1|first protein\nACDEFGH\n>second\nM\n>third.v2\nKLM-NPQR*\n"
    files = embed_esm.main(io.StringIO(fasta), str(tmp_path / "out"), [-1, 0], ["mean", "per_tok", "bos"], 2, s)
    assert files == ["sp|P1|first.npz", "second.npz", "third.v2.npz"]
    want = list(s.embed_batch(["ACDEFGH", "M", "KLMNPQR"], (-1, 0), ("mean", "per_tok", "bos")))
    for name, res in zip(files, want):
        z = np.load(tmp_path / "out" / name)
        assert sorted(z.files) == sorted("%s_%d" % (k, l) for k in ("mean", "per_tok", "bos") for l in (-1, 0))
        for kind in res:
            for layer in res[kind]:
                assert np.array_equal(z["%s_%d" % (kind, layer)], res[kind][layer]) and z["%s_%d" % (kind, layer)].dtype == np.float32


@pytest.mark.parametrize("names,message", [
    (["ok", "a/b"], r"record 2 \('a/b'\): the id 'a/b' is not a safe file name"),
    (["../x"], "not a safe file name"),
    ([".hidden"], "not a safe file name"),
    ([""], "not a safe file name"),
    (["a b", "c", "a other"], r"record 3 \('a other'\): the id 'a' was already used by record 1"),
])
def test_cli_refuses_unsafe_and_duplicate_ids(names, message, gpu_named, tmp_path):
    with pytest.raises(ValueError, match=message):
        embed_esm.record_file_names(names)
    if all(names):
        s = esm_sampler.ESM_sampler(_standin(), device="gpu")
        with pytest.raises(ValueError, match=message):
            embed_esm.main(io.StringIO("".join(">%s\nACD\n" % n for n in names)), str(tmp_path / "out"), [-1], ["mean"], None, s)
        assert not (tmp_path / "out").exists() and not s.model.model.trace      # refused before anything ran or was written


# ---- the references -----------------------------------------------------------------------------------------------------------------------
def test_sequential_mean_is_a_float32_running_sum():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((40, 12)) * 100).astype(np.float32)
    acc = np.float32(0)
    for t in range(3, 40):
        acc = np.float32(acc + x[t, 5])
    assert rr.sequential_mean(x, 3, 37)[5] == np.float32(acc / np.float32(37))
    assert np.array_equal(rr.sequential_mean(x, 7, 1), x[7]) and not rr.sequential_mean(x, 4, 0).any()
    pools = np.asarray([[[0, 5], [2, 0]], [[1, 3], [0, 8]]])
    got = rr.pooled(x[:16].reshape(2, 8, 12), pools)
    assert got.shape == (2, 2, 12) and np.array_equal(got[1, 1], rr.sequential_mean(x[8:16], 0, 8)) and not got[0, 1].any()


@pytest.mark.parametrize("pad", [False, True])
def test_esm2_layers_compose_to_esm2_forward(pad):
    cfg = weights.make_config(weights.ESM2_T33_CONFIG, d_model=128, n_layers=3, d_ffn=256, max_positions=64)
    sd = weights.synthetic_state_dict(cfg, seed=3, std=0.05, embed_std=0.3, ln_jitter=0.1)
    rcfg = r2.Esm2Config.of(cfg)
    rng = np.random.default_rng(1)
    tok = np.concatenate([np.zeros((2, 1), np.int64), rng.integers(4, 24, (2, 11)), np.full((2, 1), 2)], axis=1)
    tok[0, 4] = 32
    if pad:
        tok[1, 8:] = 1
    states = rr.esm2_layers(sd, rcfg, tok)
    assert len(states) == 4 and all(s.shape == (2, 13, 128) and s.dtype == np.float32 for s in states)
    assert np.array_equal(rr.esm2_lm_head(sd, rcfg, states[-1]), r2.esm2_forward(sd, rcfg, tok))          # exactly
    assert not states[0][tok == 1].any() and not states[0][tok == 32].any()
    # neighbouring layers are far apart on the scale the GPU tests resolve
    for a, b in zip(states[:-1], states[1:]):
        assert np.sqrt(((a - b) ** 2).mean()) > 0.3 * b.std()
