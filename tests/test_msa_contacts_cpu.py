"""MSA Transformer contact prediction without a GPU: the numpy reference (tests/_msa_contact_reference.py) against the oracle's trunk and
an independent torch restatement of the tied row maps, its fp32 fold against its float64 form under the derived rounding bound, every
host refusal of pg_msa_forward_contacts and of the two kernel-level entries, the plan text of the scores launcher,
ESM_MSA_sampler.predict_contacts_batch's grouping and memory cap (against a recording stand-in for the engine), the model holder's
regression loading, and the contacts_esm_msa front end."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _contact_reference as cr
import _msa_contact_reference as mr
from _fake_engine import fake_engine_model
from oracle import msa_forward as M
from protein_gibbs_sampler_amd import _lib, contacts_esm, contacts_esm_msa, esm_msa_sampler, models, weights
from protein_gibbs_sampler_amd.engine import NativeMaskedLM
from test_contacts_cpu import fold_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "pg_msa_forward_contacts"
CK = dict(d_model=128, n_layers=2, n_heads=2, d_ffn=256, max_pos=80, max_rows=16)


def _tokens(rng, B, R, C):
    tok = rng.integers(4, 24, (B, R, C))
    tok[rng.random((B, R, C)) < 0.1] = 30
    tok[rng.random((B, R, C)) < 0.1] = 32
    tok[..., 0] = 0
    return tok


def _ragged(rng):
    """two MSAs, 4 x 15 and 2 x 9, padded to one [2][4][15] tensor as the batch converter pads them"""
    tok = np.full((2, 4, 15), 1)
    tok[0] = _tokens(rng, 1, 4, 15)[0]
    tok[1, :2, :9] = _tokens(rng, 1, 2, 9)[0]
    return tok


# ---- the reference ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ragged", [False, True])
def test_reference_trunk_and_maps(ragged):
    """The helper's trunk output is the oracle's, and its maps are an independent torch restatement's (fair-esm's einsum string, torch's
    softmax) to 1e-6; rows sum to 1; with <pad> the key columns that are <pad> in row 0 are exactly 0."""
    ocfg = M.MsaConfig(**CK)
    sd = M.synthetic_msa_weights(ocfg, seed=4, std=0.08, embed_std=0.5, ln_jitter=0.1)
    rng = np.random.default_rng(3)
    tok = _ragged(rng) if ragged else _tokens(rng, 2, 3, 11)
    A, out = mr.msa_row_attentions(sd, ocfg, tok)
    B, R, C = tok.shape
    assert A.shape == (2, B, 2, C, C) and A.dtype == np.float32
    assert np.array_equal(out, M.msa_trunk(sd, ocfg, tok))
    assert np.abs(A.astype(np.float64).sum(-1) - 1).max() < 1e-6
    # block 0 again, from the embedding, in fair-esm's R x C x B x H x D layout
    x = M.msa_embed(sd, ocfg, tok)
    p = "layers.0.row_self_attention."
    h = torch.nn.functional.layer_norm(torch.from_numpy(x), (128,), torch.from_numpy(sd[p + "layer_norm.weight"]),
                                       torch.from_numpy(sd[p + "layer_norm.bias"]), 1e-5).permute(1, 2, 0, 3)      # R C B D
    lin = lambda t, n: torch.nn.functional.linear(t, torch.from_numpy(sd[p + "layer." + n + ".weight"]), torch.from_numpy(sd[p + "layer." + n + ".bias"]))
    q = lin(h, "q_proj").view(R, C, B, 2, 64) * (64 ** -0.5 / np.sqrt(R))
    k = lin(h, "k_proj").view(R, C, B, 2, 64)
    pad = torch.from_numpy(tok == 1)
    if ragged:
        q = q * (1 - pad.permute(1, 2, 0).unsqueeze(3).unsqueeze(4).to(q))
    a = torch.einsum("rinhd,rjnhd->hnij", q, k)
    if ragged:
        a = a.masked_fill(pad[:, 0].unsqueeze(0).unsqueeze(2), -10000)
    want = torch.softmax(a, -1).permute(1, 0, 2, 3).numpy()
    assert np.abs(A[0] - want).max() < 1e-6
    if ragged:
        assert not A[:, 1, :, :, 9:].any() and A[:, 0].min() > 0


def test_kernel_level_reference_is_the_same_map():
    """row_probs_f64 of a qkv buffer equals the trunk's row_map arithmetic on the same q and k (float64 against float32: 1e-6)"""
    rng = np.random.default_rng(5)
    B, R, C, H = 2, 3, 7, 2
    qkv = rng.standard_normal((B * R * C, 3 * H * 64)).astype(np.float32)
    tok = np.full((B, R, C), 5)
    tok[1, 0, 5:] = 1
    tok[0, 2, 3] = 1
    scale = np.float32(0.125 / np.sqrt(R))
    P, s, mag, filled = mr.row_probs_f64(qkv, B, R, C, H, scale, tok, 1)
    x = qkv.astype(np.float64).reshape(B, R, C, 3, H, 64)
    q = np.where((tok == 1)[..., None, None], 0.0, x[:, :, :, 0]) * float(scale)
    a = np.einsum("brihd,brjhd->bhij", q, x[:, :, :, 1])
    a = np.where((tok[:, 0] == 1)[:, None, None, :], -10000.0, a)
    e = np.exp(a - a.max(-1, keepdims=True))
    assert np.abs(P - e / e.sum(-1, keepdims=True)).max() < 1e-12
    assert filled.tolist() == (tok[:, 0] == 1).tolist() and not P[1, :, :, 5:].any() and (mag >= np.abs(np.where(filled[:, None, None, :], 0, s)) - 1e-9).all()


@pytest.mark.parametrize("C", [2, 7, 34, 131])
def test_the_two_forms_of_the_fold_agree_under_the_derived_bound(C):
    """tests/test_contacts_cpu.py's fold_bound: it takes the window off a [B][T] token batch with <cls> and <eos>, so the maps get one
    trailing column whose token is <eos> -- the window and the live mask are then exactly the MSA form's."""
    rng = np.random.default_rng(C)
    L, B, H = 3, 2, 4
    a = np.exp(3.0 * rng.standard_normal((L, B, H, C, C)))
    A = (a / a.sum(-1, keepdims=True)).astype(np.float32)
    tok0 = np.full((B, C), 6)
    tok0[:, 0] = 0
    if C >= 7:
        tok0[1, C - 3:] = 1
    w = (5 * rng.standard_normal(L * H)).astype(np.float32)
    l64, c64 = mr.row_contacts_f64(A, tok0, w, -0.3, 1)
    l32 = mr.row_contacts_f32(A, tok0, w, -0.3, 1)
    assert l32.dtype == np.float32 and l32.shape == l64.shape == (B, C - 1, C - 1)
    Ap = np.zeros((L, B, H, C + 1, C + 1), np.float32)
    Ap[..., :C, :C] = A
    tokp = np.concatenate([tok0, np.full((B, 1), 2)], axis=1)
    assert np.array_equal(cr.contacts_from_attentions_f64(Ap, tokp, w, -0.3, 2, 1)[0], l64)      # the same window, the same numbers
    assert np.array_equal(cr.contacts_from_attentions_f32(Ap, tokp, w, -0.3, 2, 1), l32)
    bound = fold_bound(Ap, tokp, w, -0.3, 2, 1)
    assert (np.abs(l32 - l64) <= bound).all(), float((np.abs(l32 - l64) / bound).max())
    assert bound.max() < 1e-3 * max(1.0, l64.std())
    assert np.array_equal(l32, l32.transpose(0, 2, 1)) and np.allclose(c64, 1 / (1 + np.exp(-l64)))
    dead = ~(mr.live_window(tok0, -1, 1, 0)[:, :, None] & mr.live_window(tok0, -1, 1, 0)[:, None, :])
    assert (l32[dead] == np.float32(-0.3)).all() and (l64[dead] == -0.3).all()
    # tail = 1 of the helper is tests/_contact_reference.py's fold
    assert np.array_equal(mr.fold_layer_f32(Ap[0], tokp, w[:H], 0.1, True, True, None, 2, 1, 1), cr.fold_layer_f32(Ap[0], tokp, w[:H], 0.1, True, True, None, 2, 1))


# ---- the C entries --------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "pgibbs.h")).read()
    bound = {n: a for n, _, a in _lib.SIGNATURES}
    for name, n_args in ((ENTRY, 10), ("pg_msa_contact_dbg_probs", 13), ("pg_contact_dbg_accumulate_window", 16)):
        decl = re.search(r"PG_API int %s\(([^;]*)\);" % name, hdr)
        assert decl and len(decl.group(1).split(",")) == n_args == len(bound[name]), name
        assert hasattr(_lib.lib(), name)
    assert bound[ENTRY][0] is _lib.EngineHandle


def _refused(rc, message):
    assert rc == _lib.PG_ERR_INVALID
    assert message in _lib.lib().pg_last_error().decode(), _lib.lib().pg_last_error()


def _call(h=None, tok=True, B=2, R=3, C=5, contacts=True, logits=False, layers=None, n_attn=None, attn=False):
    tokens = np.full((2, 3, 8), 5, np.int32)
    out = np.zeros(2 * 8 * 8, np.float32)
    big = np.zeros(4 * 2 * 4 * 64, np.float32)
    lay = np.asarray(layers, np.int32) if layers is not None else None
    return _lib.lib().pg_msa_forward_contacts(h, _lib.ptr(tokens) if tok else None, B, R, C, _lib.ptr(out) if contacts else None,
                                              _lib.ptr(out) if logits else None, _lib.ptr(lay) if lay is not None else None,
                                              (len(lay) if lay is not None else 0) if n_attn is None else n_attn, _lib.ptr(big) if attn else None)


def test_every_host_refusal_has_its_message_and_needs_no_device():
    """In the order pgibbs.h states, up to the null engine; the refusals that read the engine are in tests/test_gpu_msa_contacts.py."""
    _refused(_call(tok=False), ENTRY + ": null tokens")
    _refused(_call(tok=False, contacts=False), ENTRY + ": null tokens")
    _refused(_call(contacts=False), "no output requested")
    _refused(_call(attn=True), "come together or not at all")
    _refused(_call(layers=[0, 1]), "come together or not at all")
    _refused(_call(layers=[0, 1], n_attn=0, attn=True), "come together or not at all")
    _refused(_call(layers=[0], n_attn=-1, attn=True), "come together or not at all")
    _refused(_call(layers=[-1, 0], attn=True), "attention layer -1 is negative")
    _refused(_call(layers=[1, 1], attn=True), "strictly ascending")
    _refused(_call(layers=[2, 1], attn=True), "strictly ascending")
    _refused(_call(C=1), "C = 1: a contact map needs <cls> and at least one position")
    _refused(_call(C=1, layers=[0], attn=True, contacts=False), "C = 1")
    _refused(_call(), ENTRY + ": null engine")
    _refused(_call(layers=[0, 2], attn=True, contacts=False), ENTRY + ": null engine")
    w = np.zeros(4, np.float32)
    _refused(_lib.lib().pg_engine_set_contact_head(None, _lib.ptr(w), 4, 0.0), "pg_engine_set_contact_head: null engine")


def test_kernel_entries_refuse_on_the_host_and_report_the_plan_without_a_device():
    L = _lib.lib()
    qkv = np.zeros((1 * 2 * 5, 3 * 2 * 64), np.float32)
    out = np.zeros((1, 2, 5, 5), np.float32)
    plan = ctypes.create_string_buffer(128)

    def probs(precision=_lib.PG_PREC_BF16, q=qkv, B=1, R=2, C=5, H=2, o=out, pl=plan, nb=128, tok=None):
        return L.pg_msa_contact_dbg_probs(0, precision, _lib.ptr(q) if q is not None else None, B, R, C, H, 0.125, _lib.ptr(tok) if tok is not None else None,
                                          1, _lib.ptr(o) if o is not None else None, pl, nb)
    _refused(probs(precision=7), "unknown precision mode")
    _refused(probs(q=None), "pg_msa_contact_dbg_probs: bad argument")
    _refused(probs(C=0), "pg_msa_contact_dbg_probs: bad argument")
    _refused(probs(R=0), "pg_msa_contact_dbg_probs: bad argument")
    _refused(probs(o=None, pl=None), "pg_msa_contact_dbg_probs: bad argument")
    # the plan alone: no output buffer, no device.  One workgroup = (msa, head, 64 queries, one key tile): 64-key tiles up to 64 columns,
    # 160-key tiles beyond -- C = 64 | 65 and 160 | 161 are the two sides of each step, 513 the widest benchmarked alignment
    B, R, H = 2, 3, 2
    for C, kb, kt, wg in ((3, 4, 1, 4), (64, 4, 1, 4), (65, 10, 1, 8), (160, 10, 1, 12), (161, 10, 2, 24), (513, 10, 4, 144)):
        assert wg == B * H * -(-C // 64) * kt
        for precision, name in ((_lib.PG_PREC_BF16, "row-scores"), (_lib.PG_PREC_F16, "row-scores"), (_lib.PG_PREC_FP32, "row-scores-f32")):
            assert probs(precision=precision, B=B, R=R, C=C, H=H, o=None) == _lib.PG_OK
            assert plan.value.decode() == "%s kb%d kt%d %dwg" % (name, kb, kt, wg), (C, plan.value)
    tok = np.zeros((B, R, 65), np.int32)
    assert probs(B=B, R=R, C=65, H=H, o=None, tok=tok) == _lib.PG_OK and plan.value.decode() == "row-scores kb10 kt1 pad 8wg"
    P = np.zeros((1, 2, 5, 5), np.float32)
    tokf = np.zeros((1, 3, 5), np.int32)
    w = np.zeros(2, np.float32)
    lg = np.zeros((1, 4, 4), np.float32)

    def fold(P_=P, T=5, H=2, lg_=lg, tail=0, stride=15):
        return L.pg_contact_dbg_accumulate_window(0, _lib.ptr(P_) if P_ is not None else None, _lib.ptr(tokf), -1, 1, _lib.ptr(w), 0.0, 1, 1,
                                                  _lib.ptr(lg_) if lg_ is not None else None, None, 1, T, H, tail, stride)
    _refused(fold(P_=None), "pg_contact_dbg_accumulate_window: bad argument")
    _refused(fold(lg_=None), "pg_contact_dbg_accumulate_window: bad argument")
    _refused(fold(H=0), "pg_contact_dbg_accumulate_window: bad argument")
    _refused(fold(tail=2), "tail must be 0 or 1")
    _refused(fold(T=1), "T must be at least 2")
    _refused(fold(T=2, tail=1), "T must be at least 3")
    _refused(fold(stride=4), "tok_stride must be at least T")
    if L.pg_device_count() == 0:
        assert probs() == _lib.PG_ERR_NO_DEVICE and fold() == _lib.PG_ERR_NO_DEVICE


# ---- the engine wrapper and the model holder -------------------------------------------------------------------------------------------
def _msa_cfg():
    return weights.make_config(weights.MSA1B_CONFIG, d_model=128, n_layers=2, n_heads=2, d_ffn=256, max_positions=64, max_msa_rows=16)


def test_engine_wrapper_checks_before_the_engine_is_asked_for():
    lm = NativeMaskedLM(_msa_cfg(), {}, precision="bf16")
    n = lm.cfg["n_layers"] * lm.cfg["n_heads"]
    with pytest.raises(ValueError, match="%d weights for a model of 2 layers x 2 heads = %d channels" % (n + 1, n)):
        lm.set_row_contact_head(np.zeros(n + 1), 0.0)
    with pytest.raises(ValueError, match="finite"):
        lm.set_row_contact_head(np.full(n, np.inf), 0.0)
    with pytest.raises(ValueError, match="finite"):
        lm.set_row_contact_head(np.zeros(n), np.nan)
    tok = np.zeros((1, 2, 5), np.int32)
    with pytest.raises(RuntimeError, match="no contact head set"):
        lm.predict_row_contacts(tok)
    lm.set_row_contact_head(np.ones(n), 0.5)                                    # kept on the host object until a handle exists
    assert lm.has_row_contact_head and not lm.has_contact_head
    for bad, message in (([2], "outside"), ([-3], "outside"), ([0, -2], "twice"), ([1.5], "outside")):
        with pytest.raises(ValueError, match=message):
            lm.forward_row_attentions(tok, bad)
    with pytest.raises(ValueError, match="no attention layer"):
        lm.forward_row_attentions(tok, [])
    with pytest.raises(ValueError, match="C = 1"):
        lm.predict_row_contacts(np.zeros((1, 2, 1), np.int32))
    with pytest.raises(ValueError, match=r"tokens \[B, R, C\]"):
        lm.predict_row_contacts(np.zeros((2, 5), np.int32))
    with pytest.raises(ValueError, match="no output requested"):
        lm.forward_row_contacts(tok, contacts=False)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        lm.predict_row_contacts(tok)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        lm.forward_row_attentions(tok)
    lm.set_row_contact_head(None, 0.0)
    assert not lm.has_row_contact_head
    # the three refusals that stay: the [B, T] names on the MSA engine, the row names on an ESM engine
    with pytest.raises(ValueError, match="MSA engine has no contact head"):
        lm.set_contact_head(np.zeros(n), 0.0)
    with pytest.raises(ValueError, match="MSA engine has no contact head"):
        lm.forward_contacts(np.zeros((1, 5), np.int32))
    esm = NativeMaskedLM(weights.make_config(weights.ESM2_T33_CONFIG, d_model=128, n_layers=3, d_ffn=512, max_positions=64), {}, precision="bf16")
    with pytest.raises(ValueError, match="row-attention contacts are the MSA engine's"):
        esm.set_row_contact_head(np.zeros(6), 0.0)
    with pytest.raises(ValueError, match="row-attention contacts are the MSA engine's"):
        esm.forward_row_contacts(tok)


def test_model_holder_loads_the_regression(tmp_path):
    cfg = _msa_cfg()
    n = cfg["n_layers"] * cfg["n_heads"]
    m = models.ESM_MSA1(config=cfg, synthetic=True, seed=4)
    assert m.has_row_contacts and not m.has_contacts
    assert m.model.has_row_contact_head and np.array_equal(m.model._contact_head[0], weights.synthetic_contact_head(cfg, 4)[0])
    with pytest.raises(RuntimeError, match="no CPU implementation"):          # the head is there; the engine is not on a GPU
        m.predict_row_contacts(np.zeros((1, 2, 5), np.int32))
    with pytest.raises(NotImplementedError, match="ESM_MSA1.*predict_row_contacts"):      # the [B, T] name stays refused, and says where to go
        m.predict_contacts(np.zeros((1, 2, 5), np.int32))
    # weights handed in as a state dict: nothing was looked for
    sd = weights.synthetic_state_dict(cfg, seed=2)
    m = models.ESM_MSA1(state_dict=sd, config=cfg)
    assert not m.model.has_row_contact_head
    with pytest.raises(RuntimeError, match="handed in as a state dict"):
        m.predict_row_contacts(np.zeros((1, 2, 5), np.int32))
    # a checkpoint: none, in the sibling file, in the file itself, and one of another model
    ocfg = M.MsaConfig(d_model=128, n_layers=2, n_heads=2, d_ffn=256, max_pos=64, max_rows=16)
    blob = {"model": {k: torch.from_numpy(v) for k, v in M.synthetic_msa_weights(ocfg, seed=1).items()}}
    path = str(tmp_path / "msa_tiny.pt")
    torch.save(blob, path)
    m = models.ESM_MSA1(checkpoint=path, config=cfg)
    assert not m.model.has_row_contact_head
    with pytest.raises(RuntimeError, match=re.escape("msa_tiny-contact-regression.pt")):
        m.predict_row_contacts(np.zeros((1, 2, 5), np.int32))
    w, b = weights.synthetic_contact_head(cfg, 9)
    head = {"contact_head.regression.weight": torch.from_numpy(w[None]), "contact_head.regression.bias": torch.tensor([b])}
    torch.save({"model": head}, weights.contact_regression_path(path))
    m = models.ESM_MSA1(checkpoint=path, config=cfg)
    assert m.model.has_row_contact_head and np.array_equal(m.model._contact_head[0], w) and m.model._contact_head[1] == np.float32(b)
    own = str(tmp_path / "msa_own.pt")
    torch.save({"model": {**blob["model"], **head}}, own)
    m = models.ESM_MSA1(checkpoint=own, config=cfg)
    assert m.model.has_row_contact_head and np.array_equal(m.model._contact_head[0], w)
    odd = str(tmp_path / "msa_odd.pt")
    torch.save({"model": {**blob["model"], "contact_head.regression.weight": torch.zeros(1, 2 * n), "contact_head.regression.bias": torch.zeros(1)}}, odd)
    m = models.ESM_MSA1(checkpoint=odd, config=cfg)
    assert not m.model.has_row_contact_head
    with pytest.raises(RuntimeError, match=r"refused: .*shape \(1, %d\).*needs \(1, %d\)" % (2 * n, n)):
        m.predict_row_contacts(np.zeros((1, 2, 5), np.int32))


# ---- predict_contacts_batch against a recording stand-in -----------------------------------------------------------------------------------
H_FAKE = 4


def _standin():
    """fake_engine_model's MSA plug-in with a recording predict_row_contacts: entry (i, j) of MSA b holds (token_i of row 0) * 100 +
    (token_j of the last row), so a result says which alignment it came from"""
    plug = fake_engine_model(True)
    lm = plug.model
    lm.cfg = {"n_layers": 2, "n_heads": H_FAKE, "d_model": 8, "arch": _lib.PG_ARCH_MSA1B}

    def predict_row_contacts(tokens):
        tok = np.asarray(tokens)
        lm.trace.append(("predict_row_contacts", tok.copy()))
        return (tok[:, 0, 1:, None] * 100 + tok[:, -1, None, 1:]).astype(np.float32)
    lm.predict_row_contacts = predict_row_contacts
    return plug


@pytest.fixture
def gpu_named(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)


# shapes (R, L): (2, 7), (1, 3), (2, 7), (3, 7), (2, 7) -- three alignments of one shape, one of the same width but deeper
MSAS = [["ACDEFGH", "AC-EFGH"], ["MKV"], ["KLMNPQR", "KLMNPQW"], ["ACDEFGH", "ACDEFGY", "A-DEFGH"], ["WYVTSRQ", "WYVTS-Q"]]


@pytest.mark.parametrize("batch_size,cap,sizes", [
    (1, None, [1, 1, 1, 1, 1]), (2, None, [2, 1, 1, 1]), (None, None, [3, 1, 1]),
    (None, H_FAKE * 8 * 8 * 4 * 2, [2, 1, 1, 1]),          # the cap holds two maps of C = 8: the group of three is cut, as batch_size 2 cuts it
    (None, 1, [1, 1, 1, 1, 1]),                            # a cap below one map: one alignment still runs
    (2, H_FAKE * 8 * 8 * 4 * 3, [2, 1, 1, 1]),             # the smaller of the two limits
])
def test_predict_contacts_batch_groups_chunks_and_caps(gpu_named, batch_size, cap, sizes):
    plug = _standin()
    s = esm_msa_sampler.ESM_MSA_sampler(plug, device="gpu")
    out = list(s.predict_contacts_batch(MSAS, batch_size=batch_size, max_map_bytes=cap))
    lm = plug.model
    calls = [t for t in lm.trace if t[0] == "predict_row_contacts"]
    assert [c[1].shape[0] for c in calls] == sizes
    assert all((c[1] != plug.alphabet.padding_idx).all() for c in calls)              # one shape per call: an MSA is never padded
    assert all(c[1].shape[0] * H_FAKE * c[1].shape[2] ** 2 * 4 <= cap or c[1].shape[0] == 1 for c in calls if cap)
    assert lm.job_items == [3, 0, 1, 0, 1, 0]                                          # every group a job of its size, reset after it
    for msa, got in zip(MSAS, out):                                                    # input order, the columns only
        first = np.asarray([plug.alphabet.get_idx(c) for c in msa[0]])
        last = np.asarray([plug.alphabet.get_idx(c) for c in msa[-1]])
        assert got.dtype == np.float32 and np.array_equal(got, (first[:, None] * 100 + last[None, :]).astype(np.float32))
    assert np.array_equal(s.predict_contacts(MSAS[3]), out[3])


def test_predict_contacts_batch_refusals(gpu_named):
    s = esm_msa_sampler.ESM_MSA_sampler(_standin(), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        next(s.predict_contacts_batch(MSAS[:1]))
    s = esm_msa_sampler.ESM_MSA_sampler(_standin(), device="gpu")
    with pytest.raises(ValueError, match="max_map_bytes"):
        next(s.predict_contacts_batch(MSAS[:1], max_map_bytes=0))
    with pytest.raises(ValueError, match="alignment 1 is empty"):
        next(s.predict_contacts_batch([MSAS[0], []]))
    with pytest.raises(ValueError, match="rows of alignment 0 are not equally long"):
        next(s.predict_contacts_batch([["ACD", "AC"]]))


# ---- the front end ------------------------------------------------------------------------------------------------------------------------
def test_cli_parser():
    args = contacts_esm_msa.build_parser().parse_args(["-i", "a.fasta", "-o", "out"])
    assert (args.i, args.batch_size, args.precision, args.synthetic_weights, args.device) == (["a.fasta"], None, "auto", False, "gpu")
    args = contacts_esm_msa.build_parser().parse_args(["-i", "a.fa", "b.fa", "-o", "b", "--batch_size", "4", "--precision", "bf16",
                                                       "--synthetic-weights", "--device", "cuda:1"])
    assert (args.i, args.batch_size, args.precision, args.synthetic_weights, args.device) == (["a.fa", "b.fa"], 4, "bf16", True, "cuda:1")
    for bad in (["-o", "b"], ["-i", "a"], ["-i", "a", "-o", "b", "--model", "esm1b"]):
        with pytest.raises(SystemExit):
            contacts_esm_msa.build_parser().parse_args(bad)
    # the single-sequence front end keeps refusing the MSA model
    with pytest.raises(SystemExit):
        contacts_esm.build_parser().parse_args(["-i", "a", "-o", "b", "--model", "esm_msa1"])


def test_cli_writes_one_file_per_alignment(gpu_named, tmp_path):
    paths = []
    for i, msa in enumerate(MSAS[:4]):
        path = tmp_path / ("fam%d.a3m.fasta" % i)
        path.write_text("".join(">r%d\n%s\n" % (r, row.lower() if r else row) for r, row in enumerate(msa)))      # lower case -> upper
        paths.append(str(path))
    plug = _standin()
    s = esm_msa_sampler.ESM_MSA_sampler(plug, device="gpu")
    out = tmp_path / "out"
    files = contacts_esm_msa.main(paths, str(out), 2, s)
    assert files == ["fam%d.a3m.npz" % i for i in range(4)] and sorted(os.listdir(out)) == files
    want = list(s.predict_contacts_batch(MSAS[:4]))
    for name, msa, w in zip(files, MSAS, want):
        z = np.load(out / name)
        assert z.files == ["contacts"] and z["contacts"].dtype == np.float32 and z["contacts"].shape == (len(msa[0]),) * 2
        assert np.array_equal(z["contacts"], w)


def test_cli_refuses_unsafe_and_duplicate_names_before_anything_runs(gpu_named, tmp_path):
    plug = _standin()
    s = esm_msa_sampler.ESM_MSA_sampler(plug, device="gpu")
    good = tmp_path / "a.fasta"
    good.write_text(">q\nACD\n")
    (tmp_path / "sub").mkdir()
    twin = tmp_path / "sub" / "a.fa"
    twin.write_text(">q\nACD\n")
    odd = tmp_path / "b c.fasta"
    odd.write_text(">q\nACD\n")
    for paths, message in (([str(good), str(twin)], "already used"), ([str(good), str(odd)], "not a safe file name")):
        with pytest.raises(ValueError, match=message):
            contacts_esm_msa.main(paths, str(tmp_path / "out"), None, s)
    assert not (tmp_path / "out").exists() and not [t for t in plug.model.trace if t[0] == "predict_row_contacts"]
    ragged = tmp_path / "r.fasta"
    ragged.write_text(">q\nACD\n>r\nAC\n")
    with pytest.raises(ValueError, match="not an alignment"):
        contacts_esm_msa.main([str(ragged)], str(tmp_path / "out"), None, s)
    empty = tmp_path / "e.fasta"
    empty.write_text("")
    with pytest.raises(ValueError, match="no sequences"):
        contacts_esm_msa.main([str(empty)], str(tmp_path / "out"), None, s)
