"""Contact prediction without a GPU: the numpy references (tests/_contact_reference.py) against HuggingFace's recorded maps and against
each other, the contract's corner cases, the checkpoint readers of the regression head, every host refusal of the new C entries,
ESM_sampler.predict_contacts_batch's grouping and memory cap (against a recording stand-in for the engine), and the contacts_esm front
end."""
import ctypes
import io
import json
import os
import re

import numpy as np
import pytest
import torch

import _contact_reference as cr
import _esm2_reference as r2
from _fake_engine import fake_engine_model
from oracle import esm_forward as E
from protein_gibbs_sampler_amd import _lib, contacts_esm, esm_sampler, models, weights
from protein_gibbs_sampler_amd.engine import NativeMaskedLM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ENTRY = "pg_esm_forward_contacts"
U = 2.0 ** -24


# ---- the references ---------------------------------------------------------------------------------------------------------------------
def _hf_case(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    recipe = json.loads(str(z["cfg"]))
    kw = dict(seed=int(z["seed"]), std=float(z["std"]), embed_std=float(z["embed_std"]), ln_jitter=float(z["ln_jitter"]))
    if name == "esm2_hf_contacts":
        cfg = weights.make_config(weights.ESM2_T33_CONFIG, **recipe)
        sd = weights.synthetic_state_dict(cfg, **kw)
        return z, lambda t: cr.esm2_attentions(sd, r2.Esm2Config.of(cfg), t)
    ocfg = E.EsmConfig(**recipe)
    sd = E.synthetic_esm_weights(ocfg, **kw)
    return z, lambda t: cr.esm1b_attentions(sd, ocfg, t)


@pytest.mark.parametrize("name", ["esm_hf_contacts", "esm2_hf_contacts"])
def test_reference_against_the_huggingface_fixtures(name):
    """Attention rows below the generators' 2e-4; the contact probabilities of the live block within a quarter of the logit difference
    printed at record time (a logit error e moves a probability by at most e / 4) plus the fixture's float32 rounding."""
    z, attn = _hf_case(name)
    for tag in ("full", "ragged"):
        tok = z[tag + "_tokens"]
        A = attn(tok)
        assert A.dtype == np.float32 and A.shape[1:] == (tok.shape[0], 2, tok.shape[1], tok.shape[1])
        assert np.abs(A.reshape(-1, tok.shape[1])[z[tag + "_rows"]] - z[tag + "_attn_rows"]).max() < 2e-4
        assert not A[np.broadcast_to((tok == 1)[None, :, None, None, :], A.shape)].any()      # <pad> keys
        _, con = cr.contacts_from_attentions_f64(A, tok, z["head_w"], float(z["head_b"]), 2, 1)
        block = z[tag + "_live"]
        assert block.any() and np.array_equal(block, cr.live_window(tok, 2, 1)[:, :, None] & cr.live_window(tok, 2, 1)[:, None, :])
        assert np.abs(con - z[tag + "_contacts"])[block].max() < float(z[tag + "_logit_err"]) / 4 + 2.0 ** -23
        assert z[tag + "_contacts"][block].std() > 0.1                                         # not sigmoid(bias) everywhere


def fold_bound(A, tokens, w, bias, eos, pad):
    """|fp32 restatement - float64| per logit, from the fp32 contract (first order, 5 % for the rest): with e1 = (ceil(W / 64) + 7) u the
    relative error of a1 (one rounding of S, ceil(W / 64) adds in the lane, 6 across lanes) and e12 = e1 + (ceil(W / 64) + 6) u that
    of a12, the quotient q = a1[i] a1[j] / a12 carries 2 e1 + e12 + 2 u, N = S - q one rounding of S, of the subtraction and q's error,
    the product w N one more, and each of the C + 1 additions into the logit u of the running sum (<= sum_c |w N| + |bias|)."""
    A = np.asarray(A, dtype=np.float64)
    L, B, H, T, _ = A.shape
    W = T - 2
    live = cr.live_window(tokens, eos, pad)
    m = (live[:, :, None] & live[:, None, :])[None, :, None]
    win = np.where(m, A[:, :, :, 1:-1, 1:-1], 0.0)
    S = win + win.transpose(0, 1, 2, 4, 3)
    a1 = S.sum(-1)
    a12 = a1.sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(a12[..., None, None] == 0, 0.0, a1[..., :, None] * a1[..., None, :] / a12[..., None, None])
    N = S - q
    lane = -(-W // 64)
    e1 = (lane + 7) * U
    e12 = e1 + (lane + 6) * U
    wv = np.abs(np.asarray(w, dtype=np.float64)).reshape(L, 1, H, 1, 1)
    per = wv * (U * S + q * (2 * e1 + e12 + 3 * U) + 2 * U * np.abs(N))
    run = (wv * np.abs(N)).sum(axis=(0, 2)) + abs(bias)
    return 1.05 * (per.sum(axis=(0, 2)) + (L * H + 1) * U * run)


def _random_maps(rng, L, B, H, T):
    a = np.exp(3.0 * rng.standard_normal((L, B, H, T, T)))
    return (a / a.sum(-1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("T", [3, 8, 34, 131])
def test_the_two_forms_of_the_head_agree_under_the_derived_bound(T):
    rng = np.random.default_rng(T)
    L, B, H = 3, 2, 4
    A = _random_maps(rng, L, B, H, T)
    tok = np.full((B, T), 6)
    tok[:, 0], tok[:, -1] = 0, 2
    if T >= 8:
        tok[1, T - 4], tok[1, T - 3:] = 2, 1
    w = (5 * rng.standard_normal(L * H)).astype(np.float32)
    l64, c64 = cr.contacts_from_attentions_f64(A, tok, w, -0.3, 2, 1)
    l32 = cr.contacts_from_attentions_f32(A, tok, w, -0.3, 2, 1)
    assert l32.dtype == np.float32 and l32.shape == l64.shape == (B, T - 2, T - 2)
    bound = fold_bound(A, tok, w, -0.3, 2, 1)
    assert (np.abs(l32 - l64) <= bound).all(), float((np.abs(l32 - l64) / bound).max())
    assert bound.max() < 1e-3 * max(1.0, l64.std())                                             # and the bound says something
    assert np.array_equal(l32, l32.transpose(0, 2, 1))                                          # S is exactly symmetric, a1 one vector
    assert np.allclose(c64, 1 / (1 + np.exp(-l64)))


def test_wave_sum_is_the_documented_order():
    rng = np.random.default_rng(0)
    for n in (1, 5, 64, 65, 200):
        x = (rng.standard_normal(n) * 10).astype(np.float32)
        acc = np.zeros(64, np.float32)
        for k in range(n):
            acc[k % 64] = np.float32(acc[k % 64] + x[k])
        for off in (32, 16, 8, 4, 2, 1):
            acc = np.asarray([np.float32(acc[lane] + acc[lane ^ off]) for lane in range(64)], np.float32)
        assert len(set(acc.tolist())) == 1 and cr.wave_sum(x) == acc[0]
    assert cr.wave_sum(np.zeros((2, 3, 0), np.float32)).shape == (2, 3)


def test_contract_corner_cases():
    rng = np.random.default_rng(4)
    # T = 3: a window of one position: S = 2 A[1][1], a1 = a12 = S, N = S - S * S / S = 0: the logit is the bias
    A = _random_maps(rng, 2, 1, 2, 3)
    tok = np.asarray([[0, 9, 2]])
    w = np.asarray([1, -2, 3, 4], np.float32)
    l64, _ = cr.contacts_from_attentions_f64(A, tok, w, 0.25, 2, 1)
    l32 = cr.contacts_from_attentions_f32(A, tok, w, 0.25, 2, 1)
    assert l64.shape == (1, 1, 1) and abs(l64[0, 0, 0] - 0.25) < 1e-12 and abs(l32[0, 0, 0] - 0.25) < 1e-6
    # a <pad> tail (and the <eos> in front of it): its rows and columns are exactly the bias, the live block is what the sequence
    # alone gives when its maps are cut to its own length
    T, n = 12, 8
    A = _random_maps(rng, 2, 1, 2, T)
    A[..., n:] = 0
    A = (A / A.sum(-1, keepdims=True)).astype(np.float32)
    tok = np.full((1, T), 7)
    tok[0, 0], tok[0, n - 1], tok[0, n:] = 0, 2, 1
    l32 = cr.contacts_from_attentions_f32(A, tok, w, 0.25, 2, 1)
    l64, _ = cr.contacts_from_attentions_f64(A, tok, w, 0.25, 2, 1)
    live = cr.live_window(tok, 2, 1)[0]
    assert live.tolist() == [True] * (n - 2) + [False] * (T - n)
    assert (l32[0][~live] == np.float32(0.25)).all() and (l32[0][:, ~live] == np.float32(0.25)).all() and (l64[0][~live] == 0.25).all()
    alone, _ = cr.contacts_from_attentions_f64(A[:, :, :, :n, :n], tok[:, :n], w, 0.25, 2, 1)
    assert np.allclose(l64[0][:n - 2, :n - 2], alone[0], atol=1e-12)
    # a12 == 0: no live residue in the window -- every channel contributes 0 and nothing is NaN (fair-esm: 0 / 0)
    tok = np.asarray([[0, 2, 1, 1, 1]])
    A = _random_maps(rng, 2, 1, 2, 5)
    l64, c64 = cr.contacts_from_attentions_f64(A, tok, w, 0.25, 2, 1)
    l32 = cr.contacts_from_attentions_f32(A, tok, w, 0.25, 2, 1)
    assert (l64 == 0.25).all() and (l32 == np.float32(0.25)).all() and np.isfinite(c64).all()


def test_reference_maps_are_the_forwards_own_softmax():
    """rows sum to 1, <pad> keys are 0, and the ESM-2 maps applied to v reproduce tests/_esm2_reference.py's attention output"""
    cfg = weights.make_config(weights.ESM2_T33_CONFIG, d_model=128, n_layers=2, d_ffn=256, max_positions=64)
    sd = weights.synthetic_state_dict(cfg, seed=3, std=0.05, embed_std=0.3, ln_jitter=0.1)
    tok = np.concatenate([np.zeros((2, 1), np.int64), np.random.default_rng(1).integers(4, 24, (2, 11)), np.full((2, 1), 2)], axis=1)
    tok[1, 8], tok[1, 9:] = 2, 1
    A = cr.esm2_attentions(sd, r2.Esm2Config.of(cfg), tok)
    assert A.shape == (2, 2, 2, 13, 13) and np.abs(A.sum(-1) - 1).max() < 1e-6 and not A[:, 1, :, :, 9:].any()
    ocfg = E.EsmConfig(d_model=128, n_layers=2, n_heads=2, d_ffn=256, max_pos=64)
    sd1 = E.synthetic_esm_weights(ocfg, seed=3, std=0.05, embed_std=0.3, ln_jitter=0.1)
    A1 = cr.esm1b_attentions(sd1, ocfg, tok)
    assert A1.shape == A.shape and np.abs(A1.sum(-1) - 1).max() < 1e-6 and not A1[:, 1, :, :, 9:].any()


# ---- the regression head in checkpoints -------------------------------------------------------------------------------------------------
def _small_cfg():
    return weights.make_config(weights.ESM2_T33_CONFIG, d_model=128, n_layers=3, d_ffn=512, max_positions=64)


def test_contact_head_from_checkpoint_in_both_layouts(tmp_path):
    cfg = _small_cfg()
    n = cfg["n_layers"] * cfg["n_heads"]
    w, b = weights.synthetic_contact_head(cfg, seed=5)
    assert w.shape == (n,) and w.dtype == np.float32 and np.array_equal(w, weights.synthetic_contact_head(cfg, seed=5)[0])
    assert not np.array_equal(w, weights.synthetic_contact_head(cfg, seed=6)[0])
    head = {"contact_head.regression.weight": torch.from_numpy(w[None]), "contact_head.regression.bias": torch.tensor([b])}
    trunk = {"encoder.sentence_encoder.embed_tokens.weight": torch.zeros(33, 128)}
    # in the file itself, under fair-esm's prefixes
    for prefix in ("", "encoder.", "encoder.sentence_encoder.", "model."):
        path = str(tmp_path / ("own%d.pt" % len(prefix)))
        torch.save({"model": {**trunk, **{prefix + k: v for k, v in head.items()}}}, path)
        got = weights.contact_head_from_checkpoint(path, cfg)
        assert np.array_equal(got[0], w) and got[1] == np.float32(b)
    # in the sibling file, where fair-esm keeps it for ESM-1b / ESM-1v / ESM-2
    path = str(tmp_path / "esm2_t3_tiny.pt")
    torch.save({"model": trunk}, path)
    assert weights.contact_head_from_checkpoint(path, cfg) is None
    assert weights.contact_regression_path(path) == str(tmp_path / "esm2_t3_tiny-contact-regression.pt")
    torch.save({"model": head}, weights.contact_regression_path(path))
    got = weights.contact_head_from_checkpoint(path, cfg)
    assert np.array_equal(got[0], w) and got[1] == np.float32(b)
    # a head of another model: both shapes are named
    other = dict(cfg, n_layers=2)
    with pytest.raises(ValueError, match=r"shape \(1, %d\).*2 layers x %d heads needs \(1, %d\)" % (n, cfg["n_heads"], 2 * cfg["n_heads"])):
        weights.contact_head_from_checkpoint(path, other)
    torch.save({"model": {"contact_head.regression.weight": head["contact_head.regression.weight"]}}, weights.contact_regression_path(path))
    with pytest.raises(ValueError, match="without contact_head.regression.bias"):
        weights.contact_head_from_checkpoint(path, cfg)


def test_the_loader_still_ignores_the_head(tmp_path):
    """what load_fair_esm_checkpoint returns does not change: a v2 file with contact_head.* loads to the same tensors as one without"""
    cfg = _small_cfg()
    sd = weights.synthetic_state_dict(cfg, seed=2)
    blob = weights.to_fair_esm_checkpoint_v2(sd, cfg)
    plain = str(tmp_path / "plain.pt")
    torch.save(blob, plain)
    blob["model"]["encoder.sentence_encoder.contact_head.regression.weight"] = torch.zeros(1, cfg["n_layers"] * cfg["n_heads"])
    blob["model"]["encoder.sentence_encoder.contact_head.regression.bias"] = torch.zeros(1)
    with_head = str(tmp_path / "with_head.pt")
    torch.save(blob, with_head)
    a, b = weights.load_fair_esm_checkpoint(plain, cfg), weights.load_fair_esm_checkpoint(with_head, cfg)
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert weights.contact_head_from_checkpoint(plain, cfg) is None and weights.contact_head_from_checkpoint(with_head, cfg) is not None


def test_model_holders(tmp_path):
    cfg = _small_cfg()
    m = models.ESM2(config=cfg, synthetic=True, seed=4)
    assert m.model.has_contact_head and np.array_equal(m.model._contact_head[0], weights.synthetic_contact_head(cfg, 4)[0])
    with pytest.raises(RuntimeError, match="no CPU implementation"):          # the head is there; the engine is not on a GPU
        m.predict_contacts(np.zeros((1, 5), np.int32))
    # a checkpoint without a regression: the error says which files were looked in
    sd = weights.synthetic_state_dict(cfg, seed=2)
    path = str(tmp_path / "esm2_t3.pt")
    torch.save(weights.to_fair_esm_checkpoint_v2(sd, cfg), path)
    m = models.ESM2(checkpoint=path, config=cfg)
    assert not m.model.has_contact_head
    with pytest.raises(RuntimeError, match=re.escape("esm2_t3-contact-regression.pt")):
        m.predict_contacts(np.zeros((1, 5), np.int32))
    w, b = weights.synthetic_contact_head(cfg, 9)
    torch.save({"model": {"contact_head.regression.weight": torch.from_numpy(w[None]), "contact_head.regression.bias": torch.tensor([b])}},
               weights.contact_regression_path(path))
    m = models.ESM2(checkpoint=path, config=cfg)
    assert m.model.has_contact_head and np.array_equal(m.model._contact_head[0], w)
    # a regression that is not this model's (tests/test_gpu_checkpoint_and_bounds.py writes such a file): the model still loads, as it
    # always did, and predict_contacts says what was refused
    blob = weights.to_fair_esm_checkpoint_v2(sd, cfg)
    blob["model"]["encoder.sentence_encoder.contact_head.regression.weight"] = torch.zeros(1, 2 * cfg["n_layers"] * cfg["n_heads"])
    odd = str(tmp_path / "odd.pt")
    torch.save(blob, odd)
    m = models.ESM2(checkpoint=odd, config=cfg)
    assert not m.model.has_contact_head
    with pytest.raises(RuntimeError, match="refused: .*without contact_head.regression.bias"):
        m.predict_contacts(np.zeros((1, 5), np.int32))
    # ESM-1 and the MSA Transformer: NotImplementedError naming the model
    c1 = weights.make_config(weights.ESM1_T6_CONFIG, n_layers=2, d_model=128, d_ffn=256)
    with pytest.raises(NotImplementedError, match="ESM6"):
        models.ESM6(config=c1, synthetic=True).predict_contacts(np.zeros((1, 5), np.int32))
    cm = weights.make_config(weights.MSA1B_CONFIG, d_model=128, n_layers=2, n_heads=2, d_ffn=256, max_positions=64, max_msa_rows=16)
    msa = models.ESM_MSA1(config=cm, synthetic=True)
    with pytest.raises(NotImplementedError, match="ESM_MSA1"):
        msa.predict_contacts(np.zeros((1, 2, 5), np.int32))
    with pytest.raises(ValueError, match="MSA engine has no contact head"):
        msa.model.set_contact_head(np.zeros(4, np.float32), 0.0)


def test_engine_wrapper_checks_before_the_engine_is_asked_for():
    lm = NativeMaskedLM(_small_cfg(), {}, precision="bf16")
    n = lm.cfg["n_layers"] * lm.cfg["n_heads"]
    with pytest.raises(ValueError, match="%d weights for a model of 3 layers x %d heads = %d channels" % (n + 1, lm.cfg["n_heads"], n)):
        lm.set_contact_head(np.zeros(n + 1), 0.0)
    with pytest.raises(ValueError, match="finite"):
        lm.set_contact_head(np.full(n, np.nan), 0.0)
    tok = np.zeros((1, 5), np.int32)
    with pytest.raises(RuntimeError, match="no contact head set"):
        lm.predict_contacts(tok)
    lm.set_contact_head(np.ones(n), 0.5)                                        # kept on the host object until a handle exists
    assert lm.has_contact_head
    for bad, message in (([3], "outside"), ([-4], "outside"), ([0, -3], "twice"), ([1.5], "outside")):
        with pytest.raises(ValueError, match=message):
            lm.forward_attentions(tok, bad)
    with pytest.raises(ValueError, match="no attention layer"):
        lm.forward_attentions(tok, [])
    with pytest.raises(ValueError, match="T = 2"):
        lm.predict_contacts(np.zeros((1, 2), np.int32))
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        lm.predict_contacts(tok)
    lm.set_contact_head(None, 0.0)
    assert not lm.has_contact_head


# ---- the C entries ----------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "pgibbs.h")).read()
    bound = {n: a for n, _, a in _lib.SIGNATURES}
    for name, n_args in ((ENTRY, 9), ("pg_engine_set_contact_head", 4), ("pg_contact_dbg_probs", 12), ("pg_contact_dbg_accumulate", 14)):
        decl = re.search(r"PG_API int %s\(([^;]*)\);" % name, hdr)
        assert decl and len(decl.group(1).split(",")) == n_args == len(bound[name]), name
        assert hasattr(_lib.lib(), name)


def _refused(rc, message):
    assert rc == _lib.PG_ERR_INVALID
    assert message in _lib.lib().pg_last_error().decode(), _lib.lib().pg_last_error()


def _call(h=None, tok=True, B=2, T=5, contacts=True, logits=False, layers=None, n_attn=None, attn=False):
    tokens = np.full((2, 8), 5, np.int32)
    out = np.zeros(2 * 8 * 8, np.float32)
    big = np.zeros(4 * 2 * 4 * 64, np.float32)
    lay = np.asarray(layers, np.int32) if layers is not None else None
    return _lib.lib().pg_esm_forward_contacts(h, _lib.ptr(tokens) if tok else None, B, T, _lib.ptr(out) if contacts else None,
                                              _lib.ptr(out) if logits else None, _lib.ptr(lay) if lay is not None else None,
                                              (len(lay) if lay is not None else 0) if n_attn is None else n_attn, _lib.ptr(big) if attn else None)


def test_every_host_refusal_has_its_message_and_needs_no_device():
    """In the order pgibbs.h states, up to the null engine; the refusals that read the engine are in tests/test_gpu_contacts.py."""
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
    _refused(_call(T=2), "T = 2: a contact map needs <cls>, at least one position and <eos>")
    _refused(_call(T=2, layers=[0], attn=True, contacts=False), "T = 2")
    _refused(_call(), ENTRY + ": null engine")
    _refused(_call(layers=[0, 2], attn=True, contacts=False), ENTRY + ": null engine")
    w = np.zeros(4, np.float32)
    _refused(_lib.lib().pg_engine_set_contact_head(None, _lib.ptr(w), 4, 0.0), "pg_engine_set_contact_head: null engine")


def test_kernel_entries_refuse_on_the_host_and_report_the_plan_without_a_device():
    L = _lib.lib()
    qkv = np.zeros((2 * 5, 3 * 2 * 16), np.float32)
    out = np.zeros((2, 2, 5, 5), np.float32)
    plan = ctypes.create_string_buffer(128)

    def probs(precision=_lib.PG_PREC_BF16, q=qkv, n_seq=2, T=5, H=2, hd=16, o=out, pl=plan, nb=128):
        return L.pg_contact_dbg_probs(0, precision, _lib.ptr(q) if q is not None else None, n_seq, T, H, hd, None, 1,
                                      _lib.ptr(o) if o is not None else None, pl, nb)
    _refused(probs(precision=7), "unknown precision mode")
    _refused(probs(q=None), "pg_contact_dbg_probs: bad argument")
    _refused(probs(T=0), "pg_contact_dbg_probs: bad argument")
    _refused(probs(o=None, pl=None), "pg_contact_dbg_probs: bad argument")
    _refused(probs(hd=24), "head_dim must be")
    # the plan alone: no output buffer, no device -- two sweeps over 64-key tiles at every length
    for precision, T, want in ((_lib.PG_PREC_BF16, 5, "probs two-sweep t64 x1 hd16 4wg"), (_lib.PG_PREC_F16, 64, "probs two-sweep t64 x1 hd16 4wg"),
                               (_lib.PG_PREC_F16, 65, "probs two-sweep t64 x2 hd16 8wg"), (_lib.PG_PREC_FP32, 1024, "probs-f32 two-sweep t64 x16 hd16 64wg")):
        assert probs(precision=precision, T=T, o=None) == _lib.PG_OK and plan.value.decode() == want, plan.value
    P = np.zeros((1, 2, 5, 5), np.float32)
    tok = np.zeros((1, 5), np.int32)
    w = np.zeros(2, np.float32)
    lg = np.zeros((1, 3, 3), np.float32)

    def fold(P_=P, T=5, H=2, B=1, lg_=lg):
        return L.pg_contact_dbg_accumulate(0, _lib.ptr(P_) if P_ is not None else None, _lib.ptr(tok), 2, 1, _lib.ptr(w), 0.0, 1, 1,
                                           _lib.ptr(lg_) if lg_ is not None else None, None, B, T, H)
    _refused(fold(P_=None), "pg_contact_dbg_accumulate: bad argument")
    _refused(fold(lg_=None), "pg_contact_dbg_accumulate: bad argument")
    _refused(fold(H=0), "pg_contact_dbg_accumulate: bad argument")
    _refused(fold(T=2), "T must be at least 3")
    if L.pg_device_count() == 0:
        assert probs() == _lib.PG_ERR_NO_DEVICE and fold() == _lib.PG_ERR_NO_DEVICE


# ---- predict_contacts_batch against a recording stand-in -----------------------------------------------------------------------------------
H_FAKE = 4


def _standin():
    """fake_engine_model's plug-in with a recording predict_contacts: entry (i, j) of sequence b holds token_i * 100 + token_j"""
    plug = fake_engine_model(False)
    lm = plug.model
    lm.cfg = {"n_layers": 2, "n_heads": H_FAKE, "d_model": 8, "arch": _lib.PG_ARCH_ESM1B}

    def predict_contacts(tokens):
        tok = np.asarray(tokens)
        lm.trace.append(("predict_contacts", tok.copy()))
        res = tok[:, 1:-1]
        return (res[:, :, None] * 100 + res[:, None, :]).astype(np.float32)
    lm.predict_contacts = predict_contacts
    return plug


@pytest.fixture
def gpu_named(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)


SEQS = ["ACDEFGH", "M", "KLMNPQR", "ACDEFGHIKLMNPQRSTVWYACDEFGHIKL", "WYVTSRQ"]       # lengths 7, 1, 7, 30, 7


@pytest.mark.parametrize("batch_size,cap,sizes", [
    (1, None, [1, 1, 1, 1, 1]), (2, None, [2, 1, 1, 1]), (None, None, [3, 1, 1]),
    (None, H_FAKE * 9 * 9 * 4 * 2, [2, 1, 1, 1]),          # the cap holds two maps of T = 9: the group of three is cut, as batch_size 2 cuts it
    (None, 1, [1, 1, 1, 1, 1]),                            # a cap below one map: one sequence still runs
    (2, H_FAKE * 9 * 9 * 4 * 3, [2, 1, 1, 1]),             # the smaller of the two limits
])
def test_predict_contacts_batch_groups_chunks_and_caps(gpu_named, batch_size, cap, sizes):
    plug = _standin()
    s = esm_sampler.ESM_sampler(plug, device="gpu")
    out = list(s.predict_contacts_batch(SEQS, batch_size=batch_size, max_map_bytes=cap))
    lm = plug.model
    calls = [t for t in lm.trace if t[0] == "predict_contacts"]
    assert [c[1].shape[0] for c in calls] == sizes
    assert all((c[1] != plug.alphabet.padding_idx).all() for c in calls)              # equal lengths: no <pad> reaches the model
    assert all(c[1].shape[0] * H_FAKE * c[1].shape[1] ** 2 * 4 <= cap or c[1].shape[0] == 1 for c in calls if cap)
    assert lm.job_items == [3, 0, 1, 0, 1, 0]                                          # every group a job of its size, reset after it
    for seq, got in zip(SEQS, out):                                                    # input order, the residues only
        tok = np.asarray([plug.alphabet.get_idx(c) for c in seq])
        assert got.dtype == np.float32 and np.array_equal(got, (tok[:, None] * 100 + tok[None, :]).astype(np.float32))
    assert np.array_equal(s.predict_contacts("ACD"), out[0][:3, :3])


def test_predict_contacts_batch_refusals(gpu_named):
    s = esm_sampler.ESM_sampler(_standin(), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        next(s.predict_contacts_batch(["ACD"]))
    s = esm_sampler.ESM_sampler(_standin(), device="gpu")
    with pytest.raises(ValueError, match="max_map_bytes"):
        next(s.predict_contacts_batch(["ACD"], max_map_bytes=0))
    # embed_batch keeps refusing "contacts"
    with pytest.raises(ValueError, match="include"):
        next(s.embed_batch(["ACD"], include=("contacts",)))


# ---- the front end ------------------------------------------------------------------------------------------------------------------------
def test_cli_parser():
    args = contacts_esm.build_parser().parse_args(["-i", "in.fasta", "-o", "out"])
    assert (args.batch_size, args.model, args.precision, args.synthetic_weights) == (None, "esm1v", "auto", False)
    args = contacts_esm.build_parser().parse_args(["-i", "a", "-o", "b", "--model", "esm2_35m", "--batch_size", "4", "--precision", "bf16",
                                                   "--synthetic-weights"])
    assert (args.batch_size, args.model, args.precision, args.synthetic_weights) == (4, "esm2_35m", "bf16", True)
    for bad in (["-o", "b"], ["-i", "a", "-o", "b", "--model", "esm6"], ["-i", "a", "-o", "b", "--model", "esm_msa1"]):
        with pytest.raises(SystemExit):
            contacts_esm.build_parser().parse_args(bad)


def test_cli_writes_one_file_per_record(gpu_named, tmp_path):
    s = esm_sampler.ESM_sampler(_standin(), device="gpu")
    fasta = ">sp|P1|first protein\nACDEFGH\n>second\nM\n>third.v2\nKLM-NPQR*\n"
    files = contacts_esm.main(io.StringIO(fasta), str(tmp_path / "out"), 2, s)
    assert files == ["sp|P1|first.npz", "second.npz", "third.v2.npz"]
    want = list(s.predict_contacts_batch(["ACDEFGH", "M", "KLMNPQR"]))
    for name, res in zip(files, want):
        z = np.load(tmp_path / "out" / name)
        assert z.files == ["contacts"] and z["contacts"].dtype == np.float32 and np.array_equal(z["contacts"], res)
    # an unsafe or duplicate id is refused before anything runs or is written
    s.model.model.trace.clear()
    for bad in (">ok\nACD\n>a/b\nACD\n", ">a x\nACD\n>a y\nACD\n"):
        with pytest.raises(ValueError, match="safe file name|already used"):
            contacts_esm.main(io.StringIO(bad), str(tmp_path / "out2"), None, s)
    assert not (tmp_path / "out2").exists() and not s.model.model.trace
