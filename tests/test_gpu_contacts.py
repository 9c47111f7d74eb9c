"""Contact prediction on the GPU (pg_esm_forward_contacts, csrc/contact.hip): the two launchers alone through pg_contact_dbg_probs and
pg_contact_dbg_accumulate -- the probabilities against a float64 softmax of the same operands under a bound derived from the
roundings, the fold bit for bit against the fp32 restatement of its contract -- the engine's maps and contact logits against the
numpy references (tests/_contact_reference.py) and HuggingFace's recorded ones, and the structure of the call."""
import ctypes
import functools
import json
import os
import warnings

import numpy as np
import pytest

import _contact_reference as cr
import _esm2_gpu_common as C
from _esm2_sizes import SIZES
from oracle import esm_forward as E
from protein_gibbs_sampler_amd import _lib, esm_sampler, models, weights

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PRECISIONS = ["fp32", "bf16", "fp16"]
PREC = C.PREC
U = 2.0 ** -24          # unit roundoff of fp32
EPS = 2.0 ** -23        # spacing of fp32 in [1, 2)
TILE = 64               # keys per LDS tile of attn_probs_kernel


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ==== launch_attn_probs alone ==============================================================================================================
def _dbg_probs(precision, qkv, n_seq, T, H, hd, tok=None, pad_idx=1):
    out = np.full((n_seq, H, T, T), np.float32(np.nan))
    plan = ctypes.create_string_buffer(256)
    _lib.check(_lib.lib().pg_contact_dbg_probs(0, PREC[precision], _lib.ptr(qkv), n_seq, T, H, hd, _lib.ptr(tok) if tok is not None else None,
                                               pad_idx, _lib.ptr(out), plan, 256))
    return out, plan.value.decode()


def _qkv(rng, n_seq, T, H, hd):
    """q (already scaled) and k ~ N(0, 3 / sqrt(hd)): scores q . k of standard deviation about 3 -- peaked rows, not uniform ones"""
    sigma = (3.0 / np.sqrt(hd)) ** 0.5
    return (sigma * rng.standard_normal((n_seq * T, 3 * H * hd))).astype(np.float32)


def _operands(precision, qkv):
    """what the kernel multiplies: the 16-bit rounding of the mode (strict: the fp32 values themselves)"""
    return {"fp32": lambda x: x, "bf16": cr.round_bf16, "fp16": cr.round_f16}[precision](qkv)


def probs_bound(precision, hd, T, P, s, mag, pad):
    """The bound on |kernel - float64 softmax of the same operands| per entry, first order in the roundings with 5 % for the rest, not
    fitted (u = 2^-24; L = log2 e; m = the row's maximum; mag_j = sum_d |q_d k_d|):
      * the score: 16-bit modes -- products of two 16-bit values are exact in fp32 and the MFMAs add hd of them in fp32: |ds_j| <= hd u
        mag_j.  Strict -- x = hi + lo + r with |r| <= 2^-18 |x| (two bf16 roundings), the kernel adds qh.kl + ql.kh + qh.kh: the
        dropped ql.kl, r_q.k and q.r_k are each <= 2^-18 |q||k| (3.1 with the cross terms), and 3 hd additions: |ds_j| <= (3.1 * 2^-18
        + 3 hd u) mag_j.  An error ds of a score is a relative error ds of its exponential.
      * x - max and exp: the exponent fma(s, L, -m L) carries the rounding of L and of -m L (|s - m| u and |m| u after the factor
        ln 2 / L... in relative terms of the exponential) and its own (|s - m| u); v_exp_f32 is good to 1 ulp = 2 u:
        rho_j = ds_j + (2 |s_j - m| + |m| + 2) u.
      * the sum: the denominator is a p-weighted mean of the numerators' errors (<= max_j rho_j over the row's live keys), plus 16
        adds in the lane and 2 across lanes per tile, plus per tile the online rescale l * alpha + psum (alpha = exp2 of a rounded
        difference of at most R = max s - min s: (R + 2) u, one multiply, one add): (18 + n_tiles (R + 5)) u.
      * one division and one multiplication: 2 u.
    |dp_j| <= 1.05 p_j (rho_j + max rho + (20 + n_tiles (R + 5)) u) + 1e-37 (an exponential that v_exp_f32 flushes to zero)."""
    ds = (hd * U if precision != "fp32" else 3.1 * 2.0 ** -18 + 3 * hd * U) * mag
    live = np.ones_like(s, dtype=bool) if pad is None else np.broadcast_to(~np.asarray(pad, bool)[:, None, None, :], s.shape)
    sm = np.where(live, s, -np.inf)
    m = sm.max(axis=-1, keepdims=True)
    R = m - np.where(live, s, np.inf).min(axis=-1, keepdims=True)
    rho = np.where(live, ds + (2 * np.abs(s - m) + np.abs(m) + 2) * U, 0.0)
    n_tiles = (T + TILE - 1) // TILE
    return 1.05 * P * (rho + rho.max(axis=-1, keepdims=True) + (20 + n_tiles * (R + 5)) * U) + 1e-37


# T: 3, 8, 17, 34, 130 and both sides of what depends on T in the kernel -- the tile count (64 | 65, 128 | 129 <= 130) and the 16-byte
# stores of rows whose length is a multiple of 4 (8, 64, 128 against the rest)
PROBS_T = [3, 8, 17, 34, 64, 65, 128, 130]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("hd", [16, 32, 64, 128])
def test_probabilities_against_the_float64_softmax_of_the_same_operands(hd, precision):
    H, n_seq = 2, 3
    rng = np.random.default_rng(1000 + hd)
    worst = 0.0
    for T in PROBS_T:
        qkv = _qkv(rng, n_seq, T, H, hd)
        ops = _operands(precision, qkv)
        want, s, mag = cr.softmax_probs_f64(ops, n_seq, T, H, hd)
        if s.size >= 1000:
            assert 2.0 < s.std() < 4.0, (T, s.std())                     # peaked rows: the reference's own scores
        got, plan = _dbg_probs(precision, qkv, n_seq, T, H, hd)
        assert plan.startswith("probs-f32" if precision == "fp32" else "probs ") and "x%d hd%d" % ((T + TILE - 1) // TILE, hd) in plan, plan
        bound = probs_bound(precision, hd, T, want, s, mag, None)
        ratio = float((np.abs(got - want) / bound).max())
        worst = max(worst, ratio)
        assert ratio < 1.0, (T, ratio, float(np.abs(got - want).max()))
        # rows sum to 1 within n eps: n - 1 additions of the lane sums, a division and a multiplication, each half an eps at most
        assert np.abs(got.astype(np.float64).sum(axis=-1) - 1.0).max() < T * EPS, T
        # each sequence alone: the bits it has in the batch
        for b in range(n_seq):
            alone, _ = _dbg_probs(precision, np.ascontiguousarray(qkv[b * T:(b + 1) * T]), 1, T, H, hd)
            assert np.array_equal(_bits(alone[0]), _bits(got[b])), (T, b)
    print("\n[attn_probs hd%d %s] worst |kernel - float64| / derived bound = %.3g" % (hd, precision, worst))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("hd", [16, 32, 64, 128])
def test_probabilities_with_pad_keys(hd, precision):
    """rows of 40, 23 and 9 tokens in T = 40: entries at <pad> keys are exactly 0, the live ones within the bound, rows sum to 1"""
    H, n_seq, T = 2, 3, 40
    rng = np.random.default_rng(2000 + hd)
    qkv = _qkv(rng, n_seq, T, H, hd)
    tok = np.full((n_seq, T), 5, np.int32)
    for b, n in enumerate((40, 23, 9)):
        tok[b, n:] = 1
    pad = tok == 1
    want, s, mag = cr.softmax_probs_f64(_operands(precision, qkv), n_seq, T, H, hd, pad)
    got, plan = _dbg_probs(precision, qkv, n_seq, T, H, hd, tok)
    assert " pad " in plan
    assert not got[np.broadcast_to(pad[:, None, None, :], got.shape)].any()
    assert (np.abs(got - want) / probs_bound(precision, hd, T, want, s, mag, pad)).max() < 1.0
    assert np.abs(got.astype(np.float64).sum(axis=-1) - 1.0).max() < T * EPS
    for b in range(n_seq):
        alone, _ = _dbg_probs(precision, np.ascontiguousarray(qkv[b * T:(b + 1) * T]), 1, T, H, hd, np.ascontiguousarray(tok[b:b + 1]))
        assert np.array_equal(_bits(alone[0]), _bits(got[b])), b


# ==== launch_contact_accumulate alone =========================================================================================================
def _dbg_fold(P, tok, w, bias, first, last, logits, want_contacts=False, eos=2, pad=1):
    B, H, T, _ = P.shape
    lg = np.ascontiguousarray(logits, dtype=np.float32).copy() if logits is not None else np.full((B, T - 2, T - 2), np.float32(np.nan))
    con = np.full((B, T - 2, T - 2), np.float32(np.nan)) if want_contacts else None
    _lib.check(_lib.lib().pg_contact_dbg_accumulate(0, _lib.ptr(np.ascontiguousarray(P, dtype=np.float32)), _lib.ptr(np.ascontiguousarray(tok, dtype=np.int32)),
                                                    eos, pad, _lib.ptr(np.ascontiguousarray(w, dtype=np.float32)), float(bias), int(first), int(last),
                                                    _lib.ptr(lg), _lib.ptr(con) if want_contacts else None, B, T, H))
    return lg, con


def _maps(rng, B, H, T):
    """seeded non-negative rows that sum to 1, peaked like attention rows"""
    a = np.exp(3.0 * rng.standard_normal((B, H, T, T)))
    return (a / a.sum(axis=-1, keepdims=True)).astype(np.float32)


def _fold_tokens(B, T):
    """sequence 0 full; sequence 1 (when there is room) with an <eos> and a <pad> tail inside the window"""
    tok = np.full((B, T), 7, np.int32)
    tok[:, 0], tok[:, -1] = 0, 2
    if B > 1 and T >= 6:
        n = T - max(2, T // 4)
        tok[1, n - 1], tok[1, n:] = 2, 1
    return tok


@pytest.mark.parametrize("H", [1, 2, 20])
@pytest.mark.parametrize("W", [1, 6, 32, 128])
def test_fold_bit_for_bit_against_the_fp32_restatement(W, H):
    """Two layers folded in turn; the contract pins the reduction order (csrc/contact.hip), so the logits are compared bit for bit.
    Not-live rows and columns end at exactly the bias; the contact probabilities are the float64 sigmoid within 4 eps."""
    B, T, bias = 2, W + 2, -0.75
    rng = np.random.default_rng(100 * W + H)
    tok = _fold_tokens(B, T)
    w = rng.standard_normal((2, H)).astype(np.float32) * 5
    P0, P1 = _maps(rng, B, H, T), _maps(rng, B, H, T)
    l0, _ = _dbg_fold(P0, tok, w[0], bias, True, False, None)
    want0 = cr.fold_layer_f32(P0, tok, w[0], bias, True, False, None, 2, 1)
    assert np.array_equal(_bits(l0), _bits(want0))
    l1, con = _dbg_fold(P1, tok, w[1], bias, False, True, l0, want_contacts=True)
    want1 = cr.fold_layer_f32(P1, tok, w[1], bias, False, True, want0, 2, 1)
    assert np.array_equal(_bits(l1), _bits(want1))
    live = cr.live_window(tok, 2, 1)
    dead = ~(live[:, :, None] & live[:, None, :])
    assert np.array_equal(_bits(l1[dead]), _bits(np.full(int(dead.sum()), np.float32(bias))))
    if W >= 6:
        assert dead[1].any() and not dead[0].any() and l1[~dead].std() > 0.1
    assert np.abs(con - 1.0 / (1.0 + np.exp(-l1.astype(np.float64)))).max() < 4 * EPS
    # the float64 form of the same contract: the fp32 order costs at most a few hundred roundings of terms of size |w| S
    l64, _ = cr.contacts_from_attentions_f64(np.stack([P0, P1]), tok, w.reshape(-1), bias, 2, 1)
    assert np.abs(l1 - l64).max() < 1e-4 * max(1.0, float(np.abs(l64).max()))


def test_fold_one_hot_weights_pick_their_channel():
    """2 layers x 2 heads, one weight 1 and the rest 0, bias 0: the logits are that channel's APC alone (float64 reference of that
    channel) and none of the other three"""
    B, H, T = 2, 2, 19
    rng = np.random.default_rng(9)
    tok = _fold_tokens(B, T)
    A = np.stack([_maps(rng, B, H, T), _maps(rng, B, H, T)])
    apc = {}
    for l in range(2):
        for h in range(2):
            apc[l, h] = cr.contacts_from_attentions_f64(A[l:l + 1, :, h:h + 1], tok, [1.0], 0.0, 2, 1)[0]
    for c in range(4):
        w = np.zeros((2, H), np.float32)
        w.reshape(-1)[c] = 1
        lg, _ = _dbg_fold(A[0], tok, w[0], 0.0, True, False, None)
        lg, _ = _dbg_fold(A[1], tok, w[1], 0.0, False, True, lg)
        errs = {k: float(np.abs(lg - v).max()) for k, v in apc.items()}
        assert errs[c // H, c % H] < 1e-6 and all(e > 1e-3 for k, e in errs.items() if k != (c // H, c % H)), (c, errs)


# ==== the engine against the references ====================================================================================================
BATCHES = [(1, 8), (3, 27), (3, 34), (2, 130)]
FAMILIES = ["esm1b", "esm2", "esm2_8m", "esm2_150m", "esm2_15b", "esm2_35m"]      # heads of 64, 64, 16, 32, 128 and embedded 24
# max |engine - reference| over every model and batch below, per precision mode, against tests/_contact_reference.py (never against a
# rerun of the engine): attention maps absolute, contact logits per standard deviation of the reference's logits over the window.  The
# first measured run on an MI355X; the tests hold 2.5 x these (box-to-box and batch variation of the 16-bit roundings).
# Measured, maps: 9.15e-6 (strict; worst: ESM-1b 3 x 1024, (3, 27)), 4.99e-3 (bf16; ESM-1b, ragged), 7.40e-4 (fp16; ESM-1b, (1, 8));
# logits: 1.97e-4 (strict; ESM-2 heads of 128, ragged), 7.63e-2 (bf16; ESM-2 heads of 24, ragged), 8.77e-3 (fp16; heads of 128, ragged)
ATTN_MEASURED = {"fp32": 9.2e-6, "bf16": 5.0e-3, "fp16": 7.4e-4}
LOGIT_MEASURED = {"fp32": 2.0e-4, "bf16": 7.7e-2, "fp16": 8.8e-3}
ATTN_BOUND = {p: 2.5 * v for p, v in ATTN_MEASURED.items()}
LOGIT_BOUND = {p: 2.5 * v for p, v in LOGIT_MEASURED.items()}


@functools.lru_cache(maxsize=None)
def _family(name):
    if name == "esm1b":      # 3 x 1024: a width the persistent single-chain launch takes at (1, 8)
        cfg = weights.make_config(weights.ESM1B_CONFIG, d_model=1024, n_layers=3, n_heads=16, d_ffn=4096, max_positions=160)
        sd = weights.synthetic_state_dict(cfg, seed=5, std=0.03, embed_std=0.3, ln_jitter=0.1)
        ocfg = E.EsmConfig(d_model=1024, n_layers=3, n_heads=16, d_ffn=4096, max_pos=160)
        return dict(cfg=cfg, sd=sd, wrapper=models.ESM1b, attn=lambda t: cr.esm1b_attentions(sd, ocfg, t))
    over = {"esm2": dict(n_layers=3, d=256), "esm2_150m": dict(n_layers=3, d=256), "esm2_8m": dict(n_layers=3), "esm2_15b": dict(n_layers=3),
            "esm2_35m": dict(n_layers=3, d=480)}[name]
    cfg, sd, rcfg = C.case(name, **over)
    sd = dict(sd)
    return dict(cfg=cfg, sd=sd, wrapper=SIZES[name]["wrapper"], attn=lambda t: cr.esm2_attentions(sd, rcfg, t))


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The token batches of a family (the last one ragged: rows of 40, 23 and 9 right-padded to 40), the reference's maps on them and
    its contact logits under the family's head: a seeded N(0, 1) regression scaled so that the reference logits of the flattest batch
    have a standard deviation of 1.2 over the window's live block (the long batches' maps are nearly uniform and their APC small) --
    without that every output is sigmoid(bias).  Computed once, never changed."""
    f = _family(name)
    n, H = f["cfg"]["n_layers"], f["cfg"]["n_heads"]
    rng = np.random.default_rng(5)
    toks = [C.tokens(rng, B, T) for B, T in BATCHES]
    tok = np.full((3, 40), 1, dtype=np.int64)
    for b, ln in enumerate((40, 23, 9)):
        tok[b, :ln] = C.tokens(rng, 1, ln, mask_every=5)[0]
    toks.append(tok)
    maps = [f["attn"](t) for t in toks]
    w = np.random.default_rng(77).standard_normal(n * H)
    blocks = [cr.live_window(t, 2, 1)[:, :, None] & cr.live_window(t, 2, 1)[:, None, :] for t in toks]
    unit = [cr.contacts_from_attentions_f64(A, t, w, 0.0, 2, 1)[0][blk].std() for t, A, blk in zip(toks, maps, blocks)]
    w = (w * 1.2 / min(unit)).astype(np.float32)
    bias = -0.5
    out = []
    for t, A in zip(toks, maps):
        lg, _ = cr.contacts_from_attentions_f64(A, t, w, bias, 2, 1)
        live = cr.live_window(t, 2, 1)
        block = live[:, :, None] & live[:, None, :]
        A.setflags(write=False)
        out.append((t, A, lg, block))
    assert all(lg[block].std() >= 1.0 for _, _, lg, block in out), [lg[block].std() for _, _, lg, block in out]
    return w, bias, out


def _lm(name, precision, head=True):
    f = _family(name)
    lm = C.model(f["wrapper"], f["cfg"], f["sd"], precision).model.to("cuda:0")
    if head:
        w, bias, _ = _reference(name)
        lm.set_contact_head(w, bias)
    return lm


@functools.lru_cache(maxsize=None)
def _measure(name, precision):
    f = _family(name)
    n = f["cfg"]["n_layers"]
    lm = _lm(name, precision)
    w, bias, ref = _reference(name)
    fig = dict(attn=[], logit=[], sq=0.0, count=0, pad_zero=True, dead_bias=True, sig=0.0)
    for tok, A, lg, block in ref:
        B, T = tok.shape
        con, got_lg, att = lm.forward_contacts(tok, contacts=True, logits=True, attn_layers=range(n))
        assert att.shape == A.shape and got_lg.shape == lg.shape == con.shape and att.dtype == got_lg.dtype == con.dtype == np.float32
        real_q = (tok != 1)[None, :, None, :, None]
        fig["attn"].append(float(np.abs(np.where(real_q, att - A, 0)).max()))
        fig["pad_zero"] &= not att[np.broadcast_to((tok == 1)[None, :, None, None, :], att.shape)].any()
        std = float(lg[block].std())
        fig["logit"].append(float(np.abs(got_lg - lg)[block].max() / std))
        fig["dead_bias"] &= bool(np.array_equal(_bits(got_lg[~block]), _bits(np.full(int((~block).sum()), np.float32(bias)))))
        fig["sq"] += float(np.sum(np.square((got_lg - lg)[block] / std, dtype=np.float64)))
        fig["count"] += int(block.sum())
        fig["sig"] = max(fig["sig"], float(np.abs(con - 1.0 / (1.0 + np.exp(-got_lg.astype(np.float64)))).max()))
    fig["rms"] = (fig["sq"] / fig["count"]) ** 0.5
    print("\n[contacts %s %s] max|attention - reference| per batch %s; max|logit - reference| / logit std per batch %s; rms %.3e"
          % (name, precision, ["%.3g" % v for v in fig["attn"]], ["%.3g" % v for v in fig["logit"]], fig["rms"]))
    return fig


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", FAMILIES)
def test_maps_and_logits_against_the_reference(name, precision):
    """Every batch of BATCHES and the right-padded ragged batch: all layers' maps and the contact logits within 2.5 x the first
    measured worst case of the mode; <pad> key columns exactly 0; not-live window entries exactly the bias; contacts = sigmoid."""
    fig = _measure(name, precision)
    assert fig["pad_zero"] and fig["dead_bias"] and fig["sig"] < 4 * EPS
    assert max(fig["attn"]) < ATTN_BOUND[precision], fig["attn"]
    assert max(fig["logit"]) < LOGIT_BOUND[precision], fig["logit"]


@pytest.mark.parametrize("name", FAMILIES)
def test_logits_are_nearer_the_reference_in_the_finer_modes(name):
    errs = [_measure(name, p)["rms"] for p in ("fp32", "fp16", "bf16")]
    assert errs[0] < errs[1] < errs[2], errs


@pytest.mark.parametrize("name", ["esm_hf_contacts", "esm2_hf_contacts"])
def test_huggingface_contacts_and_attentions_strict(name):
    """HuggingFace's predict_contacts and output_attentions on 3 x 128 (tests/golden/make_golden_contacts.py), the full and the ragged
    batch, in strict mode: the recorded attention rows within the strict map bound, the contact probabilities of the live block within
    the strict logit bound (a logit error e moves a probability by at most e / 4), each plus what the numpy reference itself differed
    from HuggingFace by at record time."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    recipe = json.loads(str(z["cfg"]))
    kw = dict(seed=int(z["seed"]), std=float(z["std"]), embed_std=float(z["embed_std"]), ln_jitter=float(z["ln_jitter"]))
    if name == "esm2_hf_contacts":
        cfg = weights.make_config(weights.ESM2_T33_CONFIG, **recipe)
        sd, wrapper = weights.synthetic_state_dict(cfg, **kw), models.ESM2
    else:
        cfg = weights.make_config(weights.ESM1B_CONFIG, d_model=recipe["d_model"], n_layers=recipe["n_layers"], d_ffn=recipe["d_ffn"],
                                  max_positions=recipe["max_pos"])
        sd, wrapper = E.synthetic_esm_weights(E.EsmConfig(**recipe), **kw), models.ESM1b
    lm = C.model(wrapper, cfg, sd, "fp32").model.to("cuda:0")
    lm.set_contact_head(z["head_w"], float(z["head_b"]))
    n = cfg["n_layers"]
    for tag in ("full", "ragged"):
        tok = z[tag + "_tokens"]
        con, lg, att = lm.forward_contacts(tok, contacts=True, logits=True, attn_layers=range(n))
        rows = att.reshape(-1, tok.shape[1])[z[tag + "_rows"]]
        a_err = float(np.abs(rows - z[tag + "_attn_rows"]).max())
        block = z[tag + "_live"]
        c_err = float(np.abs(con - z[tag + "_contacts"])[block].max())
        std = float(lg[block].std())
        print("\n[%s %s strict] max|attention - HF| = %.3e, max|contact - HF| over the live block = %.3e (logit std %.2f)" % (name, tag, a_err, c_err, std))
        assert a_err < ATTN_BOUND["fp32"] + float(z[tag + "_attn_err"])
        assert c_err < (LOGIT_BOUND["fp32"] * std + float(z[tag + "_logit_err"])) / 4


# ==== structure ==============================================================================================================================
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_single_chain_equals_itself_inside_a_batch(precision):
    """(1, 8) -- the shape the persistent single-chain launch would take on ESM-1b; a contacts call never takes it -- against the same
    sequence inside a (3, 8) batch: bit for bit, maps and logits; and the calls around it are not changed by it."""
    lm = _lm("esm1b", precision)
    n = lm.cfg["n_layers"]
    tok3 = C.tokens(np.random.default_rng(3), 3, 8)
    before = lm.forward_logits(tok3[1:2])
    con3, lg3, att3 = lm.forward_contacts(tok3, logits=True, attn_layers=range(n))
    con1, lg1, att1 = lm.forward_contacts(tok3[1:2], logits=True, attn_layers=range(n))
    assert np.array_equal(_bits(lg1[0]), _bits(lg3[1])) and np.array_equal(_bits(con1[0]), _bits(con3[1]))
    assert np.array_equal(_bits(att1[:, 0]), _bits(att3[:, 1]))
    # maps alone need no head and are the maps of the full call; a subset in the caller's order; fair-esm's call shape
    bare = _lm("esm1b", precision, head=False)
    only = bare.forward_attentions(tok3, [-1, 0])
    assert np.array_equal(_bits(only[0]), _bits(att3[n - 1])) and np.array_equal(_bits(only[1]), _bits(att3[0]))
    with pytest.raises(RuntimeError, match="no contact head"):
        bare.predict_contacts(tok3)
    out = lm(tok3, return_contacts=True, need_head_weights=True)
    assert sorted(out) == ["attentions", "contacts", "logits"] and tuple(out["attentions"].shape) == (3, n, lm.cfg["n_heads"], 8, 8)
    assert np.array_equal(_bits(out["contacts"].numpy()), _bits(con3)) and np.array_equal(_bits(out["attentions"].numpy()[:, 1]), _bits(att3[1]))
    assert np.array_equal(_bits(lm.forward_logits(tok3[1:2])), _bits(before))
    # the two profiling classes hold this call's launches and nothing of a logits call
    lm.prof_enable(True)
    lm.prof_reset()
    lm.forward_logits(tok3)
    assert lm.prof_get("attn_probs")[1] == 0 and lm.prof_get("contact")[1] == 0
    lm.predict_contacts(tok3)
    assert lm.prof_get("attn_probs")[1] == n and lm.prof_get("contact")[1] == n
    lm.prof_enable(False)


def test_engine_refusals_that_need_an_engine():
    L = _lib.lib()
    lm = _lm("esm2", "bf16", head=False)
    tok = C.tokens(np.random.default_rng(0), 2, 9).astype(np.int32)
    out = np.zeros((2, 7, 7), np.float32)
    att = np.zeros((1, 2, lm.cfg["n_heads"], 9, 9), np.float32)
    lay = np.asarray([3], np.int32)
    assert L.pg_esm_forward_contacts(lm.handle, _lib.ptr(tok), 2, 9, _lib.ptr(out), None, None, 0, None) == _lib.PG_ERR_INVALID
    assert "no contact head set" in L.pg_last_error().decode()
    assert L.pg_esm_forward_contacts(lm.handle, _lib.ptr(tok), 2, 9, None, None, _lib.ptr(lay), 1, _lib.ptr(att)) == _lib.PG_ERR_INVALID
    assert "attention layer 3 is outside 0 .. 2" in L.pg_last_error().decode()
    w = np.zeros(5, np.float32)
    assert L.pg_engine_set_contact_head(lm.handle, _lib.ptr(w), 5, 0.0) == _lib.PG_ERR_INVALID
    assert "5 weights for a model of 3 layers x 4 heads = 12 channels" in L.pg_last_error().decode()
    w = np.zeros(12, np.float32)
    w[7] = np.inf
    assert L.pg_engine_set_contact_head(lm.handle, _lib.ptr(w), 12, 0.0) == _lib.PG_ERR_INVALID
    assert "weight 7 is not finite" in L.pg_last_error().decode()
    w[7] = 1
    assert L.pg_engine_set_contact_head(lm.handle, _lib.ptr(w), 12, 0.0) == _lib.PG_OK
    bad = tok.copy()
    bad[1, 3] = 35
    assert L.pg_esm_forward_contacts(lm.handle, _lib.ptr(bad), 2, 9, _lib.ptr(out), None, None, 0, None) == _lib.PG_ERR_INVALID
    assert "token 35 at flat index 12" in L.pg_last_error().decode()
    assert L.pg_esm_forward_contacts(lm.handle, _lib.ptr(tok), 2, 9, _lib.ptr(out), None, None, 0, None) == _lib.PG_OK
    assert L.pg_engine_set_contact_head(lm.handle, None, 0, 0.0) == _lib.PG_OK
    assert L.pg_esm_forward_contacts(lm.handle, _lib.ptr(tok), 2, 9, _lib.ptr(out), None, None, 0, None) == _lib.PG_ERR_INVALID
    # the architectures without the entry, by name
    cfg1 = weights.make_config(weights.ESM1_T6_CONFIG, n_layers=2, d_model=128, d_ffn=256)
    esm1 = C.model(models.ESM6, cfg1, weights.synthetic_state_dict(cfg1, seed=7), "bf16").model.to("cuda:0")
    assert L.pg_esm_forward_contacts(esm1.handle, _lib.ptr(tok), 2, 9, _lib.ptr(out), None, None, 0, None) == _lib.PG_ERR_INVALID
    assert "the ESM-1 architecture has no contact head" in L.pg_last_error().decode()
    assert L.pg_engine_set_contact_head(esm1.handle, _lib.ptr(w), 12, 0.0) == _lib.PG_ERR_INVALID
    assert "ESM-1" in L.pg_last_error().decode()


def test_generate_is_unchanged_by_a_contacts_call_in_between():
    """A seeded 12-iteration single-chain generate (the hipGraph path) twice on one engine, with and without a contacts call between
    the two runs: the same tokens."""
    cfg, sd, _ = C.case("esm2", n_layers=3, d=256, seed=13)
    outs = {}
    for between in (False, True):
        s, first = C.single_chain_run(C.size_model("esm2", cfg, sd, "bf16"))
        lm = s.model.model
        if between:
            lm.set_contact_head(*weights.synthetic_contact_head(cfg, seed=1))
            con = lm.predict_contacts(C.tokens(np.random.default_rng(2), 3, 27))
            assert np.isfinite(con).all()
        outs[between] = (first, C.single_chain_generate(s, False))
        assert lm.get_stat("graph_replays") > 0
    assert outs[True] == outs[False] and outs[True][0] == outs[True][1]


def test_auto_precision_falls_back_to_bf16_on_a_forced_overflow(monkeypatch):
    """tests/test_gpu_representations.py's recipe: fc1 weights of block 2 that fit fp16 but drive GELU(fc1) past 65504, the probe off.
    Block 3's qkv is then not finite in the fp16 engine, the entry answers PG_ERR_RANGE and the wrapper runs the call on the bf16
    engine -- which carries the head too."""
    monkeypatch.setenv("PGIBBS_F16_PROBE", "0")
    cfg = weights.make_config(weights.ESM1B_CONFIG, d_model=256, n_layers=3, d_ffn=512, max_positions=128)
    sd = {k: v.copy() for k, v in weights.synthetic_state_dict(cfg, seed=21, std=0.05, embed_std=0.3, ln_jitter=0.1).items()}
    sd["layers.1.fc1.weight"] *= np.float32(1e5)
    assert np.abs(sd["layers.1.fc1.weight"]).max() < 65504
    tok = C.tokens(np.random.default_rng(2), 3, 42)
    head = weights.synthetic_contact_head(cfg, seed=3, std=20.0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        lm = models.ESM1b(state_dict=sd, config=cfg).model.to("cuda:0")
        lm.set_contact_head(*head)
        early = lm.forward_attentions(tok, [0, 1])                             # below the overflow: fp16 values, no fallback
    assert lm.precision_name == "fp16" and lm.fallbacks == 0 and np.isfinite(early).all()
    with pytest.warns(UserWarning, match="run again with bf16 operands"):
        con, lg, _ = lm.forward_contacts(tok, logits=True)
    assert lm.fallbacks == 1 and np.isfinite(con).all() and np.isfinite(lg).all()
    bf = models.ESM1b(state_dict=sd, config=cfg, precision="bf16").model.to("cuda:0")
    bf.set_contact_head(*head)
    want, want_lg, _ = bf.forward_contacts(tok, logits=True)
    assert np.array_equal(_bits(con), _bits(want)) and np.array_equal(_bits(lg), _bits(want_lg))
    strict16 = models.ESM1b(state_dict=sd, config=cfg, precision="fp16").model.to("cuda:0")
    strict16.set_contact_head(*head)
    with pytest.raises(_lib.PgError) as err:
        strict16.predict_contacts(tok)
    assert err.value.code == _lib.PG_ERR_RANGE


def test_predict_contacts_batch_does_not_depend_on_the_chunking():
    f = _family("esm2_35m")
    wrapped = C.model(f["wrapper"], f["cfg"], f["sd"], "bf16")
    w, bias, _ = _reference("esm2_35m")
    wrapped.model.set_contact_head(w, bias)
    s = esm_sampler.ESM_sampler(wrapped, device="cuda:0")
    seqs = ["ACDEFGH", "M", "KLMNPQR", "ACDEFGHIKLMNPQRSTVWYACDEFGHIKL", "WYVTSRQ"]
    tiny = f["cfg"]["n_heads"] * 9 * 9 * 4 * 2          # two sequences of 7 residues per call, one of 30
    runs = [list(s.predict_contacts_batch(seqs, batch_size=bs, max_map_bytes=cap)) for bs, cap in ((1, None), (2, None), (None, None), (None, tiny))]
    for seq, *maps in zip(seqs, *runs):
        assert maps[0].shape == (len(seq), len(seq)) and maps[0].dtype == np.float32
        assert all(np.array_equal(_bits(maps[0]), _bits(m)) for m in maps[1:])
    tok = s.model.batch_converter([("0", seqs[3])])[2].numpy()
    assert np.array_equal(_bits(runs[0][3]), _bits(s.model.model.predict_contacts(tok)[0]))
    assert np.array_equal(_bits(s.predict_contacts(seqs[0])), _bits(runs[0][0]))
