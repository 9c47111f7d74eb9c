"""Masked-marginal substitution tables on the GPU: the table kernel through pg_logprob_table_device (bit-identity with the gather
kernel, a derived bound against float64 numpy), the samplers' tables against log_likelihood_batch (bit for bit) and against the
oracle forwards, probs_single, the fp16 range guard, and the two command lines end to end."""
import ctypes
import functools
import random
import warnings

import numpy as np
import pytest
import torch

from oracle.esm_forward import EsmConfig, esm1b_forward, synthetic_esm_weights
from oracle.msa_forward import MsaConfig, msa_forward, synthetic_msa_weights
from protein_gibbs_sampler_amd import _lib, esm_msa_sampler, esm_sampler, likelihood_esm, models, pgen_msa_seq_probs, seq_probs_esm, weights
from protein_gibbs_sampler_amd.esm_msa_sampler import partition
from test_gpu_sampler_golden import _Plugin

pytestmark = pytest.mark.gpu
U = 2.0 ** -24                       # unit roundoff of binary32


# ---- kernel level ---------------------------------------------------------------------------------------
def _bounds(x64, n):
    """Error bounds of one log p and of the entropy, for a row whose normalisation set x64 (float64 view of the fp32 logits) has n
    members.  See test_table_kernel_against_float64 for the derivation."""
    D = float(x64.max() - x64.min())
    eps = U * (3.0 * D + n + 3.0 + 5.0 * np.log(n)) if n > 1 else U * 8.0
    ent = eps * (1.0 + np.log(n)) + (n + 4.0) * U * np.log(n) + 1e-30
    return eps, ent


def _ref_table(logits, width, idx, row_map, cols, norm):
    """float64 numpy: (table [n_sel, P, n_cols], entropy [n_sel, P], eps [n_sel, P], ent_bound [n_sel, P], live [n_sel, P])."""
    n_sel, P = idx.shape
    tab = np.zeros((n_sel, P, len(cols)))
    ent, eps, entb = np.zeros((n_sel, P)), np.zeros((n_sel, P)), np.zeros((n_sel, P))
    live = (idx >= 0) & (idx < width)
    for s in range(n_sel):
        for p in range(P):
            if not live[s, p]:
                continue
            row = logits[row_map[s] if row_map is not None else s, idx[s, p]].astype(np.float64)
            x = row[cols] if norm == _lib.PG_TABLE_NORM_COLUMNS else row
            lp = x - x.max() - np.log(np.exp(x - x.max()).sum())
            tab[s, p] = lp if norm == _lib.PG_TABLE_NORM_COLUMNS else lp[cols]
            ent[s, p] = -(np.exp(lp) * lp).sum()
            eps[s, p], entb[s, p] = _bounds(x, len(x))
    return tab, ent, eps, entb, live


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _run_table(logits, idx, row_map, cols, norm, want_entropy):
    dev = torch.device("cuda:0")
    n_rows, width, V = logits.shape
    n_sel, P = idx.shape
    d_logits, d_idx, d_cols = (torch.from_numpy(a).to(dev) for a in (logits, idx, cols))
    d_map = torch.from_numpy(row_map).to(dev) if row_map is not None else None
    out = torch.full((n_sel, P, len(cols)), 7.0, dtype=torch.float32, device=dev)          # a pattern: skipped entries must be WRITTEN
    ent = torch.full((n_sel, P), 7.0, dtype=torch.float32, device=dev) if want_entropy else None
    L = _lib.lib()
    with torch.cuda.device(dev):
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(L.pg_logprob_table_device(st, _ptr(d_logits), n_rows, width, V, _ptr(d_idx), _ptr(d_map), n_sel, P, _ptr(d_cols),
                                             len(cols), norm, _ptr(out), _ptr(ent)))
        gathered = np.zeros((len(cols), n_sel, P), dtype=np.float32)
        if norm == _lib.PG_TABLE_NORM_VOCAB:
            for c, col in enumerate(cols):
                tgt = torch.full((n_sel, P), int(col), dtype=torch.int32, device=dev)
                g = torch.full((n_sel, P), 7.0, dtype=torch.float32, device=dev)
                _lib.check(L.pg_logprob_gather_device(st, _ptr(d_logits), n_rows, width, V, _ptr(d_idx), _ptr(d_map), _ptr(tgt), n_sel, P, _ptr(g)))
                gathered[c] = g.cpu().numpy()
        torch.cuda.synchronize(dev)
    return out.cpu().numpy(), (ent.cpu().numpy() if want_entropy else None), gathered


def _kernel_cases():
    """Every (V, n_cols) pair with both normalisations on the SAME entry shape, row_map and entropy pointer; those three cycle along
    the ten pairs (six shapes, row_map every other pair, entropy in pairs of two), so every entry count, both values of P, row_map
    null and not null and the entropy pointer null and not null each meet both normalisations."""
    shapes = [(1, 1), (256, 1), (257, 1), (171, 3), (1, 3), (86, 3)]        # (n_sel, P): 1, 256, 257, 513, 3, 258 entries
    cases, k = [], 0
    for V in (1, 33, 35, 64):
        for n_cols in sorted({1, 20, V}):
            if n_cols > V:
                continue
            n_sel, P = shapes[k % len(shapes)]
            for norm in (_lib.PG_TABLE_NORM_VOCAB, _lib.PG_TABLE_NORM_COLUMNS):
                cases.append((V, n_cols, norm, n_sel, P, k % 2 == 1, (k // 2) % 2 == 0))
            k += 1
    return cases


def test_kernel_cases_cover_every_value_under_both_normalisations():
    cases = _kernel_cases()
    for norm in (_lib.PG_TABLE_NORM_VOCAB, _lib.PG_TABLE_NORM_COLUMNS):
        mine = [c for c in cases if c[2] == norm]
        assert {c[3] * c[4] for c in mine} >= {1, 256, 257, 513} and {c[4] for c in mine} == {1, 3}
        assert {c[5] for c in mine} == {False, True} and {c[6] for c in mine} == {False, True}
        assert {c[0] for c in mine} == {1, 33, 35, 64} and {c[1] for c in mine} == {1, 20, 33, 35, 64}
        assert any(c[4] == 3 and c[3] > 1 and c[5] for c in mine)            # s = i / P and row_map[s] both non-trivial


@pytest.mark.parametrize("V,n_cols,norm,n_sel,P,with_map,with_entropy", _kernel_cases())
def test_table_kernel_against_float64(V, n_cols, norm, n_sel, P, with_map, with_entropy):
    """Exact: with PG_TABLE_NORM_VOCAB column c equals pg_logprob_gather_device for target cols[c], bit for bit, at every entry;
    skipped entries (idx < 0 or >= width) are zeros in both outputs.

    Bounded, against float64 numpy on the same fp32 logits (u = 2^-24; n = members of the normalisation set, D = max - min of its
    logits; expf and logf of the device library are taken as accurate to 2 ulp = 4u relative, twice what the library documents):
      d_v = fl(x_v - mx)                 |error| <= u D
      e_v = expf(d_v)                    relative error <= D u (from d_v) + 4u
      sum = e_0 + ... in order           n - 1 additions of positive terms: relative error <= (n - 1) u on top, sum in [1, n]
      ls  = logf(sum)                    |error| <= (D + 4 + n - 1) u + 4u log n
      lp  = fl(d_c - ls)                 |error| <= u D (d_c) + the error of ls + u (D + log n) (the rounding of the difference)
    so |lp - exact| <= eps = u (3 D + n + 3 + 5 log n).
      H = -(p_0 lp_0 + ...) with p_v = expf(lp_v): p_v has relative error <= eps + 4u, the product one more u, so the terms are off
      by at most (eps + 5u) p|lp| + eps p, which sums to (eps + 5u) H + eps; n - 1 additions of same-signed terms add (n - 1) u H;
      H <= log n:  |H - exact| <= eps (1 + log n) + (n + 4) u log n.
    With PG_TABLE_NORM_COLUMNS the exact probabilities of a row sum to 1, so the float64 sum of exp(returned lp) is within
    sum p_c (e^eps - 1) <= n_cols eps of 1."""
    rng = np.random.default_rng(1000 * V + 10 * n_cols + norm + n_sel)
    width = 7
    n_rows = n_sel + 2 if with_map else n_sel
    logits = (rng.standard_normal((n_rows, width, V)) * 2.5).astype(np.float32)
    idx = rng.integers(0, width, (n_sel, P)).astype(np.int32)
    if n_sel * P > 1:
        skip = rng.random((n_sel, P)) < 0.2
        idx[skip] = np.where(rng.random(int(skip.sum())) < 0.5, -1, width + rng.integers(0, 3, int(skip.sum())))
        idx.reshape(-1)[0], idx.reshape(-1)[-1] = -1, 3
    row_map = rng.permutation(n_rows)[:n_sel].astype(np.int32) if with_map else None
    cols = rng.permutation(V)[:n_cols].astype(np.int32)
    got, ent, gathered = _run_table(logits, idx, row_map, cols, norm, with_entropy)
    want, want_ent, eps, entb, live = _ref_table(logits, width, idx, row_map, cols, norm)
    assert (got[~live] == 0).all() and (ent is None or (ent[~live] == 0).all())
    assert np.isfinite(got).all()
    if norm == _lib.PG_TABLE_NORM_VOCAB:
        assert np.array_equal(got.view(np.uint32), np.moveaxis(gathered, 0, -1).view(np.uint32))
    err = np.abs(got.astype(np.float64) - want)
    print("max |lp err| / bound = %.3f" % (err[live] / eps[live][:, None]).max() if live.any() else "no live entry")
    assert (err <= eps[..., None]).all()
    if ent is not None:
        assert (np.abs(ent.astype(np.float64) - want_ent) <= entb).all()
    if norm == _lib.PG_TABLE_NORM_COLUMNS:
        total = np.exp(got.astype(np.float64)).sum(-1)
        assert (np.abs(total - 1.0)[live] <= (n_cols * eps)[live]).all()


# ---- sampler level: the small models of tests/test_gpu_loglik.py --------------------------------------------
SEQS = ["MRHGDISSSNDTVGVAVVNYKMPRLHTAAEVLDNAR", "ACDEFGHIKL"]
ESM_KW = (dict(mask_distance=6), dict(with_masking=False), dict(mask_distance=3, batch_size=2))
MSAS = [["ACDEFGHIKL", "AC-EFGHIKL", "ACDEFG--KL"], ["MKV-A", "MKVAA"]]
MSA_KW = (dict(target_index=1, mask_distance=4), dict(target_index=0, with_masking=False, count_gaps=True))
TOL = {"bf16": 0.15, "fp32": 1e-3}         # the logit / log-likelihood bounds test_engine_log_likelihood_vs_oracle applies to these models
OCFG = EsmConfig(d_model=128, n_layers=2, n_heads=2, d_ffn=256, max_pos=80)
MCFG = MsaConfig(d_model=128, n_layers=2, n_heads=2, d_ffn=256, max_pos=40, max_rows=8)


@functools.lru_cache(None)
def _weights():
    return (synthetic_esm_weights(OCFG, seed=21, std=0.08, embed_std=0.5, ln_jitter=0.1),
            synthetic_msa_weights(MCFG, seed=22, std=0.08, embed_std=0.5, ln_jitter=0.1))


@functools.lru_cache(None)
def _esm(precision):
    cfg = weights.make_config(weights.ESM1B_CONFIG, d_model=128, n_layers=2, d_ffn=256, max_positions=80)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return esm_sampler.ESM_sampler(models.ESM1b(state_dict=_weights()[0], config=cfg, precision=precision), device="cuda:0")


@functools.lru_cache(None)
def _msa(precision):
    cfg = weights.make_config(weights.MSA1B_CONFIG, d_model=128, n_layers=2, d_ffn=256, max_positions=40, max_msa_rows=8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return esm_msa_sampler.ESM_MSA_sampler(models.ESM_MSA1(state_dict=_weights()[1], config=cfg, precision=precision), device="cuda:0")


def _log_softmax64(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def _esm_order(L, kw):
    """0-based positions in the order log_likelihood_batch lists them: copy by copy, a copy's positions ascending."""
    n = int(min(kw.get("mask_distance", float("inf")), L)) if kw.get("with_masking", True) else 1
    return [p for i in range(n) for p in range(i, L, n)]


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def _check_esm_exact(s):
    for kw in ESM_KW:
        lists = [l for _, l in s.log_likelihood_batch(SEQS, **kw)]
        tables = list(s.masked_marginals_batch(SEQS, **kw))
        for seq, l, (logp, entropy, toks) in zip(SEQS, lists, tables):
            assert logp.shape == (len(seq), 20) and logp.dtype == np.float32 and entropy.shape == (len(seq),)
            assert toks == [s.model.alphabet.get_tok(i) for i in s.valid_aa_idx]
            own = [logp[p, toks.index(seq[p])] for p in _esm_order(len(seq), kw)]
            assert np.array_equal(_bits(own), _bits(l))
            assert (entropy > 0).all() and (entropy <= np.log(33) + 1e-5).all()


def _check_msa_exact(s):
    for kw in MSA_KW:
        lists = [l for _, l in s.log_likelihood_batch(MSAS, **kw)]
        tables = list(s.masked_marginals_batch(MSAS, **kw))
        for msa, l, (logp, entropy, positions, toks) in zip(MSAS, lists, tables):
            row = msa[kw["target_index"]]
            scored = [p for p in range(len(row)) if kw.get("count_gaps") or row[p] != "-"]
            assert positions == scored and logp.shape == (len(scored), 21) and entropy.shape == (len(scored),) and toks == s.toks
            n = int(min(kw.get("mask_distance", float("inf")), len(row))) if kw.get("with_masking", True) else 1
            order = [p for i in range(n) for p in range(i, len(row), n) if p in scored]
            own = [logp[positions.index(p), toks.index(row[p])] for p in order]
            assert np.array_equal(_bits(own), _bits(l))


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_tables_hold_log_likelihood_batch_bit_for_bit(precision):
    _check_esm_exact(_esm(precision))
    _check_msa_exact(_msa(precision))


def test_tables_hold_log_likelihood_batch_bit_for_bit_with_a_plugin_model():
    _check_esm_exact(esm_sampler.ESM_sampler(_Plugin(False), device="cuda:0"))
    _check_msa_exact(esm_msa_sampler.ESM_MSA_sampler(_Plugin(True), device="cuda:0"))


@functools.lru_cache(None)
def _oracle_esm_tables(kw_no):
    """log_softmax of the oracle's logits at the masked positions, [L, 33] per sequence (float64).  The masked copies are built here,
    from the definition (copy i of n = min(mask_distance, L) has <mask> = 32 at residues i, i + n, ...; <cls> = 0 in front, <eos> = 2
    behind), not taken from the sampler."""
    kw, sd, out = ESM_KW[kw_no], _weights()[0], []
    alphabet = _esm("fp32").model.alphabet
    for seq in SEQS:
        L = len(seq)
        one = np.asarray([0] + [alphabet.get_idx(c) for c in seq] + [2], dtype=np.int64)
        full = np.zeros((L, 33))
        if kw.get("with_masking", True):
            n = int(min(kw.get("mask_distance", float("inf")), L))
            copies = np.tile(one, (n, 1))
            for i in range(n):
                copies[i, 1 + i:L + 1:n] = 32
            lp = _log_softmax64(esm1b_forward(sd, OCFG, copies))
            for p in range(L):
                full[p] = lp[p % n, 1 + p]
        else:
            full[:] = _log_softmax64(esm1b_forward(sd, OCFG, one[None]))[0, 1:L + 1]
        out.append(full)
    return out


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_esm_table_against_the_oracle(precision):
    """|d log p_c| <= |dx_c| + max |dx|, so the bound is twice the one the engine-vs-oracle test applies to this model's logits:
    2e-3 in the strict mode (the 1e-3 all-logits contract), 0.3 with bf16 operands."""
    s = _esm(precision)
    for kw_no, kw in enumerate(ESM_KW):
        for (logp, entropy, _), want in zip(s.masked_marginals_batch(SEQS, **kw), _oracle_esm_tables(kw_no)):
            err = np.abs(logp - want[:, s.valid_aa_idx]).max()
            print("%s %r: max |log p err| %.3e" % (precision, kw, err))
            assert err < 2 * TOL[precision]
        cols = list(s.masked_marginals_batch(SEQS, normalise="columns", **kw))
        for (logp, _, _), want in zip(cols, _oracle_esm_tables(kw_no)):
            assert np.abs(logp - _log_softmax64(want[:, s.valid_aa_idx])).max() < 2 * TOL[precision]
            assert np.abs(np.exp(logp.astype(np.float64)).sum(-1) - 1).max() < 1e-5


@functools.lru_cache(None)
def _oracle_msa_tables(kw_no):
    """The same for the MSA model, [L, 33] per MSA for its target row.  Built from the definition: with masking every MSA alone, copy
    i masked at columns i, i + n, ... of the target row; without, the whole list padded with <pad> = 1 to the deepest / widest MSA
    and scored one MSA per forward (batch_size 1).  Tokens: <cls> = 0 in front of every row, no <eos>."""
    kw, sd, out = MSA_KW[kw_no], _weights()[1], []
    alphabet = _msa("fp32").model.alphabet
    tr = kw["target_index"]
    toks = [np.asarray([[0] + [alphabet.get_idx(c) for c in row] for row in msa], dtype=np.int64) for msa in MSAS]
    if kw.get("with_masking", True):
        for one in toks:
            L = one.shape[1] - 1
            n = int(min(kw.get("mask_distance", float("inf")), L))
            copies = np.tile(one[None], (n, 1, 1))
            for i in range(n):
                copies[i, tr, 1 + i:L + 1:n] = 32
            lp = _log_softmax64(msa_forward(sd, MCFG, copies))
            out.append(np.stack([lp[p % n, tr, 1 + p] for p in range(L)]))
        return out
    R, C = max(t.shape[0] for t in toks), max(t.shape[1] for t in toks)
    for one in toks:
        padded = np.full((1, R, C), 1, dtype=np.int64)
        padded[0, :one.shape[0], :one.shape[1]] = one
        out.append(_log_softmax64(msa_forward(sd, MCFG, padded))[0, tr, 1:one.shape[1]])
    return out


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_msa_table_against_the_oracle(precision):
    s = _msa(precision)
    for kw_no, kw in enumerate(MSA_KW):
        tables = list(s.masked_marginals_batch(MSAS, **kw))
        assert len(tables) == len(MSAS)
        for msa, (logp, _, positions, _), want in zip(MSAS, tables, _oracle_msa_tables(kw_no)):
            row = msa[kw["target_index"]]
            assert positions == [p for p in range(len(row)) if kw.get("count_gaps") or row[p] != "-"]
            err = np.abs(logp - want[positions][:, s.valid_aa_idx]).max()
            print("%s %r: max |log p err| %.3e" % (precision, kw, err))
            assert err < 2 * TOL[precision]


def test_score_mutations_reads_one_table():
    s = _esm("fp32")
    seq = SEQS[1]
    logp, _, toks = s.masked_marginals(seq)
    got = s.score_mutations(seq, ["A1G", "K9L", "L10L"])
    want = [logp[0, toks.index("G")] - logp[0, toks.index("A")], logp[8, toks.index("L")] - logp[8, toks.index("K")], 0.0]
    assert got == [float(v) for v in want]


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("steps", [None, 4])
def test_probs_single(steps, precision):
    s, sd = _msa(precision), _weights()[1]
    msa = MSAS[0]
    L = len(msa[0])
    random.seed(11)
    probs, toks = s.probs_single(msa, steps=steps, show_progress_bar=False)
    state = random.getstate()
    assert probs.shape == (21, L) and probs.dtype == np.float32 and toks == s.toks
    assert np.abs(probs.astype(np.float64).sum(0) - 1).max() < 1e-5
    random.seed(11)
    shuffled = list(range(1, L + 1))
    random.shuffle(shuffled)
    assert random.getstate() == state
    _, _, one = s.model.batch_converter([(str(i), r) for i, r in enumerate(msa)])
    want = np.zeros((21, L))
    for b in partition(shuffled, L if steps is None else steps):
        tok = one.numpy().copy()
        tok[0, -1, b] = s.model.alphabet.mask_idx
        lg = msa_forward(sd, MCFG, tok)[0, -1]
        want[:, np.asarray(b) - 1] = np.exp(_log_softmax64(lg[b][:, s.valid_aa_idx])).T
    tol = np.expm1(2 * TOL[precision])
    assert (np.abs(probs - want) <= want * tol + 1e-7).all(), np.abs(probs / want - 1).max()
    random.seed(11)
    again, _ = s.probs_single(msa, steps=steps, show_progress_bar=False)
    random.seed(11)
    one_by_one, _ = s.probs_single(msa, steps=steps, show_progress_bar=False, batch_size=1)
    assert np.array_equal(_bits(again), _bits(probs)) and np.array_equal(_bits(one_by_one), _bits(probs))


# ---- the fp16 range guard (the overflow weights of tests/test_gpu_fp16_mode.py) ------------------------------
def _overflow_setup():
    cfg = weights.make_config(weights.ESM1B_CONFIG, d_model=256, n_layers=3, d_ffn=512, max_positions=128)
    sd = {k: v.copy() for k, v in weights.synthetic_state_dict(cfg, seed=21, std=0.05, embed_std=0.3, ln_jitter=0.1).items()}
    sd["layers.1.fc1.weight"] *= np.float32(1e5)
    tok = np.concatenate([np.zeros((3, 1)), np.random.default_rng(2).integers(4, 24, (3, 40)), np.full((3, 1), 2)], axis=1).astype(np.int32)
    tok[1, 5] = tok[2, 17] = 32
    return cfg, sd, tok


def test_fp16_overflow_is_a_range_error_and_auto_falls_back(monkeypatch):
    monkeypatch.setenv("PGIBBS_F16_PROBE", "0")
    cfg, sd, tok = _overflow_setup()
    args = (tok, np.arange(3), np.tile(np.array([3, 9], dtype=np.int32), (3, 1)), list(range(4, 24)))
    lm = models.ESM1b(state_dict=sd, config=cfg, precision="fp16").model.to("cuda:0")
    with pytest.raises(_lib.PgError) as ei:
        lm.forward_logprob_table(*args, want_entropy=True)
    assert ei.value.code == _lib.PG_ERR_RANGE
    with pytest.raises(_lib.PgError) as ei:
        lm.forward_logprob_table(*args, normalise="columns")
    assert ei.value.code == _lib.PG_ERR_RANGE
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        auto = models.ESM1b(state_dict=sd, config=cfg).model.to("cuda:0")
    assert auto.precision_name == "fp16"
    with pytest.warns(UserWarning, match="run again with bf16 operands") as rec:
        got, got_ent = auto.forward_logprob_table(*args, want_entropy=True)
    assert len(rec) == 1 and auto.fallbacks == 1 and auto.precision_name == "fp16"
    want, want_ent = models.ESM1b(state_dict=sd, config=cfg, precision="bf16").model.to("cuda:0").forward_logprob_table(*args, want_entropy=True)
    assert np.isfinite(got).all() and np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(got_ent), _bits(want_ent))


def test_a_non_finite_logit_outside_the_selected_columns_is_a_range_error_under_both_normalisations():
    """lm_head.bias[<cls>] = inf: every row's logit 0 is inf, the 20 residue logits stay finite.  PG_TABLE_NORM_VOCAB meets it in the
    row maximum; PG_TABLE_NORM_COLUMNS never reads that logit for its result and must find it in its scan of the whole row."""
    cfg = weights.make_config(weights.ESM1B_CONFIG, d_model=128, n_layers=2, d_ffn=256, max_positions=80)
    sd = {k: np.array(v, copy=True) for k, v in _weights()[0].items()}
    sd["lm_head.bias"][0] = np.inf
    lm = models.ESM1b(state_dict=sd, config=cfg, precision="bf16").model.to("cuda:0")
    tok = np.asarray([[0, 5, 6, 7, 8, 2]], dtype=np.int32)
    lg = None
    try:
        lg = lm.forward_logits(tok)
    except _lib.PgError as e:                                   # the all-logits entry scans on the host: the same error
        assert e.code == _lib.PG_ERR_RANGE
    assert lg is None
    for normalise in ("vocab", "columns"):
        for want_entropy in (False, True):
            with pytest.raises(_lib.PgError) as ei:
                lm.forward_logprob_table(tok, [0], [[1, 3]], list(range(4, 24)), normalise=normalise, want_entropy=want_entropy)
            assert ei.value.code == _lib.PG_ERR_RANGE
    ok = _esm("bf16").model.model.forward_logprob_table(tok, [0], [[1, 3]], list(range(4, 24)), normalise="columns")[0]
    assert np.isfinite(ok).all()                                # the same call on the untouched weights


def test_engine_entries_refuse_bad_columns_by_name():
    lm = _esm("fp32").model.model
    tok = np.asarray([[0, 5, 6, 7, 2]], dtype=np.int32)
    for cols, msg in (([4, 33], "column 33 is outside the vocabulary of 33"), ([-1], "column -1"), (list(range(33)) + [0], "n_cols must be in 1..V")):
        with pytest.raises(_lib.PgError, match=msg) as ei:
            lm.forward_logprob_table(tok, [0], [[1, 2]], cols)
        assert ei.value.code == _lib.PG_ERR_INVALID


# ---- the two command lines, end to end on synthetic weights -----------------------------------------------
def test_seq_probs_esm_command_line(tmp_path, monkeypatch):
    cfg = weights.make_config(weights.ESM1B_CONFIG, d_model=128, n_layers=2, d_ffn=256, max_positions=80)
    seen = {}

    def small(checkpoint=None, precision="auto", synthetic=False):
        seen.update(synthetic=synthetic, precision=precision)
        return models.ESM1v(state_dict=_weights()[0], config=cfg, precision=precision)
    monkeypatch.setitem(likelihood_esm.model_map, "esm1v", small)
    fasta, out = tmp_path / "in.fasta", tmp_path / "out.tsv"
    fasta.write_text(">q1 first\n%s\n>q2\nACD-EFG*HIKL\n" % SEQS[0])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        seq_probs_esm.cli(["-i", str(fasta), "-o", str(out), "--synthetic-weights", "--precision", "fp32", "--mask_distance", "6",
                           "--batch_size", "4", "--device", "cuda:0"])
    assert seen == dict(synthetic=True, precision="fp32")
    with open(out) as h:
        toks, table = seq_probs_esm.read_table(h)
    s = _esm("fp32")
    assert toks == [s.model.alphabet.get_tok(i) for i in s.valid_aa_idx] and sorted(table) == ["q1", "q2"]
    assert table["q1"]["seq"] == SEQS[0] and table["q2"]["seq"] == "ACDEFGHIKL"
    for name, seq in (("q1", SEQS[0]), ("q2", SEQS[1])):
        logp, entropy, _ = s.masked_marginals(seq, mask_distance=6, batch_size=4)
        assert np.array_equal(np.asarray(table[name]["logp"], dtype=np.float32), np.asarray([[float("%.8g" % v) for v in r] for r in logp], dtype=np.float32))
        assert np.allclose(table[name]["entropy"], entropy, rtol=1e-6)


def test_pgen_msa_seq_probs_command_line(tmp_path, monkeypatch):
    cfg = weights.make_config(weights.MSA1B_CONFIG, d_model=128, n_layers=2, d_ffn=256, max_positions=40, max_msa_rows=8)
    monkeypatch.setitem(pgen_msa_seq_probs.model_map, "esm_msa1",
                        lambda checkpoint=None, precision="auto", synthetic=False: models.ESM_MSA1(state_dict=_weights()[1], config=cfg, precision=precision))
    msa = MSAS[0]
    fasta, out = tmp_path / "in.a2m", tmp_path / "probs.tsv"
    fasta.write_text("".join(">%d\n%s\n" % (i, r.lower() if i == 1 else r) for i, r in enumerate(msa)))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pgen_msa_seq_probs.cli(["--msa", str(fasta), "-o", str(out), "--steps", "4", "--synthetic-weights", "--precision", "fp32",
                                "--seed", "5", "--device", "cuda:0"])
    with open(out, newline="") as h:
        back = pgen_msa_seq_probs.read_table(h)
    s = _msa("fp32")
    random.seed(5)
    probs, toks = s.probs_single(msa, steps=4, show_progress_bar=False)
    assert back["target"] == msa[-1] and back["toks"] == toks and back["position"] == list(range(1, 11))
    assert np.array_equal(back["probs"].astype(np.float32), np.asarray([[float("%.8g" % v) for v in r] for r in probs], dtype=np.float32))
    assert back["consensus"] == "".join(toks[i] for i in probs.argmax(0))
    assert back["different"] == [int(c != t) for c, t in zip(back["consensus"], msa[-1])]
