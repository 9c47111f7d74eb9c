"""A recording stand-in for the HIP engine, shared by the CPU tests that drive the samplers without a GPU.

`fake_engine_model(msa)` returns a plug-in (alphabet, batch converter, `.model`) whose `.model` is a NativeMaskedLM subclass with
every device call replaced by a deterministic function of its inputs.  It keeps three logs: `calls` (token shapes of the Gibbs
calls), `job_items` (every set_job_items value) and `trace` (every call with its arrays' dtype, shape and bytes, its scalars and
every field of each SampleParams, taken BEFORE the call changes anything)."""
import hashlib

import numpy as np

SHADOW_BIT = 1 << 30        # include/pgibbs.h: sampled but not written


def _arr(a):
    a = np.ascontiguousarray(a.numpy() if hasattr(a, "numpy") else a)
    return ("array", a.dtype.str, a.shape, hashlib.sha256(a.tobytes()).hexdigest())


def _params(p):
    out = []
    for name, _ in p._fields_:
        v = getattr(p, name)
        out.append((name, list(v) if hasattr(v, "__len__") else v))
    return tuple(out)


def _score(row, pos, what, tok):
    """A float32 'log-probability' that depends on where it was read, what was asked for and the token found there."""
    return -np.float32(((row * 31 + pos * 17 + what * 7 + tok * 3) % 97) + 1) / np.float32(8)


def fake_engine_model(msa):
    """What the sharded generate() must reproduce for any number of ranks: draws are a function of (global Philox row id,
    iteration, slot), scores a function of (token row, position, target or column, token there)."""
    from protein_gibbs_sampler_amd.alphabet import Alphabet
    from protein_gibbs_sampler_amd.engine import NativeMaskedLM

    class FakeLM(NativeMaskedLM):
        def __init__(self):
            self.calls = []
            self.job_items = []
            self.trace = []

        def set_job_items(self, n):          # the samplers announce the whole batch around every shard call and reset it
            self.job_items.append(int(n))
            self.trace.append(("set_job_items", int(n)))

        def eval(self):
            return self

        def to(self, device):
            return self

        def gibbs_run(self, tokens, target_idx, params, want_logits=False, want_tokens=False):
            self.calls.append(tokens.shape)
            self.trace.append(("gibbs_run", _arr(tokens), _arr(target_idx), _params(params), want_logits, want_tokens))
            flat = tokens.reshape(-1, tokens.shape[-1])
            idx = np.asarray(target_idx).reshape(target_idx.shape[0], -1, target_idx.shape[-1])
            st = np.zeros(idx.shape, dtype=np.int32)
            for it in range(idx.shape[0]):
                for r in range(flat.shape[0]):
                    for p in range(idx.shape[2]):
                        v = int(idx[it, r, p])
                        if v < 0:
                            continue
                        st[it, r, p] = 4 + ((params.row_id_base + r) * 7 + it * 3 + p + params.rng_seed) % 20
                        if not v & SHADOW_BIT:
                            flat[r, v] = st[it, r, p]
            st = st.reshape(np.asarray(target_idx).shape)
            lg = (st[..., None] * np.float32(0.25) + np.arange(3, dtype=np.float32)) if want_logits else None
            return lg, (st if want_tokens else None)

        def gibbs_single_batch_run(self, tokens, mask_row, target_row, step_idx, step_sample, params_list, want_logits=False,
                                   want_tokens=False):
            self.calls.append(tokens.shape)
            self.trace.append(("gibbs_single_batch_run", _arr(tokens), int(mask_row), int(target_row), _arr(step_idx),
                               [int(f) for f in step_sample], [_params(p) for p in params_list], want_logits, want_tokens))
            st = np.zeros(step_idx.shape, dtype=np.int32)
            for s_i in range(step_idx.shape[0]):
                for b in range(tokens.shape[0]):
                    for p, pos in enumerate(step_idx[s_i, b]):
                        if pos >= 0:
                            tokens[b, mask_row, pos] = 32
                            st[s_i, b, p] = 4 + (params_list[b].rng_seed * 5 + s_i * 3 + p + int(step_sample[s_i])) % 20
                            tokens[b, target_row, pos] = st[s_i, b, p]
            lg = (st[..., None] * np.float32(0.25) + np.arange(3, dtype=np.float32)) if want_logits else None
            return lg, (st if want_tokens else None)

        def forward_logprobs(self, tokens, row_of, idx, targets):
            self.trace.append(("forward_logprobs", _arr(tokens), _arr(row_of), _arr(idx), _arr(targets)))
            flat = np.asarray(tokens).reshape(-1, np.asarray(tokens).shape[-1])
            idx, targets = np.asarray(idx), np.asarray(targets)
            out = np.zeros(idx.shape, dtype=np.float32)
            for s, row in enumerate(np.asarray(row_of)):
                for p, pos in enumerate(idx[s]):
                    if pos >= 0:
                        out[s, p] = _score(int(row), int(pos), int(targets[s, p]), int(flat[row, pos]))
            return out

        def forward_logprob_table(self, tokens, row_of, idx, cols, normalise="vocab", want_entropy=False):
            self.trace.append(("forward_logprob_table", _arr(tokens), _arr(row_of), _arr(idx), _arr(cols), normalise, want_entropy))
            flat = np.asarray(tokens).reshape(-1, np.asarray(tokens).shape[-1])
            idx, cols = np.asarray(idx), np.asarray(cols).reshape(-1)
            out = np.zeros(idx.shape + (len(cols),), dtype=np.float32)
            ent = np.zeros(idx.shape, dtype=np.float32)
            for s, row in enumerate(np.asarray(row_of)):
                for p, pos in enumerate(idx[s]):
                    if pos >= 0:
                        for c, col in enumerate(cols):
                            out[s, p, c] = _score(int(row), int(pos), int(col) + len(normalise), int(flat[row, pos]))
                        ent[s, p] = np.float32((int(row) * 13 + int(pos) * 5 + int(flat[row, pos])) % 11) / np.float32(4)
            return out, (ent if want_entropy else None)

    class Plug:
        pass

    plug = Plug()
    plug.alphabet = Alphabet(True, not msa)
    plug.batch_converter = plug.alphabet.get_batch_converter(msa=msa)
    plug.model = FakeLM()
    return plug
