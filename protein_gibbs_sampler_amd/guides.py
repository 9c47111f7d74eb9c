"""Guided Gibbs draws (pg_draw v2; not in the reference): per-position residue constraints and priors, nucleus
(top-p) truncation and a temperature schedule over the iterations.

A DrawGuide is what the user writes; compile() resolves it against one sampler's alphabet order and one token-row width into the
tables the draw kernel reads (include/pgibbs.h, pg_draw_guide): a float32 bias table [1, width, n_valid] in the order of the
sampler's `valid_aa_idx` (-inf = forbidden), a float32 temperature per iteration, and top_p.  Positions are keyed as the samplers'
`indexes` are: token positions, so residue 0 of a sequence with <cls> in front is position 1.
"""
import math

import numpy as np

SCHEDULE_KINDS = ("linear", "geometric")


def annealing_schedule(kind, t_start, t_end, n):
    """n temperatures from t_start to t_end inclusive: "linear" in T, or "geometric" (linear in log T).  n = 1 gives [t_start]."""
    if kind not in SCHEDULE_KINDS:
        raise ValueError("annealing_schedule: kind must be one of %s, got %r" % (", ".join(SCHEDULE_KINDS), kind))
    n = int(n)
    t_start, t_end = float(t_start), float(t_end)
    if n < 1:
        raise ValueError("annealing_schedule: n must be at least 1, got %d" % n)
    if not (math.isfinite(t_start) and math.isfinite(t_end) and t_start > 0 and t_end > 0):
        raise ValueError("annealing_schedule: temperatures must be finite and > 0, got %r and %r" % (t_start, t_end))
    if n == 1:
        return [t_start]
    if kind == "linear":
        out = [t_start + (t_end - t_start) * i / (n - 1) for i in range(n)]
    else:
        out = [t_start * (t_end / t_start) ** (i / (n - 1)) for i in range(n)]
    out[0], out[-1] = t_start, t_end
    return out


def parse_schedule(spec, n):
    """"kind:t0:t1" (the command-line form) -> annealing_schedule(kind, t0, t1, n)."""
    parts = str(spec).split(":")
    if len(parts) != 3:
        raise ValueError("temperature_schedule: expected kind:t_start:t_end (kind linear or geometric), got %r" % (spec,))
    return annealing_schedule(parts[0], float(parts[1]), float(parts[2]), n)


class CompiledGuide:
    """The tables of one call: bias float32 [1, width, n_valid] or None, temperatures float32 [n] or None, top_p float or None."""

    def __init__(self, bias, temperatures, top_p):
        self.bias, self.temperatures, self.top_p = bias, temperatures, top_p

    @property
    def empty(self):
        return self.bias is None and self.temperatures is None and self.top_p is None


class DrawGuide:
    """position_bias: {pos: {"A": 1.5, ...}} or an array [width][n_valid] added to the logits of the valid residues;
    allowed_residues: {pos: "DE"}: only these at pos; forbidden_residues: "C" (every position) or {pos: "C"};
    top_p in (0, 1]; temperature_schedule: one temperature per iteration (a sequence, or "kind:t_start:t_end")."""

    def __init__(self, position_bias=None, allowed_residues=None, forbidden_residues=None, top_p=None, temperature_schedule=None):
        self.position_bias = position_bias
        self.allowed_residues = allowed_residues
        self.forbidden_residues = forbidden_residues
        self.top_p = top_p
        self.temperature_schedule = temperature_schedule

    @property
    def empty(self):
        return all(v is None for v in (self.position_bias, self.allowed_residues, self.forbidden_residues, self.top_p,
                                       self.temperature_schedule))

    def digest_parts(self):
        """The guide's arguments as plain values, for the job digest that the ranks of a sharded job compare."""
        import hashlib

        def plain(v):
            if v is None or isinstance(v, (str, int, float)):
                return v
            if isinstance(v, dict):
                return tuple(sorted((repr(k), plain(x)) for k, x in v.items()))
            arr = np.ascontiguousarray(np.asarray(v, dtype=np.float64))
            return (arr.shape, hashlib.sha256(arr.tobytes()).hexdigest())
        return tuple(plain(v) for v in (self.position_bias, self.allowed_residues, self.forbidden_residues, self.top_p,
                                        self.temperature_schedule))

    def compile(self, residues, width, n_iters=None, clean=None):
        """residues: the single-letter tokens of the sampler's valid_aa_idx, in that order; width: tokens per row; n_iters: the
        iterations (or steps) of the call, which the schedule must cover; clean: the sampler's clean_seed_seq, which raises its
        "Invalid input character: ..." for a residue outside its alphabet."""
        residues = list(residues)
        nv = len(residues)
        col = {r: j for j, r in enumerate(residues)}

        def columns(text):
            text = clean(text) if clean is not None else str(text).upper()
            bad = set(text) - set(col)
            if bad:
                raise Exception("Invalid input character: " + ",".join(sorted(bad)))
            return [col[c] for c in text]

        def position(key):
            pos = int(key)
            if pos != key or isinstance(key, bool):
                raise TypeError("a draw guide's positions are integers, got %r" % (key,))
            if pos < 0 or pos >= width:
                raise IndexError("draw guide position %d is out of range for a token row of width %d" % (pos, width))
            return pos

        bias = None
        if self.position_bias is not None or self.allowed_residues is not None or self.forbidden_residues is not None:
            bias = np.zeros((1, width, nv), dtype=np.float32)
        if self.position_bias is not None:
            if isinstance(self.position_bias, dict):
                for key, entry in self.position_bias.items():
                    pos = position(key)
                    for res, value in entry.items():
                        if len(str(res)) != 1:
                            raise ValueError("position_bias: %r is not one residue" % (res,))
                        bias[0, pos, columns(res)[0]] += np.float32(value)
            else:
                arr = np.asarray(self.position_bias, dtype=np.float32)
                if arr.shape != (width, nv):
                    raise ValueError("position_bias: expected an array of shape (%d, %d) = (token-row width, valid residues), got %s"
                                     % (width, nv, arr.shape))
                bias[0] += arr
            if np.isnan(bias).any() or np.isposinf(bias).any():
                raise ValueError("position_bias: entries must be finite, or -inf to forbid a residue")
        if self.allowed_residues is not None:
            if not isinstance(self.allowed_residues, dict):
                raise TypeError("allowed_residues is a dict {position: residues}")
            for key, text in self.allowed_residues.items():
                keep = columns(text)
                off = np.ones(nv, dtype=bool)
                off[keep] = False
                bias[0, position(key), off] = -np.inf
        if self.forbidden_residues is not None:
            if isinstance(self.forbidden_residues, dict):
                for key, text in self.forbidden_residues.items():
                    bias[0, position(key), columns(text)] = -np.inf
            else:
                bias[0, :, columns(self.forbidden_residues)] = -np.inf
        if bias is not None:
            dead = np.flatnonzero(~(bias[0] > -np.inf).any(axis=1))
            if len(dead):
                raise ValueError("the draw guide forbids every residue at position %d" % int(dead[0]))

        temps = None
        if self.temperature_schedule is not None:
            sched = self.temperature_schedule
            if isinstance(sched, str):
                if n_iters is None:
                    raise ValueError("temperature_schedule %r needs the number of iterations" % (sched,))
                sched = parse_schedule(sched, n_iters)
            temps = np.asarray(list(sched), dtype=np.float32).reshape(-1)
            if not (np.isfinite(temps).all() and (temps > 0).all()) or len(temps) == 0:
                raise ValueError("temperature_schedule: temperatures must be finite and > 0")
            if n_iters is not None and len(temps) < n_iters:
                raise ValueError("temperature_schedule has %d entries, the call runs %d iterations" % (len(temps), n_iters))

        top_p = None
        if self.top_p is not None:
            top_p = float(self.top_p)
            if not (0.0 < top_p <= 1.0):
                raise ValueError("top_p must be in (0, 1], got %r" % (self.top_p,))
        return CompiledGuide(bias, temps, top_p)


def from_arguments(top_p=None, temperature_schedule=None, position_bias=None, allowed_residues=None, forbidden_residues=None):
    """The samplers' five keyword arguments as a DrawGuide, None when none of them is given."""
    g = DrawGuide(position_bias, allowed_residues, forbidden_residues, top_p, temperature_schedule)
    return None if g.empty else g


def compile_for(sampler, guide, width, n_iters):
    """guide (a DrawGuide or None) against `sampler`'s residue order; None when there is nothing to apply."""
    if guide is None:
        return None
    residues = [sampler.model.alphabet.get_tok(i) for i in sampler.valid_aa_idx]
    compiled = guide.compile(residues, width, n_iters, clean=sampler.clean_seed_seq)
    return None if compiled.empty else compiled
