#!/usr/bin/env python3
"""ESM-2 next to ESM-1b on one MI355X: what the rotary embedding costs.

For three shapes -- config 2 (256 chains x 258 tokens, 25 positions per iteration), a 32-chain shard of it, and one chain of 25
residues (27 tokens, 2 positions) -- both full-size models (33 x 1280, synthetic weights, bf16 operands) run the same Gibbs job from
device buffers (pg_esm_gibbs_run_device), alternating ESM-1b / ESM-2 for `--rounds` rounds in one process:

  * ms per Gibbs iteration: host clock around `--iters` iterations ending in a stream synchronisation, after `--warmup` iterations of the
    same shape; the median over the rounds is reported, every round is listed;
  * the rotation kernel: a separate profiled run (HIP events through pg_prof_*, class "rope"): ms per launch and achieved GB/s =
    (rows x 2 d_model x 2 B read + the same written) / time, next to the LayerNorm launches of the same run (class "layernorm":
    rows x d_model x (4 B read + 2 B written)) as the bandwidth yardstick of the box.

`--size 3b` measures ESM-2 3B (36 x 2560, 40 heads; models.ESM2_3B) alone at the same three shapes: ms per iteration, the rotation
and the LayerNorm launches at d_model 2560 with their GB/s.  Both sizes record the GEMM classes of the rotary model's profiled run
("gemm_qkv", "gemm_out", "gemm_fc1", "gemm_fc2": the launches that see every token row) as ms per launch and
TFLOP/s = 2 rows N K / time.

`--size 150m` measures ESM-2 150M (30 x 640, 20 heads of 32; models.ESM2_150M) alone at the same three shapes, with the attention
launches (class "attention") next to the rotation, and then the two head-32 kernels against their head-64 counterparts in the same
process ("head32_vs_head64"): 3-layer models of 20 heads of 32 (d_model 640), 20 heads of 64 (d_model 1280: the same B, T, H for
the attention launch) and 10 heads of 64 (d_model 640: the same bytes for the rotation), config-2 shape, profiled alternately for
`--rounds` rounds; ms per launch is the median over the rounds.

`--size 15b` measures ESM-2 15B (48 x 5120, 40 heads of 128, d_ffn 20480; models.ESM2_15B) at the same three shapes with the attention,
rotation, LayerNorm and GEMM classes.  The synthetic fp32 weights of all 48 layers are 60 GB of host memory; with `--layers L` < 48 the
tool also builds the model of L / 2 layers, times both alternately, and reports per shape the 48-layer figure EXTRAPOLATED from the two
(`ms_per_iteration_48_layers_extrapolated` = ms(L) + (48 - L) x (ms(L) - ms(L / 2)) / (L / 2): the embedding and the LM head are
counted once) -- every such key says "extrapolated".  `device_bytes` holds what hipMemGetInfo says is in use before and after each
engine is created (weights in the operand type, per precision mode) and after the config-2 run (with the activation buffers), and
the same extrapolation of the weights to 48 layers.

`--size 8m` measures ESM-2 8M (6 x 320, 20 heads of 16, d_ffn 1280; models.ESM2_8M) alone at the same three shapes with the attention,
rotation, LayerNorm and GEMM classes, and then the head-16 attention launch against the head-32 one of the same B, T, H in the same
process ("head16_vs_head32": 3-layer models of 20 heads of 16 (d_model 320) and 20 heads of 32 (d_model 640), config-2 shape,
profiled alternately).

`--size 35m` measures ESM-2 35M (12 x 480, 20 heads of 24, d_ffn 1920; models.ESM2_35M), which the engine runs embedded in slots of 32
(rows of 640 features: the byte and FLOP figures of its kernel classes are those of the RUN shape, what the kernels move and multiply),
with ESM-2 150M (30 x 640: the model whose kernels it runs) alternating in the same process at the same three shapes.

Prints one JSON line.  Needs a GPU: there is no CPU path.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

SHAPES = [("config2_256x258_p25", 256, 256, 25), ("shard_32x258_p25", 32, 256, 25), ("chain_1x27_p2", 1, 25, 2)]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=20, help="timed Gibbs iterations per run")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="alternations ESM-1b / ESM-2 per shape")
    ap.add_argument("--prof-iters", type=int, default=3, help="iterations of the profiled run")
    ap.add_argument("--layers", type=int, default=None, help="fewer layers for a rehearsal (default: 33, or 36 with --size 3b)")
    ap.add_argument("--size", choices=["650m", "3b", "150m", "15b", "8m", "35m"], default="650m",
                    help="650m: ESM-2 650M next to ESM-1b; 3b: ESM-2 3B alone; 150m: ESM-2 150M alone, then head 32 against head 64; "
                         "15b: ESM-2 15B alone (with --layers L < 48: L and L / 2 layers, 48 extrapolated); "
                         "8m: ESM-2 8M alone, then head 16 against head 32; 35m: ESM-2 35M (embedded in slots of 32) next to ESM-2 150M")
    args = ap.parse_args(argv)

    import torch
    from protein_gibbs_sampler_amd import _lib, esm_sampler, models, pyrandom, sharding, weights
    rotary = "esm2" if args.size == "650m" else "esm2_" + args.size      # the size's row of weights.ESM2_SIZES: wrapper, configuration, layers
    model_cfg = weights.ESM2_SIZES[rotary]["config"]
    if args.layers is None:
        args.layers = model_cfg["n_layers"]
    if not torch.cuda.is_available():
        raise SystemExit("esm2_bench: no GPU visible -- nothing is measured without one")
    L_ = _lib.lib()

    def build(cls, base, precision="bf16", **over):
        cfg = weights.make_config(base, **dict(dict(n_layers=args.layers), **over))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m = cls(state_dict=weights.synthetic_state_dict(cfg, seed=0), config=cfg, precision=precision)
        return esm_sampler.ESM_sampler(m, device="cuda:0")

    def build_size(cli, **kw):
        return build(getattr(models, weights.ESM2_SIZES[cli]["wrapper"]), weights.ESM2_SIZES[cli]["config"], **kw)

    def in_use():
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info()          # hipMemGetInfo
        return int(total - free)

    device_bytes = {}

    if args.size == "35m":
        samplers = {rotary: build_size(rotary), "esm2_150m": build_size("esm2_150m", n_layers=30 if args.layers == 12 else args.layers)}
        model_cfg = dict(model_cfg, d_model=model_cfg["n_heads"] * weights.embedded_slot(model_cfg))      # the run shape
    elif args.size == "15b":
        import gc
        half = args.layers // 2 if args.layers < 48 else 0
        if args.layers < 48 and (args.layers < 4 or args.layers % 4):
            raise SystemExit("esm2_bench --size 15b: --layers below 48 must be a multiple of 4 (L, L / 2 and L / 4 layers are built)")
        # the strict mode's weights first, at L / 4 and L / 2 layers (or 1 and 2 of the full model), then released
        a, b = (args.layers // 4, args.layers // 2) if half else (1, 2)
        base0 = in_use()
        m_a = build_size(rotary, precision="fp32", n_layers=a)
        used_a = in_use()
        m_b = build_size(rotary, precision="fp32", n_layers=b)
        used_b = in_use()
        device_bytes["fp32"] = {"layers": [a, b], "weights_bytes": [used_a - base0, used_b - used_a]}
        pl = (device_bytes["fp32"]["weights_bytes"][1] - device_bytes["fp32"]["weights_bytes"][0]) / float(b - a)
        device_bytes["fp32"]["weights_bytes_48_layers_extrapolated"] = int(device_bytes["fp32"]["weights_bytes"][1] + (48 - b) * pl)
        del m_a, m_b
        gc.collect()
        base1 = in_use()
        samplers = {}
        if half:
            samplers["esm2_15b_half"] = build_size(rotary, n_layers=half)
        used_h = in_use()
        samplers["esm2_15b"] = build_size(rotary)
        used_f = in_use()
        device_bytes["bf16"] = {"layers": [half, args.layers] if half else [args.layers],
                                "weights_bytes": [used_h - base1, used_f - used_h] if half else [used_f - base1],
                                "in_use_before_the_bf16_engines": base1}
        if half:
            pl = ((used_f - used_h) - (used_h - base1)) / float(args.layers - half)
            device_bytes["bf16"]["weights_bytes_48_layers_extrapolated"] = int((used_f - used_h) + (48 - args.layers) * pl)
    elif args.size == "650m":
        samplers = {"esm1b": build(models.ESM1b, weights.ESM1B_CONFIG), rotary: build_size(rotary)}
    else:
        samplers = {rotary: build_size(rotary)}
    d_model, d_ffn = model_cfg["d_model"], model_cfg["d_ffn"]

    def job(s, B, L, P, iters):
        """-> a closure that runs `iters` Gibbs iterations of B chains from fresh device buffers and synchronises"""
        T = L + 2
        rng = np.random.default_rng(1234)
        tok = np.concatenate([np.zeros((B, 1), np.int64), rng.integers(4, 24, (B, L)), np.full((B, 1), 2)], axis=1).astype(np.int32)
        r = pyrandom.NativePyRandom()
        r.seed(0)
        table = sharding.global_position_table(r, list(range(1, L + 1)), P, iters, B)
        params = _lib.make_sample_params(True, 32, 0, float("inf"), 1.0, s.valid_aa_idx, rng_seed=0)
        d_tok = torch.from_numpy(tok).cuda()
        d_idx = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)).cuda()
        lm = s.model.model

        def run():
            _lib.check(L_.pg_esm_gibbs_run_device(lm.handle, ctypes.c_void_p(d_tok.data_ptr()), B, T, ctypes.c_void_p(d_idx.data_ptr()),
                                                  iters, P, ctypes.byref(params), None, None))
            lm.synchronize()
        return run

    out = {"tool": "esm2_bench", "size": args.size, "d_model": d_model, "device": torch.cuda.get_device_name(0), "precision": "bf16",
           "layers": args.layers,
           **({"d_model_live": 480, "head_width": 24, "head_slot": 32, "esm2_150m_layers": samplers["esm2_150m"].model.cfg["n_layers"]}
              if args.size == "35m" else {}),
           "iters": args.iters, "warmup": args.warmup, "rounds": args.rounds, "shapes": {}}
    for name, B, L, P in SHAPES:
        T = L + 2
        rec = {"chains": B, "tokens": T, "positions": P}
        timed = {k: job(s, B, L, P, args.iters) for k, s in samplers.items()}
        warm = {k: job(s, B, L, P, max(args.warmup, 3)) for k, s in samplers.items()}
        for k in samplers:
            warm[k]()
        ms = {k: [] for k in samplers}
        for _ in range(args.rounds):
            for k in samplers:                      # same order every round: ESM-1b, then ESM-2
                t0 = time.perf_counter()
                timed[k]()
                ms[k].append((time.perf_counter() - t0) * 1e3 / args.iters)
        for k in samplers:
            rec[k + "_ms_per_iteration"] = round(statistics.median(ms[k]), 4)
            rec[k + "_ms_per_iteration_rounds"] = [round(v, 4) for v in ms[k]]
        if "esm2_15b_half" in samplers:
            full, hv, Lf = rec["esm2_15b_ms_per_iteration"], rec["esm2_15b_half_ms_per_iteration"], args.layers
            rec["ms_per_layer"] = round((full - hv) / (Lf - Lf // 2), 4)
            rec["ms_per_iteration_48_layers_extrapolated"] = round(full + (48 - Lf) * (full - hv) / (Lf - Lf // 2), 3)
        if name == SHAPES[0][0] and device_bytes:
            device_bytes["in_use_after_the_config2_runs"] = in_use()
        if "esm1b" in samplers:
            rec["esm2_over_esm1b"] = round(rec["esm2_ms_per_iteration"] / rec["esm1b_ms_per_iteration"], 4)
        # the rotation and the LayerNorm launches, by HIP events, in a run of their own
        lm = samplers[rotary].model.model
        prof = job(samplers[rotary], B, L, P, args.prof_iters)
        lm.prof_enable(True)
        lm.prof_reset()
        prof()
        rope_ms, rope_n = lm.prof_get("rope")
        ln_ms, ln_n = lm.prof_get("layernorm")
        att_ms, att_n = lm.prof_get("attention")
        gemm = {c: lm.prof_get(c) for c in ("gemm_qkv", "gemm_out", "gemm_fc1", "gemm_fc2")}
        gemm_kernels = {c: lm.prof_get_kernels(c) for c in gemm}
        lm.prof_enable(False)
        rows = B * T
        if att_n:
            rec["attention_ms_per_launch"] = round(att_ms / att_n, 5)
            rec["attention_ms_per_iteration"] = round(att_ms / args.prof_iters, 4)
        rec["rope_launches_per_iteration"] = rope_n // args.prof_iters
        rec["rope_ms_per_launch"] = round(rope_ms / max(rope_n, 1), 5)
        rec["rope_ms_per_iteration"] = round(rope_ms / args.prof_iters, 4)
        rope_bytes = rows * 2 * d_model * 2 * 2
        rec["rope_bytes_per_launch"] = rope_bytes
        rec["rope_GBps"] = round(rope_bytes / (rope_ms / max(rope_n, 1) * 1e-3) / 1e9, 1) if rope_ms > 0 else None
        if ln_n:
            # the trunk's LayerNorm launches see all token rows except the pruned last layer's (the selected rows only): bytes by launch
            # count would overstate them, so only full-row launches are priced -- 2 per layer, minus the pruned layer's second
            rec["layernorm_ms_per_launch"] = round(ln_ms / ln_n, 5)
            rec["layernorm_launches"] = ln_n
            rec["layernorm_GBps_if_full_rows"] = round(rows * d_model * 6 / (ln_ms / ln_n * 1e-3) / 1e9, 1)
        # the classes whose launches see every token row (the pruned last layer's projections fall under "gemm_other")
        nk = {"gemm_qkv": (3 * d_model, d_model), "gemm_out": (d_model, d_model), "gemm_fc1": (d_ffn, d_model), "gemm_fc2": (d_model, d_ffn)}
        for c, (g_ms, g_n) in gemm.items():
            if g_n:
                n, k = nk[c]
                rec[c] = {"launches": g_n, "ms_per_launch": round(g_ms / g_n, 5), "N": n, "K": k, "kernels": gemm_kernels[c],
                          "TFLOPs": round(2.0 * rows * n * k / (g_ms / g_n * 1e-3) / 1e12, 1)}
        out["shapes"][name] = rec
    if device_bytes:
        out["device_bytes"] = device_bytes
    if args.size in ("150m", "8m"):
        # the head-32 kernels against the head-64 ones (8m: head 16 against head 32): same process, alternating, config-2 shape
        name, B, L, P = SHAPES[0]
        rows = B * (L + 2)
        if args.size == "8m":
            trio = {"h20x16_d320": build_size("esm2_8m", n_layers=3), "h20x32_d640": build_size("esm2_150m", n_layers=3)}
        else:
            trio = {"h20x32_d640": build_size("esm2_150m", n_layers=3), "h20x64_d1280": build_size("esm2", n_layers=3),
                    "h10x64_d640": build_size("esm2", n_layers=3, d_model=640, d_ffn=2560)}
        jobs = {k: job(s, B, L, P, args.prof_iters) for k, s in trio.items()}
        for k in trio:
            jobs[k]()                                   # warm-up of every shape, unprofiled
        per = {k: {"attention": [], "rope": []} for k in trio}
        for _ in range(max(args.rounds, 3)):
            for k, s in trio.items():
                lm = s.model.model
                lm.prof_enable(True)
                lm.prof_reset()
                jobs[k]()
                for c in ("attention", "rope"):
                    c_ms, c_n = lm.prof_get(c)
                    per[k][c].append(c_ms / max(c_n, 1))
                lm.prof_enable(False)
        cmp = {"shape": name, "rounds": max(args.rounds, 3)}
        for k in trio:
            dm = trio[k].model.cfg["d_model"]
            r_ms = statistics.median(per[k]["rope"])
            cmp[k] = {"attention_ms_per_launch": round(statistics.median(per[k]["attention"]), 5),
                      "attention_ms_per_launch_rounds": [round(v, 5) for v in per[k]["attention"]],
                      "rope_ms_per_launch": round(r_ms, 5), "rope_ms_per_launch_rounds": [round(v, 5) for v in per[k]["rope"]],
                      "rope_GBps": round(rows * 2 * dm * 2 * 2 / (r_ms * 1e-3) / 1e9, 1) if r_ms > 0 else None}
        out["head16_vs_head32" if args.size == "8m" else "head32_vs_head64"] = cmp
    print(json.dumps(out))


if __name__ == "__main__":
    main()
