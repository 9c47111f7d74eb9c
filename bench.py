#!/usr/bin/env python3
"""Headline benchmark: sampled positions / second of the ESM-1b Gibbs hot path (BASELINE.json configs[1] at N = 1,
configs[2] -- the same 256 chains sharded over N GPUs -- at N > 1).

  python bench.py --gpus N --steps K --warmup W
      N = 1: runs in this process.  N > 1 without a launcher: re-executes itself under
      `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ...`; the driver's own
      torchrun command line works too (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* are read from the environment).

A "step" is one Gibbs iteration over the chains resident on one GPU: draw P = 25 positions for each chain of L = 256
residues (CPython-exact random.sample stream, native), scatter <mask>, run the 33-layer ESM-1b forward (T = 258 tokens
per chain), evaluate the LM head at the sampled rows, draw tokens (top_k = 0, temperature = 1, burnin = inf) and write
them back -- all inside one C-ABI call (pg_esm_gibbs_run_device) with the token buffer resident in HBM.  Weights are
seeded synthetic weights of the ESM-1b architecture (no checkpoints offline); throughput does not depend on their values.

Multi-GPU (BASELINE config 3): the SAME 256 chains split contiguously, GPU g owns chains
[g*256/N, (g+1)*256/N) -- "scaling": "strong".  Chains never interact, so there is no data-path collective; the only
collective is one RCCL all-gather of the final token buffers.  Every rank derives its slice of the position table from the
one CPython-exact stream and token draws are keyed by global chain id, so the gathered result is bit-identical to the
N = 1 result: with `--full` rank 0 re-runs the whole job on its own GPU after the timed region and asserts that
(`verified_vs_single_gpu`).
`--weak` keeps 256 chains per GPU instead.

`--dump-outputs DIR` writes what the last timed step handed back -- the token buffer, and that step's logits and draws at the
sampled positions -- as DIR/<name>.npy (float32) after the timed region.  Every input is seeded (seeds, weights, position stream,
draws), so equal arguments give equal inputs and two builds can be compared array for array.

Output: ONE JSON line (rank 0): `metric`, `value`, `unit`, `higher_is_better`, `dtype`, `ms_per_step` and the run's configuration.
A plain run sets up, warms up, times the K steps, writes `--dump-outputs` if asked and prints that line -- nothing else runs, so
the headline figure costs no more than it needs.
`--full` runs every other leg and check after the timed region (each has a `--no-*` option there) and adds to the line
  roofline     -- the GEMM kernel family (96.5 % of the FLOPs): executed FLOPs / HIP-event time on the engine's stream
  strict_mode  -- (N = 1) the same workload in the parity mode (PG_PREC_FP32: split-bf16 x3 GEMMs and attention): its
                  positions/s and its measured max |logit error| against the fp32 oracle -- the mode north_star's 1e-3
                  tolerance refers to; `bf16_max_abs_logit_err` is the same measurement for the benchmarked mode
  value_at_tolerance -- strict-mode positions/s with its measured max |logit error|: the throughput at north_star's 1e-3
  cpu_baseline -- BASELINE.md 3: 8 chains x 2 Gibbs iterations of the same workload in torch CPU ops on all host cores
                  (oracle/esm_forward_torch.py, the reference's CPU path restated: fair-esm is not installed), config 1 in full,
                  the reference-style per-position sampling-loop cost; and the numpy fp32 oracle as the checker of the engines'
                  logits (`logit_check`) -- the checker and the baseline, never the product
"""
import argparse
import ctypes
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MFMA_BF16_PEAK_TFLOPS = 2500.0     # dense bf16 MFMA peak of the MI355X (see roofline.peak_note)
DUMP_MAX_BYTES = 64 << 20          # --dump-outputs: all files together
TOTAL_CHAINS = 256                 # BASELINE.json configs[1] / configs[2]
SYNTH_KW = dict(std=0.025, embed_std=0.3, ln_jitter=0.1)     # seeded synthetic weights at a realistic logit scale (std ~ 10)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--weak", action="store_true", help="weak scaling: 256 chains PER GPU instead of 256 in total")
    ap.add_argument("--chains", type=int, default=TOTAL_CHAINS, help="chains in total (per GPU with --weak)")
    ap.add_argument("--length", type=int, default=256)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run every leg and check around the headline: host-buffer entry, roofline, "
                         "shard proxy, strict and fp16 modes, config 1, CPU baseline and logit check, ESM-MSA-1b; N > 1: the "
                         "single-GPU re-run and the C-ABI gather.  The --no-* options and --native-gather choose among them and "
                         "mean nothing without it")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "fp32"],
                    help="mode of the timed run: bf16 = throughput mode (the headline), fp16 = the same kernels with fp16 operands, "
                         "fp32 = strict parity mode")
    ap.add_argument("--no-fp16", action="store_true", help="skip the fp16-operand leg (N = 1)")
    ap.add_argument("--layers", type=int, default=None, help="debug only: fewer layers (the JSON then says so)")
    ap.add_argument("--greedy-after-burnin", action="store_true",
                    help="SURVEY 8d variant: top_k=1, burnin=25 (argmax after 25 sampled iterations) instead of all-sampling")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"], help="nccl = RCCL over xGMI; gloo for dry runs")
    ap.add_argument("--oversubscribe", action="store_true", help="testing: ranks share GPUs (LOCAL_RANK mod device count); implies gloo")
    ap.add_argument("--dry-run", action="store_true",
                    help="no GPU work at all: launcher, sharding, position tables and the gather only (CPU container check)")
    ap.add_argument("--no-verify", action="store_true", help="skip the N > 1 bit-equality check against a single-GPU run")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-strict", action="store_true", help="skip the strict-mode leg (N = 1)")
    ap.add_argument("--no-host-entry", action="store_true", help="skip the host-buffer entry-point leg (PCIe-inclusive rate; N = 1)")
    ap.add_argument("--no-msa", action="store_true", help="skip the ESM-MSA-1b legs (BASELINE configs 4 and 5; N = 1)")
    ap.add_argument("--native-gather", action="store_true",
                    help="after the timed region: repeat the final gather through the C ABI (pg_comm_* / pg_gather_tokens, RCCL opened by "
                         "libpgibbs.so itself) and require the same tokens (`native_gather_equal`); RCCL backend only.  Since round 6 this "
                         "is the DEFAULT whenever more than one rank runs on the nccl backend; the flag forces it at world size 1 too")
    ap.add_argument("--no-native-gather", action="store_true", help="N > 1 on nccl: skip the C-ABI repeat of the gather")
    ap.add_argument("--no-shard-proxy", action="store_true",
                    help="N = 1: skip the shard_proxy leg (128 / 64 / 32 chains of the 256-chain job on this one GPU: what one GPU of "
                         "BASELINE config 3 runs at 2 / 4 / 8 GPUs)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps: write what the last timed step handed back as DIR/<name>.npy (float32) -- tokens "
                         "[chains, L + 2], the final token buffer of the timed job itself; last_step_logits [chains, P, vocab] and "
                         "last_step_sampled_tokens [chains, P], the optional outputs of the same native call for that step (from an "
                         "untimed replay of the job that must end in the same tokens).  Inputs are seeded: equal arguments give equal "
                         "inputs, so two builds can be compared array for array.  Past 64 MB a fixed seeded subset of the chains")
    ap.add_argument("--force-dist", action="store_true",
                    help="N = 1: still create the torch.distributed process group (world_size 1) and run the final all-gather "
                         "through it, so that the RCCL path is executed on a single GPU")
    args = ap.parse_args(argv)
    if not args.full:              # a plain run: the headline and nothing else -- every leg after the timed steps is off
        args.no_verify = args.no_cpu_baseline = args.no_roofline = args.no_strict = args.no_fp16 = args.no_host_entry = True
        args.no_msa = args.no_shard_proxy = args.no_native_gather = True
        args.native_gather = False
    return args


def self_launch(args):
    """`python bench.py --gpus N` with no launcher around it: one rank per GPU under torch.distributed.run."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def gemm_flops_per_iter(cfg, n_tokens, n_sampled):
    d, f, nl = cfg["d_model"], cfg["d_ffn"], cfg["n_layers"]
    return nl * 2.0 * (4 * d * d + 2 * d * f) * n_tokens + 2.0 * d * d * n_sampled


def total_flops_per_iter(cfg, n_tokens, T, n_sampled):
    """GEMM + attention contractions, 2 FLOP/MAC, LM head at the sampled rows only."""
    d, V = cfg["d_model"], cfg["vocab"]
    return gemm_flops_per_iter(cfg, n_tokens, n_sampled) + cfg["n_layers"] * 4.0 * T * d * n_tokens + 2.0 * V * d * n_sampled


GEMM_CLASS_PATTERNS = (            # projection -> substring of the rocprofv3 kernel name (tools/pmc_traffic.sh writes the same table
    ("gemm_qkv", "gemm_bf16_w16_kernel<0"),            # into the JSON as "classes"; that one wins when present)
    ("gemm_fc1", "gemm_bf16_w16_kernel<1"),
    ("gemm_out", "gemm_bf16_pp_kernel<2, 0, 4"),
    ("gemm_fc2", "gemm_bf16_pp_kernel<2, 0, 2"))


def measured_gemm_traffic():
    """Fabric (L2 <-> Infinity Cache/HBM) bytes per GEMM launch of THIS workload (ESM-1b config 2) from the committed PMC passes
    (tools/pmc_traffic.sh: separate rocprofv3 --pmc runs of this very script; since round 6 from the request counters themselves --
    reads = 128-B requests x 128, writes = requests x 64 as a lower bound, checked on kernels whose bytes are known exactly; the
    LayerNorm-derived scale factors of rounds 1-5 made every read 22 % too high).  The newest profiles/rNN_hbm_traffic_pmc.json wins -- the ESM-MSA-1b files
    (rNN_msa_hbm_traffic_pmc.json) are another workload and are never read here.  Returns (launch-weighted bytes per launch,
    {projection: bytes per launch}, file name); (None, {}, None) when there is no file.  PMC counters cannot be collected from
    inside the timed process, so this is a committed measurement of the same command, not of the run that prints it."""
    import glob
    paths = sorted(p for p in glob.glob(os.path.join(ROOT, "profiles", "r*_hbm_traffic_pmc.json"))
                   if "_msa_" not in os.path.basename(p))
    if not paths:
        return None, {}, None
    doc = json.load(open(paths[-1]))
    k = doc["kernels"]
    classes = doc.get("classes") or {}
    per = {}
    for cls, pat in GEMM_CLASS_PATTERNS:
        names = [classes[cls]] if classes.get(cls) in k else [n for n in k if pat in n]
        if names:
            v = k[names[0]]
            per[cls] = {"launches": v["launches"], "read": 1e6 * v["read_MB_per_launch"], "write": 1e6 * v["write_MB_per_launch"]}
    if not per:
        return None, {}, os.path.basename(paths[-1])
    n = sum(v["launches"] for v in per.values())
    return sum(v["launches"] * (v["read"] + v["write"]) for v in per.values()) / n, per, os.path.basename(paths[-1])


def pmc_derived():
    """north_star's evidence words -- matrix-pipe (MFMA) utilisation and L2 hit rate of the hot kernels -- derived from the newest
    committed profiles/rNN_gemm_pmc_counters.txt (tools/pmc_bench.sh: three rocprofv3 --pmc passes per kernel; PMC cannot be read
    from inside the timed process, so like roofline.traffic this is a committed measurement of the same kernels, with its file name):
      mfma_util = SQ_VALU_MFMA_BUSY_CYCLES / (n_SIMD x GRBM_GUI_ACTIVE / n_XCD)   (busy matrix-pipe cycles per SIMD / kernel cycles)
      l2_hit    = TCC_HIT / (TCC_HIT + TCC_MISS);   l2_read_latency_cycles = TCP_TCC_READ_REQ_LATENCY / TCP_TCC_READ_REQ"""
    import ast
    import glob
    paths = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_gemm_pmc_counters.txt")))
    if not paths:
        return None
    kern, cur = {}, None
    for ln in open(paths[-1]):
        ln = ln.strip()
        if ln.startswith("== "):
            cur = kern.setdefault(ln[3:].strip(), {})
        elif ln.startswith("pass ") and cur is not None and "{" in ln:
            try:
                cur.update(ast.literal_eval(ln[ln.index("{"):ln.rindex("}") + 1]))
            except (ValueError, SyntaxError):
                pass
    out = {"source": os.path.basename(paths[-1]), "kernels": {}}
    for k, c in kern.items():
        d = {}
        if c.get("GRBM_GUI_ACTIVE") and "SQ_VALU_MFMA_BUSY_CYCLES" in c:
            d["mfma_util"] = c["SQ_VALU_MFMA_BUSY_CYCLES"] / 1024.0 / (c["GRBM_GUI_ACTIVE"] / 8.0)
        if c.get("TCC_HIT") is not None and (c.get("TCC_HIT", 0) + c.get("TCC_MISS", 0)) > 0:
            d["l2_hit"] = c["TCC_HIT"] / (c["TCC_HIT"] + c["TCC_MISS"])
        if c.get("TCP_TCC_READ_REQ"):
            d["l2_read_latency_cycles"] = c["TCP_TCC_READ_REQ_LATENCY"] / c["TCP_TCC_READ_REQ"]
        if c.get("SQ_WAVE_CYCLES"):
            d["wave_cycles_waiting"] = c.get("SQ_WAIT_ANY", 0) / c["SQ_WAVE_CYCLES"]
        out["kernels"][k] = d
    return out


def host_cpu_quota():
    """What the host really grants this process: logical CPUs, the scheduler affinity mask, and the cgroup CPU quota (cgroup v2
    cpu.max / v1 cfs_quota_us) in CPUs -- the MI355X boxes report 256 logical CPUs but a container may be capped far below."""
    q = {"logical_cpus": os.cpu_count()}
    try:
        q["sched_affinity_cpus"] = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        pass
    try:
        a, b = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        q["cgroup_cpu_max"] = "%s %s" % (a, b)
        q["cgroup_quota_cpus"] = None if a == "max" else float(a) / float(b)
    except (OSError, ValueError):
        try:
            a = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            b = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            q["cgroup_quota_cpus"] = None if a < 0 else a / b
        except (OSError, ValueError):
            q["cgroup_quota_cpus"] = "unknown"
    return q


def cpu_baseline(cfg, sd, lm, lm_strict, B, L, P, valid_idx, gpu_cfg1, lm_f16=None, chains=8, iters=2, check_chains=2):
    """the reference's CPU path -- fair-esm fp32 under PyTorch, all host cores -- as this repo's torch-CPU
    restatement (oracle/esm_forward_torch.py; fair-esm itself is not installed and reference files never travel to the GPU box):
    `chains` = 8 chains x `iters` = 2 full Gibbs iterations of config 2 (mask, the WHOLE forward incl. the LM head on every row as
    `model(batch)["logits"]` computes it, then the reference's per-position Python draw loop), linear in chains.  Config 1 in full.
    Separately, the numpy fp32 oracle (the checker, never the product) scores the engines' logits on `check_chains` chains."""
    import numpy as np
    import torch
    from oracle import draw as odraw
    from oracle import esm_forward_torch as eft
    from oracle.esm_forward import EsmConfig, esm1b_trunk, lm_head
    ocfg = EsmConfig(vocab=cfg["vocab"], d_model=cfg["d_model"], n_layers=cfg["n_layers"], n_heads=cfg["n_heads"],
                     d_ffn=cfg["d_ffn"], max_pos=cfg["max_positions"])
    wt = eft.torch_state(sd)
    rng = np.random.default_rng(1234)
    # Threads: the fastest count on THIS host, found by a sweep over one layer of the same batch -- not blindly "all of them":
    # on the 256-logical-CPU hosts of the MI355X boxes torch's OpenMP pool collapses past ~32 threads (8 x 258 tokens, 4 layers:
    # 16 threads 877 GFLOP/s, 64: 425, 256: 22 -- profiles/r05_cpu_baseline_thread_sweep.txt), so all-cores would flatter the GPU.
    one = EsmConfig(vocab=ocfg.vocab, d_model=ocfg.d_model, n_layers=1, n_heads=ocfg.n_heads, d_ffn=ocfg.d_ffn, max_pos=ocfg.max_pos)
    tok_sweep = np.concatenate([np.zeros((chains, 1), np.int64), rng.integers(4, 24, (chains, L)), np.full((chains, 1), 2)], axis=1)
    sweep, n_cpu = {}, os.cpu_count() or 1
    for nt in sorted({min(n_cpu, c) for c in (4, 8, 16, 32, 64, 128, 256)}):
        torch.set_num_threads(nt)
        eft.esm1b_forward(wt, one, tok_sweep[:1, :16])
        best = float("inf")
        for _ in range(2):
            t0 = time.perf_counter()
            eft.esm1b_forward(wt, one, tok_sweep)
            best = min(best, time.perf_counter() - t0)
        sweep[nt] = best
        if sweep[nt] > 2.5 * min(sweep.values()):
            break                                                  # past the knee: more threads only get slower
    cores = min(sweep, key=sweep.get)
    torch.set_num_threads(cores)

    def seeds(b, T_len):
        return np.concatenate([np.zeros((b, 1), np.int64), rng.integers(4, 24, (b, T_len)), np.full((b, 1), 2)], axis=1)

    def targets(b, T_len, n_pos, n_it):
        return [[sorted(rng.choice(np.arange(1, T_len + 1), n_pos, replace=False).tolist()) for _ in range(b)] for _ in range(n_it)]

    # ---- config 2 sample: `chains` chains x `iters` iterations, top_k = 0, temperature = 1, all-sampling (burnin = inf)
    eft.gibbs_iterations(wt, ocfg, seeds(1, 16), targets(1, 16, 2, 1), valid_idx)                  # thread pool / allocator warm-up
    tok0, tg = seeds(chains, L), targets(chains, L, P, iters)
    t0 = time.perf_counter()
    _, t_fwd, t_loop = eft.gibbs_iterations(wt, ocfg, tok0, tg, valid_idx, top_k=0, temperature=1.0, sample=True)
    t = time.perf_counter() - t0
    out = {"value": chains * P * iters / t, "unit": "sampled positions/s", "cores": int(cores), "kind": "port",
           "sample": "%d of %d chains x %d Gibbs iterations (L=%d, P=%d; BASELINE.md section 3), fp32 torch-CPU restatement of the "
                     "reference path (full forward + LM head on every row + per-position torch draw loop), %d threads = the fastest count of a sweep on this host, "
                     "%.1f s (forward %.1f s, draw loop %.2f s); chains are independent, so the whole-batch figure is the same rate"
                     % (chains, B, iters, L, P, cores, t, t_fwd, t_loop),
           "host_logical_cpus": n_cpu, "host_cpu_quota": host_cpu_quota(), "thread_sweep_s_per_layer": {str(k_): round(v_, 4) for k_, v_ in sweep.items()},
           "seconds_per_iteration_scaled_to_%d_chains" % B: t / iters * B / chains,
           "forward_gflops_per_s": total_flops_per_iter(cfg, chains * (L + 2), L + 2, chains * (L + 2)) * iters / t_fwd / 1e9}

    # ---- the numpy oracle as CHECKER: logits of the engine modes at the sampled rows of `check_chains` masked chains
    b = check_chains
    tokc = seeds(b, L)
    idx = np.stack([rng.choice(np.arange(1, L + 1), P, replace=False) for _ in range(b)])
    for i in range(b):
        tokc[i, idx[i]] = cfg["mask_idx"]
    x = esm1b_trunk(sd, ocfg, tokc)
    ref = lm_head(sd, np.stack([x[i, idx[i]] for i in range(b)]).reshape(b * P, -1))
    check = {"chains": b, "rows": int(b * P), "logit_std": float(ref.std()), "checker": "oracle/esm_forward.py (numpy fp32)"}

    def dist20(lg):                                   # the distribution generate_step samples from: softmax over the valid residues
        z = lg[:, valid_idx].astype(np.float64)
        z = np.exp(z - z.max(axis=1, keepdims=True))
        return z / z.sum(axis=1, keepdims=True)
    p_ref = dist20(ref)
    for name, eng in (("bf16", lm), ("fp16", lm_f16), ("fp32", lm_strict)):
        if eng is None:
            continue
        full = eng.forward_logits(tokc)
        got = np.stack([full[i, idx[i]] for i in range(b)]).reshape(b * P, -1)
        err = np.abs(got - ref)
        check[name + "_max_abs_logit_err"] = float(err.max())
        check[name + "_mean_abs_logit_err"] = float(err.mean())
        q = dist20(got)
        kl = (q * (np.log(q + 1e-300) - np.log(p_ref + 1e-300))).sum(axis=1)
        check[name + "_argmax_agreement"] = float((got[:, valid_idx].argmax(1) == ref[:, valid_idx].argmax(1)).mean())
        check[name + "_kl_sampled_dist_mean"] = float(kl.mean())
        check[name + "_kl_sampled_dist_max"] = float(kl.max())
    got_t = eft.esm1b_forward(wt, ocfg, tokc).numpy()
    check["torch_baseline_vs_checker_max_abs"] = float(np.abs(np.stack([got_t[i, idx[i]] for i in range(b)]).reshape(b * P, -1) - ref).max())
    out["logit_check"] = check

    # ---- BASELINE config 1 in full on the CPU: one chain, L = 25, P = 2, 20 iterations (top_k = 1, burnin = 10)
    tok1 = seeds(1, 25)
    t0 = time.perf_counter()
    for it in range(20):
        tok1, _, _ = eft.gibbs_iterations(wt, ocfg, tok1, targets(1, 25, 2, 1), valid_idx, top_k=1, temperature=1.0, sample=it < 10)
    tc1 = time.perf_counter() - t0
    out["config1"] = {"cpu_positions_per_s": 40 / tc1, "cpu_ms_per_iter": 1e3 * tc1 / 20,
                      "workload": "ESM-1b, 1 chain x L=25 (T=27), P=2, 20 iterations, top_k=1, burnin=10, torch CPU, %d threads" % cores}
    if gpu_cfg1:
        out["config1"].update(gpu_cfg1)

    # ---- reference-style sampling loop alone: the per-position torch draw the reference runs in Python
    # (esm_sampler.py:225-234), on the checker's logits
    rows = torch.from_numpy(ref)
    vi = torch.as_tensor(valid_idx)
    n = min(len(ref), 400)
    t0 = time.perf_counter()
    for i in range(n):
        eft.generate_step(rows, i, top_k=0, temperature=1.0, sample=True, valid_idx=vi)
    per = (time.perf_counter() - t0) / n
    out["reference_style_position_loop"] = {"us_per_position_one_core": 1e6 * per, "s_per_iteration_at_config2": per * B * P,
                                            "note": "per-position torch draw (topk + Categorical) as in esm_sampler.py:8-45,225-234, %d calls timed" % n}
    return out


def main():
    args = parse_args()
    if args.gpus > 1 and "RANK" not in os.environ:
        raise SystemExit(self_launch(args))

    import numpy as np
    import torch
    from protein_gibbs_sampler_amd import _lib, models, pyrandom, sharding, weights

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    dry = args.dry_run
    backend = "gloo" if (dry or args.oversubscribe) else args.backend
    dev = None
    if not dry:
        n_dev = torch.cuda.device_count()
        if n_dev == 0:
            raise SystemExit("bench.py needs an MI355X (use --dry-run for the launcher/sharding plumbing check)")
        if local_rank >= n_dev and not args.oversubscribe:
            raise SystemExit("rank %d has no GPU (%d visible); --oversubscribe shares GPUs for testing" % (local_rank, n_dev))
        dev = torch.device("cuda", local_rank % n_dev)
        torch.cuda.set_device(dev)
    dist = None
    if world > 1 or args.force_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:
            s_ = socket.socket()
            s_.bind(("127.0.0.1", 0))
            os.environ["MASTER_PORT"] = str(s_.getsockname()[1])
            s_.close()
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group("gloo")

    cfg = dict(weights.ESM1B_CONFIG)
    if args.layers:
        cfg["n_layers"] = args.layers
    L = args.length
    T = L + 2
    P = int(L * 10 / 100)
    K, W = args.steps, args.warmup
    B_total = args.chains * world if args.weak else args.chains
    lo, hi = sharding.shard_range(B_total, world, rank)
    B = hi - lo
    counts = [sharding.shard_range(B_total, world, r)[1] - sharding.shard_range(B_total, world, r)[0] for r in range(world)]

    valid_idx = list(range(4, 24))                      # ACDEFGHIKLMNPQRSTVWY in the ESM-1b alphabet (sorted ids)
    top_k, burnin = (1, 25.0) if args.greedy_after_burnin else (0, float("inf"))
    # seeds: B_total chains, L residues i.i.d. uniform over the 20 amino acids, numpy default_rng(1234)
    rng = np.random.default_rng(1234)
    aa = rng.integers(0, 20, (B_total, L))
    tok_all = np.concatenate([np.zeros((B_total, 1), np.int64), np.asarray(valid_idx)[aa], np.full((B_total, 1), 2)],
                             axis=1).astype(np.int32)
    population = list(range(1, L + 1))

    sd = lm = L_ = None
    if not dry:
        # realistic-scale synthetic weights (logit std ~ 10, max |logit| ~ 40 -- what the full-size parity tests use): the
        # logit-error figures this line reports are then the honest ones (N(0, 0.02) weights give logit std 0.7 and errors 15x smaller)
        sd = weights.synthetic_state_dict(cfg, seed=0, **SYNTH_KW)
        wrapper = models.ESM1b(state_dict=sd, config=cfg, precision=args.precision)
        lm = wrapper.model.to(str(dev))
        L_ = _lib.lib()
        assert valid_idx == sorted(wrapper.alphabet.get_idx(t) for t in "ACDEFGHIKLMNPQRSTVWY")
        stream = torch.cuda.current_stream(dev)
        _lib.check(L_.pg_engine_set_stream(lm.handle, ctypes.c_void_p(stream.cuda_stream)))

    class Job:
        """The Gibbs job on chains [c_lo, c_hi) of the B_total: its own position stream (CPython-exact, seed 0; every rank
        generates the table for ALL chains and slices its block) and token buffer; run(n) advances n iterations."""

        def __init__(self, engine, c_lo, c_hi):
            self.engine, self.c_lo, self.c_hi, self.done = engine, c_lo, c_hi, 0
            self.pos_rng = pyrandom.NativePyRandom()
            self.pos_rng.seed(0)
            t = torch.from_numpy(tok_all[c_lo:c_hi].copy())
            self.tok = t if dry else t.to(dev).contiguous()
            self.params = _lib.make_sample_params(True, cfg["mask_idx"], top_k, burnin, 1.0, valid_idx, rng_seed=0, rng_stream=0,
                                                  row_id_base=c_lo)

        def run(self, n_iters, logits=None, sampled=None):
            """logits [n_iters, chains, P, vocab] fp32 / sampled [n_iters, chains, P] int32: the call's optional per-step outputs."""
            table = sharding.global_position_table(self.pos_rng, population, P, n_iters, B_total)
            mine = sharding.local_slice(table, self.c_lo, self.c_hi)
            self.params.iter_base = self.done
            self.done += n_iters
            if dry or self.c_hi == self.c_lo:
                return mine
            d_idx = torch.from_numpy(mine).to(dev, non_blocking=True)
            _lib.check(L_.pg_esm_gibbs_run_device(self.engine.handle, ctypes.c_void_p(self.tok.data_ptr()), self.c_hi - self.c_lo, T,
                                                  ctypes.c_void_p(d_idx.data_ptr()), n_iters, P, ctypes.byref(self.params),
                                                  None if logits is None else ctypes.c_void_p(logits.data_ptr()),
                                                  None if sampled is None else ctypes.c_void_p(sampled.data_ptr())))
            return d_idx                                     # caller keeps it alive until the stream is synchronised

    def barrier():
        if dist is not None:
            dist.barrier()
        if not dry:
            torch.cuda.synchronize(dev)

    if not dry:
        lm.set_job_items(B_total)     # rank's chains are a shard of the B_total-chain job: same kernel choices as the single-GPU run
    job = Job(lm, lo, hi)
    if W > 0:
        keep = job.run(W)
    barrier()
    t0 = time.perf_counter()
    keep = job.run(K)                                                  # noqa: F841
    gathered = None
    if dist is not None:
        if not dry:
            lm.synchronize()                                           # engine stream -> before the collective reads the tokens
        src = job.tok.cpu() if (backend == "gloo" and not dry) else job.tok
        gathered = sharding.gather_tokens(dist, src, counts)           # the one collective: final token buffers
    barrier()
    elapsed = time.perf_counter() - t0
    rank_elapsed = [elapsed]
    if dist is not None:
        # every rank's own clock around the same barrier-bracketed region: the MAX is the job's time, min / max show the skew
        mine_t = torch.tensor([elapsed], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        all_t = [torch.empty_like(mine_t) for _ in range(world)]
        dist.all_gather(all_t, mine_t)
        rank_elapsed = [float(t_.item()) for t_ in all_t]
        elapsed = max(rank_elapsed)
    final = (gathered if gathered is not None else job.tok).cpu().numpy()
    assert final.shape == (B_total, T)
    if not dry:
        assert ((final[:, 1:-1] >= 4) & (final[:, 1:-1] <= 23)).all(), "chains left the 20-amino-acid alphabet"

    # ---- --dump-outputs: what the last timed step handed back (rank 0, outside the timed region) ----------------------------
    dumped = None
    if args.dump_outputs and rank == 0:
        arrays = {"tokens": final}
        if not dry:
            # The timed call passes NULL for the optional per-step outputs, as the drivers do.  The same job run again from the
            # seeds -- W + K - 1 steps, then the last one with both output buffers -- gives that step's logits at the sampled
            # positions and its draws; every draw is keyed by (seed, chain, iteration), so the replay must end in the timed job's tokens.
            rj = Job(lm, 0, B_total)
            if W + K > 1:
                keep_r = rj.run(W + K - 1)
            lg = torch.empty((1, B_total, P, cfg["vocab"]), dtype=torch.float32, device=dev)
            st = torch.empty((1, B_total, P), dtype=torch.int32, device=dev)
            keep_r = rj.run(1, lg, st)                                 # noqa: F841
            torch.cuda.synchronize(dev)
            assert (rj.tok.cpu().numpy() == final).all(), "the replay for --dump-outputs ended in other tokens than the timed job"
            arrays["last_step_logits"] = lg[0].cpu().numpy()
            arrays["last_step_sampled_tokens"] = st[0].cpu().numpy()
        n_fit = (DUMP_MAX_BYTES - 4096) // (4 * sum(a[0].size for a in arrays.values()))      # 4096: the .npy headers
        if n_fit < B_total:
            rows = np.sort(np.random.default_rng(0).choice(B_total, n_fit, replace=False))
            arrays = {name: a[rows] for name, a in arrays.items()}
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, a in arrays.items():
            np.save(os.path.join(args.dump_outputs, name + ".npy"), a.astype(np.float32))
        dumped = {name: list(a.shape) for name, a in arrays.items()}

    mode = {"bf16": "bf16", "fp16": "fp16", "fp32": "bf16x3"}[args.precision]
    out = {"metric": "sampled positions/sec (whole node), ESM-1b L=256 B=256 Gibbs", "value": B_total * P * K / elapsed,
           "unit": "sampled positions/s", "n_gpus": world, "steps": K, "warmup": W, "ms_per_step": 1e3 * elapsed / K,
           "higher_is_better": True, "scaling": "weak" if args.weak else "strong", "vs_baseline": None, "dtype": mode,
           "data": "synthetic",
           "config": {"workload": "ESM_sampler ESM-1b (33 layers, d=1280) Gibbs: %d chains in total, %s per GPU x L=%d (T=%d), P=%d "
                                  "positions per chain per iteration, mask=True top_k=%d temperature=1.0 burnin=%s; %s; "
                                  "synthetic weights N(0,0.025), embeddings N(0,0.3), LayerNorm jitter 0.1 (logit std ~10)"
                                  % (B_total, "/".join(str(c) for c in sorted(set(counts))), L, T, P, top_k,
                                     "inf" if burnin == float("inf") else int(burnin),
                                     "%s MFMA operands, fp32 accumulate + fp32 residual stream" % args.precision if args.precision != "fp32"
                                     else "strict mode: split-bf16 x3 MFMA GEMMs and attention products, fp32 softmax/LayerNorm/residual"),
                      "global_batch": B_total, "seq_len": L,
                      "parallelism": "chains sharded %d-way (contiguous blocks), 1 %s all-gather at the end"
                                     % (world, "RCCL" if backend == "nccl" else "gloo"),
                      "n_layers": cfg["n_layers"]},
           "ranks_seen": 1, "backend": backend if dist is not None else None,
           "per_rank_elapsed_s": {"min": min(rank_elapsed), "max": max(rank_elapsed), "ranks": rank_elapsed,
                                  "chains_per_rank": counts}}
    if dumped is not None:
        out["dumped_outputs"] = {"dir": args.dump_outputs, "float32_arrays": dumped}
    if dist is not None:
        # counted, not assumed: every rank contributes a one to an all-reduce on the job's backend
        ones = torch.ones(1, dtype=torch.int64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(ones)
        out["ranks_seen"] = int(ones.item())
        assert out["ranks_seen"] == world, "all_reduce saw %d ranks, WORLD_SIZE is %d" % (out["ranks_seen"], world)
    if dry:
        out["dry_run"] = True
        out["value"] = 0.0
        # plumbing check: every rank's table slice equals the single-stream table, the gather restores the chain order
        random_ok = bool((final == tok_all).all())
        assert random_ok, "gather changed the chain order"
        out["verified_vs_single_gpu"] = random_ok

    # ==== from here to the printed line: the legs and checks of --full (parse_args switches all of them off in a plain run) ====
    # ---- N = 1: the same job through the HOST-buffer entry point (pg_esm_gibbs_run: tokens and position table cross PCIe inside
    # the call, the tokens come back) -- the PCIe-inclusive rate; never `value`.  W + K iterations in one call from the initial
    # tokens: the result must equal the device-pointer job's tokens bit for bit.
    if not dry and dist is None and not args.no_host_entry and lo == 0 and hi == B_total:
        r_h = pyrandom.NativePyRandom()
        r_h.seed(0)
        table_h = np.ascontiguousarray(sharding.global_position_table(r_h, population, P, W + K, B_total), dtype=np.int32)
        tok_h = np.ascontiguousarray(tok_all.copy(), dtype=np.int32)
        p_h = _lib.make_sample_params(True, cfg["mask_idx"], top_k, burnin, 1.0, valid_idx, rng_seed=0, rng_stream=0, row_id_base=0)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        lm.gibbs_run(tok_h, table_h, p_h)
        th = time.perf_counter() - t0
        out["host_buffer_entry"] = {"value": B_total * P * (W + K) / th, "unit": "sampled positions/s", "ms_per_step": 1e3 * th / (W + K),
                                    "steps": W + K, "includes": "H2D of tokens + position table, D2H of tokens (PCIe), one native call",
                                    "equals_device_pointer_job": bool((tok_h == final).all())}
        assert out["host_buffer_entry"]["equals_device_pointer_job"], "host-buffer entry point disagrees with the device-pointer one"

    # ---- opt-in: the same collective through the C ABI (no torch in the data path), outside the timed region ----
    want_native = args.native_gather or (world > 1 and not args.no_native_gather)
    if want_native and dist is not None and backend == "nccl" and not dry:
        # every rank first proves it can open RCCL through the library (pg_comm_unique_id needs nothing else); only if ALL can
        # does anybody enter the collective ncclCommInitRank -- a rank that cannot must not leave the others waiting in it
        probe = ctypes.create_string_buffer(_lib.PG_COMM_ID_BYTES)
        can = torch.tensor([1 if L_.pg_comm_unique_id(probe) == 0 else 0], dtype=torch.int64, device=dev)
        dist.all_reduce(can, op=dist.ReduceOp.MIN)
        if int(can.item()) == 1:
            comm = sharding.NativeComm(rank, world, dev.index)             # the id travels over the existing process group
            lm.synchronize()
            nat = comm.gather_tokens(job.tok, counts)
            torch.cuda.synchronize(dev)
            same = bool((nat.cpu().numpy() == final).all())
            comm.close()
            flag = torch.tensor([1 if same else 0], dtype=torch.int64, device=dev)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            out["native_gather_equal"] = bool(flag.item())
            assert out["native_gather_equal"], "pg_gather_tokens disagrees with the torch.distributed gather"
        else:
            out["native_gather_equal"] = None
            out["native_gather_note"] = "librccl.so could not be opened by libpgibbs.so on some rank: " + (L_.pg_last_error() or b"").decode()

    # ---- N > 1: the gathered tokens must equal the single-GPU result bit for bit (rank 0, outside the timed region) ----
    if not dry and dist is not None and not args.no_verify:
        if rank == 0:
            ref = Job(lm, 0, B_total)
            if W > 0:
                k2 = ref.run(W)
            k3 = ref.run(K)                                            # noqa: F841
            torch.cuda.synchronize(dev)
            same = bool((ref.tok.cpu().numpy() == final).all())
            out["verified_vs_single_gpu"] = same
            assert same, "sharded result differs from the single-GPU result"
        dist.barrier()

    def executed_flops_per_iter():
        """What one iteration launches: every layer's four GEMMs on all B*T rows except the LAST layer's out-proj / fc1 / fc2, which
        run on the B*P sampled rows only (exact pruning); attention on all rows; the LM head at the sampled rows."""
        d_, f_, nl_, V_ = cfg["d_model"], cfg["d_ffn"], cfg["n_layers"], cfg["vocab"]
        full = 2.0 * (4 * d_ * d_ + 2 * d_ * f_) * (B * T)
        last = 2.0 * (3 * d_ * d_) * (B * T) + 2.0 * (d_ * d_ + 2 * d_ * f_) * (B * P)
        gemm = (nl_ - 1) * full + last
        return gemm, gemm + nl_ * 4.0 * T * d_ * (B * T) + (2.0 * d_ * d_ + 2.0 * V_ * d_) * (B * P)

    if rank == 0 and not dry:
        n_tok, n_samp = B * T, B * P
        mult = 3 if args.precision == "fp32" else 1          # strict mode: three bf16 MFMA products per product
        out["model_tflops_per_gpu"] = total_flops_per_iter(cfg, n_tok, T, n_samp) * K / elapsed / 1e12
        out["executed_tflops_per_gpu"] = executed_flops_per_iter()[1] * mult * K / elapsed / 1e12     # last layer pruned: ~2 % below the model's
        out["frac_of_bf16_mfma_peak"] = out["executed_tflops_per_gpu"] / MFMA_BF16_PEAK_TFLOPS
    if not dry and not args.no_roofline:
        # HIP events on the engine's stream around every launch, per kernel class (pg_prof_*)
        lm.prof_enable(True)
        lm.prof_reset()
        n_prof = min(K, 3)
        keep = job.run(n_prof)
        torch.cuda.synchronize(dev)
        classes = ("gemm", "gemm_qkv", "gemm_out", "gemm_fc1", "gemm_fc2", "gemm_other", "attention", "layernorm", "embed", "head", "sample")
        parts = {c: lm.prof_get(c) for c in classes}
        ms, launches = parts["gemm"]
        lm.prof_enable(False)
        if rank == 0 and launches and args.precision in ("bf16", "fp16"):
            d_, f_, Mr = cfg["d_model"], cfg["d_ffn"], B * T
            el = 2                                                     # bytes per 16-bit operand
            # per launch: FLOPs and ALGORITHMIC bytes (operands read once + outputs written once; the residual GEMMs read and
            # write the fp32 stream) -- derived from the shapes, DESIGN.md section 4's table
            shapes = {"gemm_qkv": (Mr, 3 * d_, d_, Mr * d_ * el + 3 * d_ * d_ * el + Mr * 3 * d_ * el),
                      "gemm_out": (Mr, d_, d_, Mr * d_ * el + d_ * d_ * el + 2 * Mr * d_ * 4),
                      "gemm_fc1": (Mr, f_, d_, Mr * d_ * el + f_ * d_ * el + Mr * f_ * el),
                      "gemm_fc2": (Mr, d_, f_, Mr * f_ * el + d_ * f_ * el + 2 * Mr * d_ * 4)}
            per = {}
            for name, (m_, n_, k_, nbytes) in shapes.items():
                t_ms, n_l = parts[name]
                if n_l:
                    fl = 2.0 * m_ * n_ * k_
                    per[name] = {"launches_per_iter": n_l // n_prof, "avg_launch_us": 1e3 * t_ms / n_l, "gflop_per_launch": fl / 1e9,
                                 "algorithmic_MB_per_launch": nbytes / 1e6, "tflops": fl / (t_ms / n_l * 1e-3) / 1e12,
                                 "frac_of_mfma_peak": fl / (t_ms / n_l * 1e-3) / 1e12 / MFMA_BF16_PEAK_TFLOPS,
                                 "algorithmic_TB_per_s": nbytes / (t_ms / n_l * 1e-3) / 1e12}
            gf = executed_flops_per_iter()[0] * n_prof
            family = gf / (ms * 1e-3) / 1e12
            dom = max(per, key=lambda k_: parts[k_][0]) if per else None           # the kernel the iteration spends most time in
            _, pmc, traffic_src = measured_gemm_traffic()
            for k_ in per:
                if k_ in pmc:
                    tb = pmc[k_]["read"] + pmc[k_]["write"]
                    per[k_].update({"measured_fabric_MB_per_launch": tb / 1e6, "measured_fabric_read_MB_per_launch": pmc[k_]["read"] / 1e6,
                                    "traffic_ratio": tb / (per[k_]["algorithmic_MB_per_launch"] * 1e6)})
            w_l = {k_: per[k_]["launches_per_iter"] for k_ in per}
            alg_avg = (sum(per[k_]["algorithmic_MB_per_launch"] * w_l[k_] for k_ in per) / max(1, sum(w_l.values())) * 1e6) if per else None
            have = [k_ for k_ in per if "measured_fabric_MB_per_launch" in per[k_]]
            traffic = (sum(per[k_]["measured_fabric_MB_per_launch"] * w_l[k_] for k_ in have) / sum(w_l[k_] for k_ in have) * 1e6) if have else None
            kname = {"gemm_qkv": "QKV projection (gemm_bf16_w16_kernel<EPI_BF16>)", "gemm_out": "attention out-projection (gemm_bf16_pp_kernel<EPI_F32_RESID>)",
                     "gemm_fc1": "fc1 + GELU (gemm_bf16_w16_kernel<EPI_BF16_GELU>)", "gemm_fc2": "fc2 (gemm_bf16_pp_kernel<EPI_F32_RESID>)"}
            out["roofline"] = {"bound": "mfma", "kernel": kname.get(dom, "bf16 MFMA GEMM"),
                               "achieved": per[dom]["tflops"] if dom else family, "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
                               "frac": (per[dom]["tflops"] if dom else family) / MFMA_BF16_PEAK_TFLOPS,
                               "traffic": traffic,
                               "traffic_ratio": (traffic / alg_avg) if (traffic and alg_avg) else None,
                               "traffic_dominant_kernel": (per[dom].get("measured_fabric_MB_per_launch", 0) * 1e6 or None) if dom else None,
                               "traffic_note": "bytes/launch L2<->fabric (read / write request counters in separate --pmc passes of this script: "
                                               "reads = 128-B requests x 128, writes = requests x 64 and never below the output size; "
                                               "committed file %s -- PMC cannot be read from inside the timed process), "
                                               "weighted by this run's launches per iteration over the four per-layer GEMMs; algorithmic bytes of "
                                               "the same launches, from the shapes: %.0f; per-kernel measured / algorithmic in per_kernel[*].traffic_ratio"
                                               % (traffic_src, alg_avg or 0),
                               "avg_launch_ms": (per[dom]["avg_launch_us"] / 1e3) if dom else ms / launches,
                               "flops_per_launch": (per[dom]["gflop_per_launch"] * 1e9) if dom else gf / launches,
                               "gemm_family": {"achieved": family, "frac": family / MFMA_BF16_PEAK_TFLOPS, "launches_per_iter": launches // n_prof,
                                               "avg_launch_ms": ms / launches, "executed_gemm_tflop_per_iter": gf / n_prof / 1e12},
                               "per_kernel": per,
                               "peak_note": "peak = dense bf16 MFMA rate at 2.4 GHz; under this load the shader clock measured inside "
                                            "the GEMM main loop is ~1.72 GHz (power limit: 2.29 GHz with all-zero operands), "
                                            "profiles/r02_gemm_clock_probe.txt"}
            # north_star: "evidenced by rocprof HBM GB/s and MFMA utilisation".  (a) HBM-bound kernels of THIS run: bytes from the
            # shapes / this run's HIP-event time.  LayerNorm: 2 per layer on all M rows (fp32 row in, 16-bit row out) but for the
            # pruned last layer (one, on B*P rows); attention: q | k | v in, context out, one launch per layer.
            nl_ = cfg["n_layers"]
            ln_ms, ln_n = parts["layernorm"]
            at_ms, at_n = parts["attention"]
            ln_bytes = n_prof * (2 * (nl_ - 1) * Mr * d_ * (4 + el) + (B * P) * d_ * (4 + el))   # layer 0's LN1 is part of the embedding pass
            at_bytes = n_prof * nl_ * (Mr * 3 * d_ * el + Mr * d_ * el)
            hbm_peak = 8000.0
            out["roofline"]["hbm_bound_kernels"] = {
                "peak_GBps": hbm_peak, "achievable_GBps": 6300.0,
                "layernorm_bf16_kernel": {"launches_per_iter": ln_n // n_prof, "algorithmic_MB_per_iter": ln_bytes / n_prof / 1e6,
                                          "ms_per_iter": ln_ms / n_prof, "achieved_GBps": ln_bytes / (ln_ms * 1e-3) / 1e9 if ln_ms else None,
                                          "frac_of_hbm_peak": ln_bytes / (ln_ms * 1e-3) / 1e9 / hbm_peak if ln_ms else None},
                "attention_kernel": {"launches_per_iter": at_n // n_prof, "algorithmic_MB_per_iter": at_bytes / n_prof / 1e6,
                                     "ms_per_iter": at_ms / n_prof, "achieved_GBps": at_bytes / (at_ms * 1e-3) / 1e9 if at_ms else None,
                                     "frac_of_hbm_peak": at_bytes / (at_ms * 1e-3) / 1e9 / hbm_peak if at_ms else None,
                                     "gflop_per_launch": 4.0 * T * d_ * Mr / 1e9,
                                     "tflops": (4.0 * T * d_ * Mr * at_n) / (at_ms * 1e-3) / 1e12 if at_ms else None}}
            # (b) PMC-derived matrix-pipe utilisation and L2 hit rate of the hot kernels from the committed counters file
            pd = pmc_derived()
            if pd:
                kd = pd["kernels"]
                fam = "gemm_bf16_w16_kernel" if dom in ("gemm_fc1", "gemm_qkv") else "gemm_bf16_pp_kernel"
                out["roofline"]["mfma_util"] = kd.get(fam, {}).get("mfma_util")
                out["roofline"]["l2_hit"] = kd.get(fam, {}).get("l2_hit")
                out["roofline"]["pmc_derived"] = kd
                out["roofline"]["pmc_note"] = ("mfma_util = SQ_VALU_MFMA_BUSY_CYCLES / 1024 SIMDs / (GRBM_GUI_ACTIVE / 8 XCDs), l2_hit = TCC_HIT / "
                                               "(TCC_HIT + TCC_MISS); separate rocprofv3 --pmc passes of tools/pmc_bench.sh over the same kernels at the "
                                               "config-2 shapes, committed as profiles/%s (PMC cannot be read inside the timed process); the top-level "
                                               "mfma_util / l2_hit are those of the dominant kernel's family (%s)" % (pd["source"], fam))
        if rank == 0:
            out["time_split_ms_per_iter"] = {c: parts[c][0] / n_prof for c in ("gemm", "attention", "layernorm", "embed", "head", "sample")}
            out["time_split_ms_per_iter"]["gemm_by_projection"] = {c: parts[c][0] / n_prof for c in ("gemm_qkv", "gemm_out", "gemm_fc1", "gemm_fc2", "gemm_other")}

    # ---- N = 1: shard_proxy -- what ONE GPU of BASELINE config 3 runs at 2 / 4 / 8 GPUs, measured on this GPU ----------------
    # The first 128 / 64 / 32 chains of the SAME 256-chain job (engine told `set_job_items(256)`: the kernel choices of the whole job,
    # so the shard's tokens are bit-identical with the single-GPU run's -- tests/test_gpu_fullsize.py), ms per Gibbs iteration,
    # efficiency against 1/N of this run's full-batch step, and the whole-node rate N such GPUs would deliver (the final 33-KB
    # all-gather is not in it: microseconds once per job).  Chains are independent in the reference (esm_sampler.py:223-234).
    if rank == 0 and world == 1 and not dry and not args.no_shard_proxy and B_total == TOTAL_CHAINS and not args.weak:
        lm.set_job_items(B_total)
        full_ms = 1e3 * elapsed / K
        proxy = {"full_batch_ms_per_step": full_ms, "shards": {}}
        for n_gpu in (2, 4, 8):
            c = B_total // n_gpu
            pj = Job(lm, 0, c)
            keep = pj.run(2)
            torch.cuda.synchronize(dev)
            kp = max(3, min(K, 10))
            t0 = time.perf_counter()
            keep = pj.run(kp)
            torch.cuda.synchronize(dev)
            ms = 1e3 * (time.perf_counter() - t0) / kp
            proxy["shards"][str(n_gpu)] = {"chains_per_gpu": c, "token_rows": c * T, "steps": kp, "ms_per_step": ms,
                                           "efficiency_vs_linear": full_ms / n_gpu / ms,
                                           "predicted_whole_node_positions_per_s": B_total * P / (ms * 1e-3)}
        proxy["note"] = ("single-GPU proxy for the strong-scaling curve (no 8-GPU node on this pool): ms/step of a 1/N shard of the "
                         "256-chain job with the job's kernel choices; predicted whole-node rate = 256 x P / that time; "
                         "tools/shard_regime.py --engine is the stand-alone form")
        out["shard_proxy"] = proxy

    # ---- N = 1 extras: strict-mode leg, config 1 on the GPU, CPU baseline ------------------------------------------------
    lm_strict = None
    if rank == 0 and world == 1 and not dry and args.precision == "bf16" and not args.no_strict:
        lm_strict = models.ESM1b(state_dict=sd, config=cfg, precision="fp32").model.to(str(dev))
        _lib.check(L_.pg_engine_set_stream(lm_strict.handle, ctypes.c_void_p(stream.cuda_stream)))
        sj = Job(lm_strict, 0, B_total)
        keep = sj.run(1)
        torch.cuda.synchronize(dev)
        ks = max(1, min(K, 3))
        t0 = time.perf_counter()
        keep = sj.run(ks)
        torch.cuda.synchronize(dev)
        ts = time.perf_counter() - t0
        out["strict_mode"] = {"value": B_total * P * ks / ts, "unit": "sampled positions/s", "ms_per_step": 1e3 * ts / ks, "steps": ks,
                              "precision": "PG_PREC_FP32: split-bf16 x3 MFMA products (lo.hi + hi.lo + hi.hi) in the projections and in attention, fp32 accumulation/softmax/LayerNorm",
                              "max_abs_logit_err": None}
    # fp16-operand throughput mode: the headline's kernels with v_mfma_f32_16x16x32_f16 and fp16 stores
    lm_f16 = None
    if rank == 0 and world == 1 and not dry and args.precision == "bf16" and not args.no_fp16:
        lm_f16 = models.ESM1b(state_dict=sd, config=cfg, precision="fp16").model.to(str(dev))
        _lib.check(L_.pg_engine_set_stream(lm_f16.handle, ctypes.c_void_p(stream.cuda_stream)))
        lm_f16.set_job_items(B_total)
        fj = Job(lm_f16, 0, B_total)
        keep = fj.run(2)
        torch.cuda.synchronize(dev)
        kf = max(1, min(K, 10))
        t0 = time.perf_counter()
        keep = fj.run(kf)
        torch.cuda.synchronize(dev)
        tf = time.perf_counter() - t0
        out["fp16_mode"] = {"value": B_total * P * kf / tf, "unit": "sampled positions/s", "ms_per_step": 1e3 * tf / kf, "steps": kf,
                            "precision": "PG_PREC_F16: the bf16 mode's kernels with IEEE fp16 operands (v_mfma_f32_16x16x32_f16, fp16 "
                                         "weights / LayerNorm outputs / q,k,v / softmax numerators / context / FFN rows), fp32 accumulation, "
                                         "residual stream, softmax, LayerNorm",
                            "max_abs_logit_err": None}
    gpu_cfg1 = None
    if rank == 0 and world == 1 and not dry and not args.no_cpu_baseline:
        # BASELINE config 1 on the GPU: one chain, L = 25 (T = 27), P = 2, 20 iterations, top_k = 1, burnin = 10
        import random
        from protein_gibbs_sampler_amd import esm_sampler
        lm.set_job_items(0)            # config 1 is a whole job of its own, not a shard of the 256-chain job (r02's 4.27 ms/iteration
                                       # was this: the single chain ran with the big job's kernel choices)
        s1 = esm_sampler.ESM_sampler(wrapper, device=str(dev))
        kw = dict(batch_size=1, num_iters=20, burnin=10, mask=True, in_order=False, num_positions_percent=10, top_k=1,
                  show_progress_bar=False)
        random.seed(0)
        s1.generate(1, "MEPAATGQEAEECAHSGRGEAWEEV", **kw)
        s1.generate(1, "MEPAATGQEAEECAHSGRGEAWEEV", **kw)
        c0, r0 = lm.get_stat("graph_captures"), lm.get_stat("graph_replays")
        n_calls = 20
        t0 = time.perf_counter()
        for _ in range(n_calls):
            s1.generate(1, "MEPAATGQEAEECAHSGRGEAWEEV", **kw)      # one generate() per sequence, as pgen_esm.py issues them
        tg = (time.perf_counter() - t0) / n_calls
        gpu_cfg1 = {"gpu_positions_per_s": 40 / tg, "gpu_ms_per_iter": 1e3 * tg / 20, "gpu_ms_per_generate_call": 1e3 * tg,
                    "generate_calls_timed": n_calls,
                    "graph_captures_during_timing": lm.get_stat("graph_captures") - c0,
                    "graph_replayed_iterations_during_timing": lm.get_stat("graph_replays") - r0,
                    "note": "whole generate() calls (tokenise, position table, H2D, 20 iterations as replays of one captured "
                            "hipGraph, D2H, untokenise); a fresh torch draw seed per call"}
        _lib.check(L_.pg_engine_set_stream(lm.handle, ctypes.c_void_p(stream.cuda_stream)))
    if rank == 0 and world == 1 and not dry and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(cfg, sd, lm if args.precision == "bf16" else None,
                                           lm_strict if lm_strict is not None else (lm if args.precision == "fp32" else None),
                                           B_total, L, P, valid_idx, gpu_cfg1, lm_f16=lm_f16)
        chk = out["cpu_baseline"]["logit_check"]
        if "fp16_mode" in out:
            out["fp16_mode"].update({k_[5:]: v_ for k_, v_ in chk.items() if k_.startswith("fp16_")})
            out["fp16_mode"]["logit_std"] = chk["logit_std"]
            out["fp16_mode"]["bf16_mode_for_comparison"] = {k_[5:]: v_ for k_, v_ in chk.items() if k_.startswith("bf16_")}
        if "strict_mode" in out:
            out["strict_mode"]["max_abs_logit_err"] = chk.get("fp32_max_abs_logit_err")
            out["strict_mode"]["logit_std"] = chk["logit_std"]
        out["bf16_max_abs_logit_err"] = chk.get("bf16_max_abs_logit_err")
        if "strict_mode" in out and out["strict_mode"]["max_abs_logit_err"] is not None:
            # north_star: "within 1e-3 on emitted logits".  `value` above is the bf16-operand mode BASELINE config 2 names, which does
            # NOT meet that tolerance; this is the throughput of the mode that does, on the same workload and weights.
            out["value_at_tolerance"] = {"value": out["strict_mode"]["value"], "unit": "sampled positions/s",
                                         "ms_per_step": out["strict_mode"]["ms_per_step"], "mode": "PG_PREC_FP32 (strict)",
                                         "tolerance": 1e-3, "max_abs_logit_err": out["strict_mode"]["max_abs_logit_err"],
                                         "meets_tolerance": bool(out["strict_mode"]["max_abs_logit_err"] < 1e-3),
                                         "headline_mode_max_abs_logit_err": chk.get("bf16_max_abs_logit_err"),
                                         "headline_mode_meets_tolerance": bool((chk.get("bf16_max_abs_logit_err") or 1.0) < 1e-3)}
        # BASELINE config 1 (one chain, L = 25) measured on CPU and GPU inside cpu_baseline(): also at the top level of the line
        if "config1" in out["cpu_baseline"]:
            out["config1"] = out["cpu_baseline"]["config1"]
    # ---- N = 1: the ESM-MSA-1b configurations (BASELINE configs 4 and 5) on the same GPU, driver-timed -------------------
    if rank == 0 and world == 1 and not dry and not args.no_msa and args.precision == "bf16":
        import bench_msa
        del lm_strict, lm_f16
        mw, mlm, mcfg = bench_msa.build("bf16", str(dev), realistic=True)
        _lib.check(L_.pg_engine_set_stream(mlm.handle, ctypes.c_void_p(stream.cuda_stream)))
        c4 = bench_msa.run_config4(mw, mlm, mcfg, steps=3, warmup=1, dev=dev)
        c5 = bench_msa.run_config5(mw, mlm, mcfg, templates=4, dev=dev, max_batch=4)
        c5_1 = bench_msa.run_config5(mw, mlm, mcfg, templates=1, dev=dev, max_batch=1)
        keep4 = ("value", "unit", "ms_per_step", "steps", "model_tflops", "frac_of_bf16_mfma_peak", "time_split_ms_per_iter", "config")
        keep5 = ("value", "unit", "templates", "templates_per_call", "ms_per_forward", "ms_per_template_forward", "model_tflops",
                 "frac_of_bf16_mfma_peak", "time_split_ms_per_forward", "config")
        out["msa"] = {"config4": {k_: c4[k_] for k_ in keep4}, "config5": {k_: c5[k_] for k_ in keep5},
                      "config5_one_template_per_call": {k_: c5_1[k_] for k_ in keep5},
                      "weights": "synthetic ESM-MSA-1b (12 layers, d=768), same scale as above"}
        if not args.no_strict:
            # north_star's 1e-3 for the ESM-MSA-1b configurations too: the strict engine's throughput on configs 4 and 5 (one
            # step / one template), with its max |logit error| against the fp32 oracle measured on one config-4 alignment of the
            # same weights (the bf16 engine's beside it); config 5's 128 x 513 shape against the oracle: tests/test_gpu_config5_oracle.py
            mws, mls, _ = bench_msa.build("fp32", str(dev), realistic=True)
            _lib.check(L_.pg_engine_set_stream(mls.handle, ctypes.c_void_p(stream.cuda_stream)))
            chk4 = bench_msa.logit_check({"bf16": mlm, "fp32": mls}) if not args.no_cpu_baseline else {}
            s4 = bench_msa.run_config4(mws, mls, mcfg, steps=1, warmup=1, precision="fp32", dev=dev)
            s5 = bench_msa.run_config5(mws, mls, mcfg, templates=1, precision="fp32", dev=dev, max_batch=1)
            e32, e16 = chk4.get("fp32_max_abs_logit_err"), chk4.get("bf16_max_abs_logit_err")

            def at_tol(v, ms_key, ms):
                return {"value": v, "unit": "sampled positions/s", ms_key: ms, "mode": "PG_PREC_FP32 (strict)", "tolerance": 1e-3,
                        "max_abs_logit_err": e32, "meets_tolerance": (bool(e32 < 1e-3) if e32 is not None else None),
                        "headline_mode_max_abs_logit_err": e16,
                        "headline_mode_meets_tolerance": (bool(e16 < 1e-3) if e16 is not None else None)}
            out["msa"]["config4"]["value_at_tolerance"] = at_tol(s4["value"], "ms_per_step", s4["ms_per_step"])
            out["msa"]["config5"]["value_at_tolerance"] = at_tol(s5["value"], "ms_per_template_forward", s5["ms_per_template_forward"])
            out["msa"]["config5"]["value_at_tolerance"]["templates_per_call"] = 1
            out["msa"]["logit_check"] = chk4
            del mls, mws
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(out))


if __name__ == "__main__":
    main()
