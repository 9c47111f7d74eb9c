#!/bin/bash
# The round-6 experiments as they were run on the GPU box (each section wrote the profiles/r06_* file named beside it).  The legs of the
# tile-height and full-row LayerNorm GEMM experiments left with their kernels (EXPERIMENTS.md; the tree at commit 2e0ada3 has them).
#   bash tools/r06_experiments.sh fewchain|traffic
cd "${GRAFT_REPO_ROOT:-.}"
O=gpurun_out/r06x; mkdir -p $O
case "$1" in
  fewchain)        # profiles/r06_few_chain_gemm_bench.txt: every tile kernel forced at 8 ... 32 chains
    python tools/few_chain_gemm_bench.py | tee $O/few_chain_gemm_bench.txt ;;
  traffic)         # profiles/r06_hbm_traffic_pmc.json, r06_gemm_pmc_counters.txt
    bash tools/pmc_traffic.sh r06 | tee $O/traffic.txt
    for k in gemm_bf16_w16_kernel gemm_bf16_pp_kernel attention_kernel layernorm_bf16_kernel; do echo "== $k"; bash tools/pmc_bench.sh $k r06$k; done 2>&1 | grep -E "^==|^pass" > $O/gemm_pmc_counters_raw.txt
    python tools/pmc_counters_report.py $O/gemm_pmc_counters_raw.txt "round 6" > $O/gemm_pmc_counters.txt ;;
  *) echo "usage: $0 fewchain|traffic" ;;
esac
