#!/bin/bash
# Every bench.py workload line of DESIGN.md section 0 on one MI355X -> gpurun_out/bench_<name>.json
set -o pipefail
mkdir -p gpurun_out
run() {  # name args...
  local n=$1; shift
  timeout -k 10 300 python3 bench.py "$@" > gpurun_out/bench_$n.json 2> gpurun_out/bench_$n.err \
    || { tail -5 gpurun_out/bench_$n.err; return 1; }
  python3 -c "import json,sys; d=json.load(open(sys.argv[1])); print(sys.argv[2], d['ms_per_step'], d['roofline'].get('valu', {}).get('frac'), d['roofline'].get('frac'))" \
    gpurun_out/bench_$n.json $n
}
F=--full  # the summary above reads the roofline
run lde $F --workload lde && run lde_bitrev $F --workload lde --order bitrev && run msm $F --workload msm \
  && run msm_small $F --workload msm --msm-scalars small && run ntt4 $F --workload ntt4 \
  && run msm_shard $F --workload msm-shard && run quotient_fused $F --workload quotient \
  && run quotient_generic $F --workload quotient --air generic && run verify $F --workload verify
