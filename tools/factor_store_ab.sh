#!/bin/bash
# binary against binary on one box: the headline step with the library at $1 (GPMP_HIP_LIB, e.g. a build of the parent commit), with
# the in-tree library, and with the in-tree library and the factor store off -- interleaved, three times each.  Results: $2/*.json
base=$1; out=${2:-factor_store_ab}
mkdir -p "$out"
for rep in 1 2 3; do
  for cfg in parent new off; do
    case $cfg in
      parent) envs="GPMP_HIP_LIB=$base";;
      new) envs="GPMP_FACTOR_STORE_AB=1";;
      off) envs="GPMP_FACTOR_STORE_MB=0";;
    esac
    env $envs timeout -k 10 300 python3 bench.py --gpus 1 --steps 20 --warmup 5 --no-extras --no-cpu-baseline --no-live-pmc \
      > "$out/${cfg}_$rep.json" 2> "$out/${cfg}_$rep.err" || { echo "$cfg $rep failed"; tail -20 "$out/${cfg}_$rep.err"; exit 1; }
    echo "$cfg $rep: $(grep -o '"ms_per_step": [0-9.]*' "$out/${cfg}_$rep.json" | head -1)"
  done
done
