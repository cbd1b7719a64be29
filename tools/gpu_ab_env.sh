# A/B of env knobs / library variants on the default bench (AB_FLAGS picks the secondary legs); logs in $OUT:
# LB_RUNS="default env:LB_SUBGROUP_G8_MAX=1000000 lib:sub1"
set -o pipefail
OUT=${OUT:-bench_out/ab}
mkdir -p $OUT
for r in $LB_RUNS; do
  unset LODESTAR_BLS_LIB
  envs=""
  case "$r" in
    env:*) envs="${r#env:}"; envs=${envs//+/ } ;;
    lib:*) export LODESTAR_BLS_LIB=$GRAFT_REPO_ROOT/build/variants/${r#lib:}.so ;;
  esac
  tag=$(echo "$r" | tr ':=/' '___')
  env $envs timeout -k 10 300 python -u bench.py --full --steps 5 --warmup 1 --no-cpu-baseline --no-distinct $AB_FLAGS > $OUT/$tag.log 2>&1 || { tail -5 $OUT/$tag.log; exit 1; }
  echo "== $r"; tail -1 $OUT/$tag.log | python3 tools/bench_summary.py
done
