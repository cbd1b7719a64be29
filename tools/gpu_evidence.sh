# Evidence pass: PMC traffic passes first (-> profiles/traffic.json on the box, copied back),
# then the default bench (with CPU baseline, reads traffic.json), then a rocprof kernel trace of
# one batch in flight.  Every GPU step has its own time limit; the first failure ends the script.
set -o pipefail
EV=${EV:-bench_out/evidence}
mkdir -p $EV
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
ONE="--steps 2 --warmup 1 --inflight 1 --no-cpu-baseline --no-distinct --no-extra"
R=${R:-r3}
echo "== pmc: FETCH_SIZE"
timeout -s KILL 120 rocprofv3 --pmc FETCH_SIZE -d $EV/pmc_fetch -o $R --output-format csv -- python3 bench.py $ONE > $EV/pmc_fetch.log 2>&1 || { tail -3 $EV/pmc_fetch.log; exit 1; }
echo "== pmc: WRITE_SIZE"
timeout -s KILL 120 rocprofv3 --pmc WRITE_SIZE -d $EV/pmc_write -o $R --output-format csv -- python3 bench.py $ONE > $EV/pmc_write.log 2>&1 || { tail -3 $EV/pmc_write.log; exit 1; }
echo "== pmc: valu"
timeout -s KILL 120 rocprofv3 --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_INSTS_SALU -d $EV/pmc_valu -o $R --output-format csv -- python3 bench.py $ONE > $EV/pmc_valu.log 2>&1 || { tail -3 $EV/pmc_valu.log; exit 1; }
NSETS=$(grep -h '"metric"' $EV/pmc_fetch.log | python3 -c 'import json,sys; print(json.loads(sys.stdin.read())["config"]["sets_per_gpu"])')
python3 tools/pmc_traffic.py $(find $EV/pmc_fetch -name "*counter_collection.csv") $(find $EV/pmc_write -name "*counter_collection.csv") $NSETS > profiles/traffic.json && cp profiles/traffic.json $EV/traffic.json
echo "== bench (default flags, with cpu baseline)"
timeout -k 10 600 python3 -u bench.py --full > $EV/bench_default.log 2>&1 || { tail -20 $EV/bench_default.log; exit 1; }
tail -1 $EV/bench_default.log | cut -c1-400
echo "== rocprof kernel trace (single batch in flight)"
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $EV/kt -o $R --output-format csv -- python3 bench.py --steps 5 --warmup 1 --inflight 1 --no-cpu-baseline --no-distinct --no-extra > $EV/kt.log 2>&1 || { tail -20 $EV/kt.log; exit 1; }
grep -h '"metric"' $EV/kt.log | cut -c1-200
find $EV -name "*.csv" | sort
