# bench lines for a list of configs: bash tools/gpurun/bench_cfgs.sh TAG "c3 c2" [extra bench args]
set -o pipefail
O=${OUT:-bench_out}
mkdir -p $O
TAG=${1:-run}; CFGS=${2:-c3}; shift 2 || true
for c in $CFGS; do
  timeout -k 10 300 python -u bench.py --full --config $c --steps 3 --warmup 1 --no-cpu-baseline --no-ingest "$@" \
    > $O/${TAG}_$c.json 2> $O/${TAG}_$c.log || exit $?
done
