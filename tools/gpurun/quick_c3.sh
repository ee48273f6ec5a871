# quick check after a kernel change: parity subset, then c3 phase times and one bench line
# usage: bash tools/gpurun/quick_c3.sh TAG "pytest -k expression"
set -o pipefail
O=${OUT:-bench_out}
mkdir -p $O
TAG=${1:-q}; K=${2:-gossip_batch or kat or fixture or incremental or int32}
timeout -k 10 400 python -u -m pytest tests/test_gpu_parity.py tests/test_gpu_incremental.py -x -q --timeout 200 --timeout-method thread -k "$K" > $O/${TAG}_tests.log 2>&1 || { tail -30 $O/${TAG}_tests.log; exit 1; }
tail -1 $O/${TAG}_tests.log
timeout -k 10 300 python -u bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-ingest --no-check --no-chunked > $O/${TAG}_bench.json 2> $O/${TAG}_bench.log && grep "kernel profile" $O/${TAG}_bench.log
