# SHA-256 parity tests then a c3 bench line with the ingest side leg
set -o pipefail
O=${OUT:-bench_out}
mkdir -p $O
timeout -k 10 300 python -u -m pytest tests/test_gpu_sha256.py -m gpu -x -v --timeout 200 --timeout-method thread > $O/sha_tests.log 2>&1 && \
timeout -k 10 300 python -u bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $O/sha_bench.json 2> $O/sha_bench.log
