O=${OUT:-bench_out}
mkdir -p $O
timeout -k 10 200 python -u bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-ingest --no-chunked > $O/b1.json 2> $O/b1.log; echo "bench rc=$?" >> $O/b1.log
HGX_LIB=libhgx_prof.so timeout -k 10 200 python -u tools/phase_timing.py c3 2 > $O/ph_c3.log 2>&1
HGX_LIB=libhgx_prof.so timeout -k 10 200 python -u tools/phase_timing.py c2 2 > $O/ph_c2.log 2>&1
tail -5 $O/b1.log
