# PMC passes for the bench's SpMM kernel (separate passes: FETCH_SIZE and WRITE_SIZE do not fit one TCC pass),
# then the kernel-trace summary and the full bench line (with the CPU baseline)
set -o pipefail
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
OUT=${OUT:?set OUT to the folder the results go to}
mkdir -p $OUT/r11
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --kernel-include-regex "spmm_main<64, 0>" --output-format csv -d $OUT/r11/pmc_fetch -o run -- python bench.py --full --steps 20 --warmup 2 --no-cpu-baseline > /dev/null 2> $OUT/r11/pmc_fetch.err && \
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --kernel-include-regex "spmm_main<64, 0>" --output-format csv -d $OUT/r11/pmc_write -o run -- python bench.py --full --steps 20 --warmup 2 --no-cpu-baseline > /dev/null 2> $OUT/r11/pmc_write.err && \
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/r11/stats -o bench -- python bench.py --full --no-cpu-baseline > $OUT/r11/bench_prof.json 2> $OUT/r11/bench_prof.err && \
timeout -k 10 600 python bench.py --full > $OUT/r11/bench_full.json 2> $OUT/r11/bench_full.err
rc=$?
find $OUT/r11 -name '*kernel_trace.csv' -delete
echo "rc=$rc"
