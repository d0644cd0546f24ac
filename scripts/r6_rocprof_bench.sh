# rocprofv3 kernel trace + stats of a short bench.py --full run (the GPU probes
# and the placement check are the bench's GPU work); rocpd db under $OUT.
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/out}/r6ar_rocprof_bench
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
timeout -k 10 900 rocprofv3 --kernel-trace --stats -d $OUT -o bench -- python3 $R/bench.py --full --steps 5 --warmup 1 --no-open-loop --no-scenarios --no-service-mode > $OUT/bench.log 2>&1
tail -c 200 $OUT/bench.log
