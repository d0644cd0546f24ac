# One full default bench.py run (the driver's N=1 command) with its stderr progress.
set -e
OUT=${OUT:-out}/${TAG:-r6ae}
mkdir -p $OUT
timeout -k 10 1000 python bench.py --full > $OUT/bench1.json 2> $OUT/bench1.err
tail -c 300 $OUT/bench1.json
