# Evidence of a round on one MI355X: bench line, rocprofv3 kernel stats of the same command, two PMC passes and their summary (copy into profiles/).
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd); OUT=$ROOT/${OUT:-results}; mkdir -p "$OUT"
cd $ROOT
timeout -k 10 400 python bench.py --full > $OUT/v13_bench.json 2> $OUT/v13_bench.err
cd /tmp && export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_v13 -o v13 -- python3 $ROOT/bench.py --gpus 1 --full --steps 4 --warmup 2 --no-cpu-baseline > $OUT/v13_under.json 2> $OUT/v13_under.err
timeout -k 10 300 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_v13_f -o f -- python3 $ROOT/bench.py --steps 2 --warmup 1 --no-cpu-baseline > $OUT/pmc_f.log 2>&1
timeout -k 10 300 rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_v13_w -o w -- python3 $ROOT/bench.py --steps 2 --warmup 1 --no-cpu-baseline > $OUT/pmc_w.log 2>&1
cd $ROOT
python scripts/pmc_summarize.py $OUT/pmc_v13_f/f_counter_collection.csv $OUT/pmc_v13_w/w_counter_collection.csv 249999970 $OUT/pmc_v13.json
cat $OUT/v13_bench.json
