cd "$(dirname "$0")/.."
out=${1:?usage: bash tools/r4_final.sh <output dir>}
mkdir -p $out
( time python bench.py --full ) > $out/bench_default.json 2> $out/bench_default.err
python bench.py --full --workload lm13_n4096 --no-extras > $out/bench_lm13.json 2> $out/bench_lm13.err
python bench.py --full --workload ycbv_rr21 --no-extras > $out/bench_ycbv.json 2> $out/bench_ycbv.err
python bench_train.py > $out/bench_train.json 2> $out/bench_train.err
tail -4 $out/bench_default.err
