# bench lines (the default policy, the f32-input MFMA visibility kernel) + rocprofv3 kernel traces of both -> OUT_DIR
# usage: bash tools/run_bench_prof.sh OUT_DIR
O=$(realpath -m "${1:?usage: bash tools/run_bench_prof.sh OUT_DIR}")
cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
mkdir -p $O/prof
python bench.py --full > $O/bench_final.json 2> $O/bench_final.err
cat $O/bench_final.json
python bench.py --full --vis-precision fp32 --no-cpu-baseline > $O/bench_fp32.json 2> $O/bench_fp32.err
cat $O/bench_fp32.json
rocprofv3 --kernel-trace --stats -d $O/prof -o trace -- python bench.py --steps 2 --warmup 1 --no-cpu-baseline > $O/prof/bench.log 2>&1
python tools/rocpd_summary.py $(find $O/prof -name '*.db' | head -1) > $O/prof/summary.md
find $O/prof -name '*.db' -delete
rocprofv3 --kernel-trace --stats -d $O/prof32 -o trace -- python bench.py --steps 2 --warmup 1 --no-cpu-baseline --vis-precision fp32 > $O/prof/bench32.log 2>&1
python tools/rocpd_summary.py $(find $O/prof32 -name '*.db' | head -1) > $O/prof/summary_fp32.md
rm -rf $O/prof32
head -24 $O/prof/summary.md
python tools/bench_configs.py 2>&1 | grep -E "^config"
