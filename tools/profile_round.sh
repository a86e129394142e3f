# refreshes the evidence for the default bench under build/profile_<tag>/ (or $OUT): the --full JSON line, rocprofv3 kernel stats, HBM counters (separate passes)
# usage: bash tools/profile_round.sh <tag>
tag=${1:-run}
R=${GRAFT_REPO_ROOT:-$PWD}
O=${OUT:-$R/build/profile_$tag}; mkdir -p $O
cd /tmp && export TMPDIR=/tmp
python $R/bench.py --full > $O/bench_$tag.json 2> $O/bench_$tag.err
rocprofv3 --kernel-trace --stats -d $O/kt_$tag -- python $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $O/kt_$tag.log 2>&1
rocprofv3 --pmc FETCH_SIZE -d $O/pmc_fetch_$tag --output-format csv -- python $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $O/pmc_fetch_$tag.log 2>&1
rocprofv3 --pmc WRITE_SIZE -d $O/pmc_write_$tag --output-format csv -- python $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $O/pmc_write_$tag.log 2>&1
cd $R
python tools/prof_summary.py $O/kt_$tag $O/kernel_stats_$tag.txt > /dev/null 2>&1
python tools/pmc_summary.py $O/pmc_fetch_$tag $O/pmc_fetch_$tag.txt > /dev/null 2>&1
python tools/pmc_summary.py $O/pmc_write_$tag $O/pmc_write_$tag.txt > /dev/null 2>&1
rm -rf $O/kt_$tag $O/pmc_fetch_$tag $O/pmc_write_$tag   # (raw traces: tens of MB)
cut -c1-1800 $O/bench_$tag.json; head -8 $O/kernel_stats_$tag.txt
