# full check on the GPU box: tests, smoke, bench (+ rocprofv3 kernel stats), HBM traffic passes
set -eo pipefail
cd $GRAFT_REPO_ROOT
R=$GRAFT_REPO_ROOT
TAG=${1:-r01d}
O=${2:-$R/bench_out/$TAG}
mkdir -p $O
timeout 1500 python -m pytest tests -x -q -m gpu 2>&1 | tail -4 > $O/pytest_gpu.txt
cat $O/pytest_gpu.txt
timeout 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -2
timeout 900 python bench.py --full > $O/bench_line.json 2> $O/bench_err.txt
tail -c 3000 $O/bench_line.json
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats -- python3 $R/bench.py --no-cpu --no-e2e --no-overlap > $O/bench_under_rocprof.json 2>/dev/null
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/pmc_fetch -- python3 $R/bench.py --steps 1 --warmup 1 --no-cpu --no-e2e --no-overlap > /dev/null 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/pmc_write -- python3 $R/bench.py --steps 1 --warmup 1 --no-cpu --no-e2e --no-overlap > /dev/null 2>&1
for c in rox rolz; do
  rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats_$c -- python3 $R/bench.py --no-cpu --no-e2e --no-overlap --codec $c > $O/bench_line_$c.json 2>/dev/null
done
cd $R
python3 tools/collect_traffic.py $O/pmc_fetch $O/pmc_write $O/traffic.json "bench.py --steps 1 --warmup 1, 1e8 B shard" > /dev/null
cat $O/stats/*/*kernel_stats.csv | cut -c1-120 | head -14
for c in rox rolz; do cat $O/stats_$c/*/*kernel_stats.csv | cut -c1-100 | head -10; done
find $O -name "*.csv" -size +2M -delete
find $O -name "*counter_collection.csv" -delete
