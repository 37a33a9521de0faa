cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
O=${1:?usage: other_configs_r01.sh <output directory>}
mkdir -p $O; rm -rf $O/*
rocprofv3 --kernel-trace --stats -d $O/t5 -o r -- python bench.py --full --steps 1 --warmup 0 --workload manip7 > $O/bench_manip7.json 2> $O/err5.log
python profiles/summarize_rocpd.py $O/t5/r_results.db $O/kernel_stats_manip7.md | head -3
rocprofv3 --kernel-trace --stats -d $O/t4 -o r -- python bench.py --full --steps 1 --warmup 0 --workload quadrotor --batch 2048 > $O/bench_quadrotor.json 2> $O/err4.log
python profiles/summarize_rocpd.py $O/t4/r_results.db $O/kernel_stats_quadrotor.md | head -3
python bench.py --full --steps 3 --warmup 1 --workload unicycle --batch 8192 > $O/bench_unicycle.json 2>> $O/err4.log
for f in manip7 quadrotor unicycle; do python -c "
import json,sys;d=json.load(open('$O/bench_$f.json'));print('$f',d['value'],d['ms_per_step'],d['roofline']['frac'],d['cpu_baseline']['value'])"; done
