# LandModel paths after a change of the surface processes: parity suites, then C4 / C4-VG per-step and the 1/8 shard's multi-step program
python -m pytest tests/test_gpu_parity.py tests/test_gpu_column_programs.py tests/test_gpu_reference_tests.py tests/test_gpu_input_series.py tests/test_gpu_coupled_vegetation.py tests/test_gpu_property.py tests/test_golden_vectors.py -q -x -W ignore::DeprecationWarning > gpurun_out/land.log 2>&1; tail -2 gpurun_out/land.log
OUT=${OUT:-$(mktemp -d)}     # the bench lines and their stderr
for wl in c4 c4vg c3vg; do python bench.py --full --workload $wl --no-cpu-baseline --no-hbm-resident --multistep 0 --steps 100 --warmup 10 > $OUT/$wl.json 2> $OUT/$wl.err; python -c "
import json; d=json.load(open('$OUT/$wl.json')); print('$wl', round(d['value']/1e9,3), round(d['ms_per_step']*1e3,2), round(d['roofline']['kernel_ms']*1e3,2), round(d['roofline']['frac'],3))"; done
for wl in c4 c3; do TRM_BENCH_SHARD_OF=8 python bench.py --full --workload $wl --no-cpu-baseline --no-hbm-resident --multistep 50 --steps 200 --warmup 10 > $OUT/${wl}_shard.json 2> $OUT/${wl}_shard.err; python -c "
import json; d=json.load(open('$OUT/${wl}_shard.json')); print('$wl shard', round(d['ms_per_step']*1e3,2), 'multistep', d['multistep']['us_per_step'])"; done
