python -m pytest tests/test_gpu_parity.py tests/test_gpu_column_programs.py tests/test_gpu_reference_tests.py -q -x > gpurun_out/pk.log 2>&1; tail -3 gpurun_out/pk.log
OUT=${OUT:-$(mktemp -d)}     # the bench lines and their stderr
for wl in c3vg c4vg c5vg; do python bench.py --full --workload $wl --no-cpu-baseline --no-hbm-resident --multistep 0 --steps 50 --warmup 5 > $OUT/$wl.json 2> $OUT/$wl.err; python -c "
import json; d=json.load(open('$OUT/$wl.json')); print('$wl', round(d['value']/1e9,3), d['roofline']['kernel_ms'], round(d['roofline']['frac'],3))"; done
