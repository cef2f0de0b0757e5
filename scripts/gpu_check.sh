#!/bin/bash
# Replays the end-of-round checks in their order: the GPU tests, smoke(), the full bench line (bench.py --full).
#   bash scripts/gpu_check.sh [OUTDIR]      (OUTDIR: where the log and the bench line go, default gpu_check_out)
out=${1:-gpu_check_out}
mkdir -p "$out"
{
python3 -m pytest tests -q -m gpu -x 2>&1 | tail -4
python3 -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -2
t0=$SECONDS
python3 bench.py --full 2> "$out/gpu_check_bench.err" | tail -1 > "$out/gpu_check_bench.json"
echo "bench.py wall $((SECONDS - t0)) s"
python3 - "$out/gpu_check_bench.json" <<'PY'
import json, sys
d=json.load(open(sys.argv[1]))
print('ms/step %.3f value %.4g frac %.3f fp64 %.3f/%.3f' % (d['ms_per_step'], d['value'], d['roofline']['frac'], d['roofline']['fp64_frac'], d['roofline']['fp64_frac_incl_halo']), d['phase_ms'])
print('cg', d['cg_iterations_per_s'], d['distributed_cg']['local_spmv_ms'], 'graph_step', (d.get('graph_step') or {}).get('ms_per_step'), 'xch', d['slab_sweep'].get('exchange_latency')); print('kernel', d['roofline']['kernel'], 'limiter', d['roofline'].get('limiter')); print('cpu', d['cpu_baseline']['value'], d['cpu_baseline'].get('parity'))
for k,v in d['slab_sweep']['layers'].items(): print('  ', k, {a:(round(b,4) if isinstance(b,float) else b) for a,b in v.items() if a!='phase_ms'})
print({k:{a:round(b) for a,b in v.items() if a.endswith('per_s')} for k,v in d['cpu_baseline']['table'].items()}, d['cpu_baseline']['physical_cores'])
PY
} > "$out/gpu_check.log" 2>&1
tail -c 6000 "$out/gpu_check.log"
