#!/bin/bash
# per-kernel time of the bf16 bench under fixed GEMM tile shapes (cpt_set_tuning key 0); usage: tools/variant_sweep.sh "3 17 ..."
for a in $1; do
  python bench.py --full --no-cpu --no-check --steps 30 --warmup 5 --tune "0=$a" 2>/dev/null | python -c "
import sys, json
d = json.loads(sys.stdin.read())
k = d['kernel_ms_per_step']
print('variant %-5s ms/step %.4f  qkv %.1f ao %.1f up %.1f down %.1f (us per launch)' % ('$a', d['ms_per_step'], k['gemm_qkv']/12*1e3, k['gemm_attn_out']/12*1e3, k['gemm_ffn_up']/12*1e3, k['gemm_ffn_down']/12*1e3))"
done
