#!/bin/bash
# PMC counters of the persistent 256x256 kernel's K loop on one shape: tools/pp_pmc.sh M N K kind  -> pp_pmc.txt beside the pp_pmc/ directory of the passes
ROOT=$(pwd); OUT=$ROOT/gpurun_out/pp_pmc; rm -rf $OUT; mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
i=0
for C in "SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_WAVE_CYCLES SQ_BUSY_CYCLES" "SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_ACTIVE_INST_LDS SQ_INSTS_LDS" "SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_WAIT_ANY SQ_ACTIVE_INST_ANY" "SQ_INST_CYCLES_VMEM SQ_ACTIVE_INST_VMEM SQ_INSTS_VALU_MFMA_MOPS_BF16 SQ_INSTS_MFMA"; do
  rocprofv3 --kernel-trace --pmc $C --output-format csv -d $OUT/pass_$i -o x -- python $ROOT/tools/pp_probe.py $1 $2 $3 $4 6 > /dev/null 2> $OUT/pass_$i.err
  i=$((i+1))
done
cd $ROOT; export OUT
python - <<'PY' > gpurun_out/pp_pmc.txt
import csv, glob, collections, os
agg = collections.defaultdict(list)
for f in glob.glob(os.environ['OUT'] + '/pass_*/*counter_collection.csv'):
    for r in csv.DictReader(open(f)):
        if 'gemm256p' in r['Kernel_Name']:
            agg[r['Counter_Name']].append(float(r['Counter_Value']))
for k, v in sorted(agg.items()):
    print('%-34s launches %3d  mean %.4g' % (k, len(v), sum(v) / len(v)))
PY
cat gpurun_out/pp_pmc.txt
