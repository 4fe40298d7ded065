# Evidence set for one BASELINE workload on an MI355X: bench line (--full), rocprofv3 kernel statistics, PMC passes (traffic + SQ / MFMA counters).
# usage: bash tools/evidence.sh C4 r03_v1   ->  evidence/r03_v1/C4_{bench.json,kernel_stats.csv,pmc.txt}   (EVIDENCE_DIR=<dir> instead of evidence/)
# full evidence run for one workload: bench line, kernel stats, PMC traffic
W=${1:-C4}; TAG=${2:-r03_v1}
cd "$(dirname "$0")/.."
OUT=${EVIDENCE_DIR:-evidence}/$TAG
mkdir -p $OUT && export TMPDIR=/tmp
python bench.py --full --workload $W --steps 100 --warmup 10 > $OUT/${W}_bench.json 2> $OUT/${W}_bench.err
rocprofv3 --kernel-trace --stats -d $OUT/prof_$W -o k -- python3 bench.py --full --workload $W --steps 50 --warmup 5 --no-cpu-baseline --no-batched > $OUT/prof_$W.log 2>&1
python tools/kstats.py $OUT/prof_$W/k_results.db > $OUT/${W}_kernel_stats.csv
i=0
for set in "FETCH_SIZE" "WRITE_SIZE" "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VALU_MFMA_F64 SQ_VALU_MFMA_BUSY_CYCLES" "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU"; do
  i=$((i+1))
  rocprofv3 --kernel-trace --pmc $set --output-format csv -d $OUT/pmc_${W}_$i -o p -- python3 bench.py --full --workload $W --steps 20 --warmup 5 --no-cpu-baseline --no-batched > $OUT/pmc_${W}_$i.log 2>&1 || echo "pmc pass $i failed"
done
python tools/pmc_aggregate.py $OUT --prefix pmc_${W}_ | grep -v "rocclr" > $OUT/${W}_pmc.txt
head -12 $OUT/${W}_kernel_stats.csv
grep -E "FETCH_SIZE|WRITE_SIZE" $OUT/${W}_pmc.txt
python -c "
import json;d=json.load(open('$OUT/${W}_bench.json'));print(d['value'],d['ms_per_step'],d['config']['kernel_launches_per_solve'],d['roofline'])"
