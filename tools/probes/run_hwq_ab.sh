# files-to-files regions of bench.py with 4 (default) and 8 hardware queues, same box, alternating: bash run_hwq_ab.sh [output folder]
set -e
O=${1:-hwq_ab}
mkdir -p $O
for q in 4 8 4 8; do
  GPU_MAX_HW_QUEUES=$q timeout -k 10 400 python bench.py --full --steps 8 --warmup 3 --no-r101 --no-fp16-b32 --no-two-model --no-cpu-baseline --no-serial --no-profile --no-lzw --detail $O/detail_$q.json > $O/q$q.log 2> $O/q$q.err || { tail -5 $O/q$q.err; exit 1; }
  python - <<PY
import json
d=json.loads([l for l in open("$O/q$q.log") if l.startswith("{")][-1])
r=d["regions"]
print("queues $q", d["value"], {k:r[k] for k in ("fp16","e2e_f32","e2e_f16","e2e_chained_f16","e2e_crowns_f16","e2e_crowns_f16_ratio","e2e_crowns_chained_f16_ratio","predict_tiles_f32","predict_tiles_f16","predict_tiles_f32_ratio","predict_tiles_f16_ratio") if k in r})
PY
done
