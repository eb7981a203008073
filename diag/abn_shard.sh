#!/bin/bash
# same-box A/B of library builds on the 1250-clip shard (a chain encode of ONE round), ROUNDS interleaved passes; per
# variant the shard's kernel_ms and ms_per_step of every pass, their median, minimum and min-to-max range:
#   ROUNDS=5 diag/abn_shard.sh name1 name2 ...   ("full" = the product library, others diag/libflo_NAME.so)
# (the bench's main leg is cut to 256 clips: the smallest batch that takes the chain kernel, whose name the shard leg reuses)
R=$(cd "$(dirname "$0")/.." && pwd); cd $R
log=$(mktemp); trap 'rm -f $log' EXIT
for r in $(seq 1 ${ROUNDS:-5}); do
  for v in "$@"; do
    if [ "$v" != "full" ]; then export FLO_HIP_LIB=$R/diag/libflo_$v.so; else unset FLO_HIP_LIB; fi
    out=$(timeout -k 10 300 python bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-single-clip --no-lossless --no-e2e --clips-per-gpu 256 2>/dev/null) || { echo "$v: bench failed ($?)"; exit 1; }
    echo "$v $(echo "$out" | python -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1])['shard_1250']; print(d['kernel_ms'], d['ms_per_step'])")" | tee -a $log
  done
done
python - $log <<'PY'
import sys,collections,statistics
d=collections.OrderedDict()
for l in open(sys.argv[1]):
    v,k,s=l.split(); d.setdefault(v,([],[]))[0].append(float(k)); d[v][1].append(float(s))
for v,(k,s) in d.items():
    for nm,x in (("kernel_ms",k),("ms_per_step",s)):
        print(f"{v:10s} {nm:11s} median {statistics.median(x):7.4f}  min {min(x):7.4f}  range {max(x)-min(x):6.4f} ({100*(max(x)-min(x))/min(x):.2f} %)  n={len(x)}  {x}")
PY
