# tools/profile.sh, its summaries, and the full bench line (--full: every secondary leg) beside them.
# TAG = the profile's name; OUT_ROOT = where everything goes (default build/bench_out)
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); O=${OUT_ROOT:-$R/build/bench_out}; P=$O/prof_${TAG:-r1}; S=$O/summ_${TAG:-r1}
OUT_ROOT=$O bash $R/tools/profile.sh ${TAG:-r1} || exit 1
mkdir -p $S
python3 $R/tools/profile_summary.py $P $S > $S/summary.txt 2>&1 || { rm -rf $P; exit 2; }
python3 $R/tools/busy.py $(ls $P/trace/*kernel_trace.csv | head -1) 250 > $S/busy.txt 2>&1
cp $P/trace_bench.json $S/ 2>/dev/null
rm -rf $P
cd $R && timeout -k 10 300 python3 bench.py --full > $S/bench.json 2> $S/bench.err || exit 3
echo all-done
