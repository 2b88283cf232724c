# Round-end evidence run (GPU box): full GPU test suite, bench lines, rocprofv3 kernel stats, PMC traffic and SQ counters.
#     tools/_measure.sh TAG OUT        everything lands in OUT/m_*; tools/install_profiles.py TAG OUT copies the summaries into profiles/.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
TAG=${1:?usage: tools/_measure.sh TAG OUT}
mkdir -p "${2:?usage: tools/_measure.sh TAG OUT}"
OUT=$(cd "$2" && pwd)
cd "$ROOT"
timeout -k 10 1000 python -m pytest tests -x -q -m gpu > "$OUT/m_gpu_tests.log" 2>&1
tail -2 "$OUT/m_gpu_tests.log"
timeout -k 10 600 python bench.py --full > "$OUT/m_bench.json" 2> "$OUT/m_bench.err"
timeout -k 10 300 python bench.py --full --config cfg2 > "$OUT/m_bench_cfg2.json" 2> "$OUT/m_bench_cfg2.err"
timeout -k 10 300 python bench.py --full --config cfg4 > "$OUT/m_bench_cfg4.json" 2> "$OUT/m_bench_cfg4.err"
timeout -k 10 300 python bench.py --full --config cfg5 > "$OUT/m_bench_cfg5.json" 2> "$OUT/m_bench_cfg5.err"
timeout -k 10 400 python bench.py --config cfg4 --train > "$OUT/m_bench_cfg4_train.json" 2> "$OUT/m_bench_cfg4_train.err"
timeout -k 10 400 python bench.py --config cfg5 --train > "$OUT/m_bench_cfg5_train.json" 2> "$OUT/m_bench_cfg5_train.err"
timeout -k 10 300 python bench.py --use-checkpoint > "$OUT/m_bench_cfg3_use_checkpoint.json" 2> "$OUT/m_bench_cfg3_use_checkpoint.err"
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/m_prof" -- python3 "$ROOT/bench.py" --full --no-cpu-baseline --steps 20 > "$OUT/m_prof_bench.json" 2> "$OUT/m_prof.err"
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$OUT/m_pmc_fetch" -- python3 "$ROOT/bench.py" --steps 3 --warmup 1 > /dev/null 2> "$OUT/m_pmc_fetch.err"
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d "$OUT/m_pmc_write" -- python3 "$ROOT/bench.py" --steps 3 --warmup 1 > /dev/null 2> "$OUT/m_pmc_write.err"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/s_prof" -- python3 "$ROOT/bench.py" --steps 10 --warmup 3 > /dev/null 2> "$OUT/s_prof.err"
timeout -k 10 300 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_INSTS_VALU SQ_INSTS_MFMA --output-format csv -d "$OUT/s_pmcA" -- python3 "$ROOT/bench.py" --steps 2 --warmup 1 > /dev/null 2> "$OUT/s_pmcA.err"
timeout -k 10 300 rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_LDS SQ_INSTS_SALU SQ_INSTS_VMEM SQ_BUSY_CYCLES SQ_WAIT_INST_LDS --output-format csv -d "$OUT/s_pmcB" -- python3 "$ROOT/bench.py" --steps 2 --warmup 1 > /dev/null 2> "$OUT/s_pmcB.err"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/m_prof_cfg4" -- python3 "$ROOT/bench.py" --config cfg4 --no-graph --steps 10 --warmup 2 > /dev/null 2> "$OUT/m_prof_cfg4.err"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/m_prof_cfg4_train" -- python3 "$ROOT/bench.py" --config cfg4 --train --no-graph --steps 3 --warmup 1 > /dev/null 2> "$OUT/m_prof_cfg4_train.err"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/m_prof_cfg5_train" -- python3 "$ROOT/bench.py" --config cfg5 --train --no-graph --steps 3 --warmup 1 > /dev/null 2> "$OUT/m_prof_cfg5_train.err"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/m_prof_cfg5" -- python3 "$ROOT/bench.py" --config cfg5 --no-graph --steps 10 --warmup 2 > /dev/null 2> "$OUT/m_prof_cfg5.err"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/m_prof_cfg2" -- python3 "$ROOT/bench.py" --config cfg2 --no-graph --steps 50 --warmup 2 > /dev/null 2> "$OUT/m_prof_cfg2.err"
cd "$ROOT"
python tools/sq_summary.py "$OUT" s_ > "$OUT/m_sq.txt"
timeout -k 10 120 python __graft_entry__.py --smoke > "$OUT/m_smoke.log" 2>&1
tail -2 "$OUT/m_smoke.log"
cut -c1-500 "$OUT/m_bench.json"
