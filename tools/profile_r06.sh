#!/bin/bash
# Round-6 measurement (GPU box).  Outputs: gpurun_out/r06p/ (copy what should be judged into profiles/).
#   rocprofv3 kernel traces of the five bench workloads + the CRNN at 32 crops per GPU: per-kernel statistics and the launch
#   sequence of one replayed step; FETCH_SIZE / WRITE_SIZE PMC passes (separate passes) of ALL five workloads ->
#   pmc_traffic_<workload>.json, stamped with the kernel-source hash bench.py checks.
# usage: bash tools/profile_r06.sh [quick|pmc]      (quick: no PMC passes; pmc: only the PMC passes)
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
O=gpurun_out/r06p; mkdir -p $O
MODE=$1
trace() {   # name, marker, bench args...
  if [ "$MODE" = "pmc" ]; then return; fi
  local name=$1; local marker=$2; shift; shift
  timeout 300 rocprofv3 --kernel-trace -d $O/trace_$name -- python bench.py "$@" --no-cpu-baseline --no-secondary --no-kernel-timer --steps 10 --warmup 3 > $O/trace_$name.log 2>&1
  local db=$(find $O/trace_$name -name "*.db" | head -1)
  if [ -n "$db" ]; then
    python tools/rocpd_stats.py "$db" > $O/${name}_kernel_stats.csv 2>&1
    python tools/rocpd_sequence.py "$db" --marker $marker > $O/${name}_step_sequence.txt 2>&1
    head -1 $O/${name}_step_sequence.txt
  fi
  grep -o '"ms_per_step": [0-9.]*' $O/trace_$name.log | head -1
  rm -rf $O/trace_$name
}
trace crnn adam_kernel --workload crnn
trace crnn_b32 adam_kernel --workload crnn --batch 32
trace res50ppm adam_kernel --workload res50ppm
trace fpn_attention adam_kernel --workload fpn_attention
trace fpn_attention_random_coins adam_kernel --workload fpn_attention --teacher-forcing random
trace db sgd_kernel --workload db
# the configuration every rank runs when WORLD_SIZE > 1 (one-pass BatchNorm backward off), at the 8-GPU strong-scaling shard and
# at configs[3]'s per-GPU batch: the kernel statistics DESIGN.md section 7 bases its 8-GPU model on
export MEGREADER_TUNING=bn_onepass=0
trace crnn_b32_world_gt1 adam_kernel --workload crnn --batch 32
trace fpn_attention_world_gt1 adam_kernel --workload fpn_attention
unset MEGREADER_TUNING
if [ "$1" != "quick" ]; then
pmc() {   # json name, bench args...
  local w=$1; shift
  for c in FETCH_SIZE WRITE_SIZE; do
    timeout 500 rocprofv3 --pmc $c --output-format csv -d $O/pmc_${w}_$c -- python bench.py "$@" --no-secondary --no-cpu-baseline --no-graph --no-kernel-timer --steps 3 --warmup 2 > $O/pmc_${w}_$c.log 2>&1
    f=$(find $O/pmc_${w}_$c -name "*counter_collection.csv" | head -1)
    if [ -n "$f" ]; then python tools/pmc_summary.py "$f" > $O/pmc_${w}_$c.txt 2>&1; fi
    rm -rf $O/pmc_${w}_$c
  done
  python tools/pmc_to_json.py $O/pmc_${w}_FETCH_SIZE.txt $O/pmc_${w}_WRITE_SIZE.txt $O/pmc_traffic_${w}.json > /dev/null 2>&1
  ls -la $O/pmc_traffic_${w}.json
}
pmc crnn --workload crnn
pmc res50ppm --workload res50ppm
pmc fpn_attention --workload fpn_attention
pmc db --workload db
pmc res50ppm_64x256 --workload res50ppm --crop 64x256
fi
echo done
if [ "$MODE" = "pmc" ]; then exit 0; fi
# ---- extras of round 6: the configuration world > 1 actually runs (bn_onepass = 0), the multi-GPU code path on one rank, the
# reference-precision line, the MFMA ceiling
{
echo "# bench.py, hipGraph replay, one MI355X: default vs MEGREADER_TUNING=bn_onepass=0 (what every rank runs when WORLD_SIZE > 1: the"
echo "# one-pass BatchNorm backward is a resident-grid kernel and is refused beside collectives) -- per-GPU cost of that rule"
B="--no-cpu-baseline --no-secondary --no-kernel-timer --steps 30 --warmup 5"
for wl in "crnn" "crnn --batch 32" "res50ppm" "fpn_attention" "db"; do
  for cfg in "bn_onepass=1" "bn_onepass=0"; do
    ms=$(MEGREADER_TUNING=$cfg timeout 300 python bench.py --workload $wl $B 2>/dev/null | grep -o '"ms_per_step": [0-9.]*' | head -1)
    echo "$wl | $cfg | $ms"
  done
done
} > $O/ab_world_gt1_configuration.txt 2>&1
RANK=0 LOCAL_RANK=0 WORLD_SIZE=1 MASTER_ADDR=127.0.0.1 MASTER_PORT=29517 timeout 300 python bench.py --full --force-ddp --ddp-mode capture --no-cpu-baseline --no-secondary --steps 20 --warmup 5 > $O/bench_force_ddp_capture.json 2> $O/bench_force_ddp_capture.err
timeout 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29518 bench.py --gpus 1 --steps 20 --warmup 5 --full --no-secondary --no-cpu-baseline > $O/bench_torchrun_n1.json 2> $O/bench_torchrun_n1.err
timeout 300 python bench.py --full --workload res50ppm --dtype f32 --no-secondary --steps 10 --warmup 3 > $O/bench_res50ppm_f32.json 2> $O/bench_res50ppm_f32.err
tools/mfma_ceiling > $O/mfma_ceiling.txt 2>&1
timeout 300 python tools/microbench_lstm.py --phases 2>&1 | grep -v amdgpu.ids > $O/lstm_phases.txt
# the persistent decode kernels beside the per-step launches they replace, with the kernels' own phase clock
{
for cfg in "32 64 552 32" "32 64 552 32 coins" "16 64 552 32"; do
  echo "## python tools/microbench_decode.py $cfg"
  timeout 300 python tools/microbench_decode.py $cfg 2>&1 | grep -v amdgpu.ids
done
echo "## MEGREADER_TUNING=decode_persist=2 (no XCD-colocating block map): python tools/microbench_decode.py 32 64 552 32"
MEGREADER_TUNING=decode_persist=2 timeout 300 python tools/microbench_decode.py 32 64 552 32 2>&1 | grep -v amdgpu.ids | grep "persistent\|status"
echo "## bench.py --workload fpn_attention, MEGREADER_DECODE_PERSIST = 1 / fwd / bwd / 0, fixed teacher forcing then the YAML-default coins"
B="--no-cpu-baseline --no-secondary --no-kernel-timer --steps 30 --warmup 5"
for tf in "" "--teacher-forcing random"; do
  for p in 1 fwd bwd 0; do
    ms=$(MEGREADER_DECODE_PERSIST=$p timeout 300 python bench.py --workload fpn_attention $tf $B 2>/dev/null | grep -o '"ms_per_step": [0-9.]*' | head -1)
    echo "fpn_attention $tf | MEGREADER_DECODE_PERSIST=$p | $ms"
  done
done
} > $O/decode_persist_microbench.txt 2>&1
python bench.py --full > $O/bench_default_final.json 2> $O/bench_default_final.err
echo extras done
