# r06h: elementwise products (plain products, product sums, tensor) in FP64 against build/vx/nowave
# (the integer products): parity, same-box HMult bench A/B, ResNet-level ops, ResNet-20 batch.
set -u
cd "$GRAFT_REPO_ROOT"
R=$GRAFT_REPO_ROOT
D=gpurun_out/r06h_$(date +%H%M%S)
mkdir -p $D
echo "logs in $D"
export TMPDIR=/tmp
step() { # name seconds cmd...
  local name=$1 secs=$2; shift 2
  timeout -k 10 $secs "$@" > $D/$name.log 2>&1
  local rc=$?
  echo "$name rc=$rc" | tee -a $D/rc.txt
  [ $rc -eq 0 ] || exit $rc
}
step parity 600 python -u -m pytest -x -q --timeout 300 --timeout-method thread -m gpu tests/test_gpu_parity.py tests/test_gpu_batch.py tests/test_bench_path.py
tail -2 $D/parity.log
for rep in 1 2; do
for lib in main nowave; do
  if [ $lib = main ]; then L=$R/fhe-gpt-2_amd/libmhe.so; else L=$R/build/vx/$lib/libmhe.so; fi
  MHE_LIB_PATH=$L step bench_${lib}_$rep 300 python -u bench.py --resnet-images 0 --no-cpu --steps 20 --warmup 3
  grep '^{' $D/bench_${lib}_$rep.log | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print('$lib', d['value'], d['ms_per_step'], d['roofline']['avg_launch_us'], d['roofline']['modup_col_avg_launch_us'], d.get('valu_roofline',{}).get('frac'))" | tee -a $D/bench.txt
done
done
for lib in main nowave; do
  if [ $lib = main ]; then L=$R/fhe-gpt-2_amd/libmhe.so; else L=$R/build/vx/$lib/libmhe.so; fi
  MHE_LIB_PATH=$L step u_${lib} 300 python -u scripts/ubench_ops.py --limbs 25 --ops ks,ks4,ks4s,rot4,hmult --reps 30
  grep '^{' $D/u_${lib}.log | sed "s/}/, \"v\": \"$lib\"}/" >> $D/ubench.jsonl
done
P=tests/golden/resnet/resnet20_params.bin; C=tests/golden/comp
for lib in main nowave; do
  if [ $lib = main ]; then LD=$R/fhe-gpt-2_amd; else LD=$R/build/vx/$lib; fi
  LD_LIBRARY_PATH=$LD MHE_RESNET_FIBERS=8 step resnet_$lib 400 ./build/resnet_test $P $C 24 20 3
  echo "$lib $(grep '^batch:' $D/resnet_$lib.log)" | tee -a $D/resnet.txt
done
