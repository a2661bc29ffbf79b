# HMult bench with the nontemporal-access variants of libmhe (exp/libmhe_nt*.so) vs the default.
# Logs and the summary go under $OUT_DIR (default: out/).
set -u
R="$(cd "$(dirname "$0")/.." && pwd)"
cd "$R"
O="${OUT_DIR:-out}"
mkdir -p "$O"
for v in ${NT_VARIANTS:-base 1 6 7 base}; do
  if [ "$v" = base ]; then unset MHE_LIB_PATH; else export MHE_LIB_PATH="$R/exp/libmhe_$v.so"; fi
  # --full for the kernel's own launch time (avg_launch_us); no ResNet or CPU legs
  timeout -k 10 200 python bench.py --full --no-cpu --resnet-images 0 --steps 10 --warmup 2 > "$O/nt_$v.log" 2>&1 || exit $?
  echo "$v $(grep -o '"value": [0-9.]*' "$O/nt_$v.log") $(grep -o '"avg_launch_us": [0-9.]*' "$O/nt_$v.log")" >> "$O/nt_summary.txt"
done
