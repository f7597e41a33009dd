# A/B of two builds of the library on the bench line: usage  bash tools/gpu_lib_ab.sh LIB_B BATCH...
# (alternating A = vqhmm/libvqhmm.so and B, twice each; prints ms/step and the dominant stage's time)
set -o pipefail
LB=$1; shift
OUT=$(mktemp -d)
for b in "$@"; do for rep in 1 2; do for lib in vq-vae-hmm-model_amd/vqhmm/libvqhmm.so $LB; do
  VQHMM_LIB_PATH=$PWD/$lib timeout -k 10 200 python bench.py --full --batch $b --no-cpu-baseline --no-hmm --steps 300 > $OUT/o.json 2>$OUT/err || exit 1
  python - $OUT/o.json $(basename $lib) $b <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read())
print(sys.argv[3], sys.argv[2], d["ms_per_step"], {k[:12]: v for k, v in d["step_kernels_us"].items() if not k.startswith("(")})
PY
done; done; done
