# K11w timing ablations (libraries from tools/probes/k11w_ablate.py), interleaved
# with the unpatched probe build: v1 and v5 (K11w) per shape, bs128.  K11w is
# not in the production library: every arm, "probe" included, is a scratch
# library that exports tcamd_x3_dense_fused_ws
# (python tools/probes/build_variant.py --unit k11w tools/probes/k11w.hip).
set -o pipefail
cd "${GRAFT_REPO_ROOT:-.}"
export PYTHONPATH=$PWD
for r in 1 2; do
for v in probe ${K11W_ARMS:-noconv nomma1 no3x3}; do
  if [ $v = probe ]; then lib=$PWD/k12ab/libtcamd_hip_k11w.so; else lib=$PWD/k12ab/libtcamd_hip_k11w_$v.so; fi
  if [ ! -f "$lib" ]; then echo "$lib is missing: build it first (see the header of this script)"; exit 1; fi
  export TCAMD_HIP_LIB=$lib
  echo "== $v"
  timeout -k 10 120 python -u tools/k11x_ab.py --versions 1,5 --imgs 128 --shapes 56:64,56:224,28:480 --rounds 2 || exit 1
done
done
