#!/bin/bash
# tools/sanitize_beam_host.sh  ->  builds and runs a stand-alone CPU program (tools/sanitize_beam_host.cpp) that drives the argument
# handling of csrc/api_beam.hip (kws_ctc_beam_search) -- every refusal, all of them decided before the device is probed, and the probe itself -- under AddressSanitizer and
# UndefinedBehaviorSanitizer.  The host halves of the api_*.hip files, weight_pack.hip and selftest.hip are compiled host-only with
# the sanitizers and linked with the kernel launchers left unresolved: no refusal reaches one.  Runs on a machine WITHOUT a GPU (the
# probe is expected to answer KWS_ERR_NO_DEVICE); nothing is loaded into Python.  Exit 0: every refusal as expected, no report.
set -e -o pipefail
ROOT=$(cd $(dirname $0)/.. && pwd)
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}; LLVM=${LLVM_BIN:-/opt/rocm/lib/llvm/bin}; ROCM_LIB=${ROCM_LIB:-/opt/rocm/lib}
C=$ROOT/keyword_spotting_amd/csrc
W=$(mktemp -d); trap 'rm -rf $W' EXIT
pids=()
for f in $C/api_*.hip $C/weight_pack.hip $C/selftest.hip; do
  $HIPCC --offload-arch=gfx950 --cuda-host-only -O1 -g -std=c++17 -fPIC -I$ROOT/include -I$C -fsanitize=address,undefined -fno-omit-frame-pointer \
    -c $f -o $W/$(basename $f .hip).o &
  pids+=($!)
done
for p in "${pids[@]}"; do wait $p || { echo "sanitize_beam_host: a host-only compile failed (see above)"; exit 1; }; done
$LLVM/clang++ -std=c++17 -fsanitize=address,undefined -I$ROOT/include $ROOT/tools/sanitize_beam_host.cpp $W/*.o -L$ROCM_LIB -lamdhip64 \
  -Wl,-rpath,$ROCM_LIB -Wl,--unresolved-symbols=ignore-all -o $W/sanitize_beam_host
$W/sanitize_beam_host
