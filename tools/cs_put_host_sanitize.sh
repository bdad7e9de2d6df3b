#!/bin/bash
# Host sanitizers for the cubed-sphere put's planner (no GPU): builds the stand-alone program
# tests/cpp/cs_put_host_check.cpp together with the library's sources, host code instrumented with
# AddressSanitizer + UndefinedBehaviorSanitizer (each -fsanitize= after -Xarch_host, so no device
# code is touched), and runs it. The program has its own main: nothing is preloaded.
# Usage: bash tools/cs_put_host_sanitize.sh [scratch dir, default /tmp/ghx_cs_put_san]
set -e
S=${1:-/tmp/ghx_cs_put_san}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
mkdir -p "$S"
SAN="-Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -Xarch_host -fno-omit-frame-pointer"
FLAGS="-std=c++17 -O1 -g -Wall -Wno-unused-parameter -I$ROOT/include --offload-arch=gfx950 $SAN"
C="$ROOT/ghex_amd/csrc"
OBJS=""
for f in ghx_kernels.hip ghx_epochs.hip ghx_copier.hip ghx_plan.cpp ghx_abi.cpp ghx_pattern.cpp \
         ghx_cubed_sphere.cpp ghx_upattern.cpp ghx_pipeline.cpp; do
  o="$S/${f%.*}.o"
  if [ "${f##*.}" = hip ]; then x="-munsafe-fp-atomics"; else x=""; fi
  $HIPCC $FLAGS $x -c "$C/$f" -o "$o" &
  OBJS="$OBJS $o"
done
$HIPCC $FLAGS -c "$ROOT/tests/cpp/cs_put_host_check.cpp" -o "$S/cs_put_host_check.o" &
wait
$HIPCC --offload-arch=gfx950 -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -o "$S/cs_put_host_check" \
  "$S/cs_put_host_check.o" $OBJS -ldl -L/opt/rocm/lib -lhsa-runtime64
ASAN_OPTIONS=detect_leaks=1:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 \
  "$S/cs_put_host_check"
