#!/bin/bash
# Host sanitizers for the cubed-sphere planner and the index-list plan introspection (no GPU):
# builds the library's sources once, host code instrumented with AddressSanitizer +
# UndefinedBehaviorSanitizer (each -fsanitize= after -Xarch_host, so no device code is touched),
# links the stand-alone programs tests/cpp/cs_host_check.cpp (unpack plans),
# cs_self_host_check.cpp (fused self exchange), cs_put_host_check.cpp (put),
# uplan_segment_host_check.cpp (ghx_uplan_segment), uself_host_check.cpp (ghx_uself_create),
# umixed_host_check.cpp (ghx_umixed_create), uaccum_host_check.cpp (ghx_uaccum_create),
# saccum_host_check.cpp (ghx_saccum_create), sget_host_check.cpp (ghx_saccum_get_create),
# cs_adjoint_host_check.cpp (the reverse pack of ghx_cs_exchange_adjoint_create) and
# cs_get_host_check.cpp (the get plan of ghx_cs_exchange_adjoint_self_create) against them and runs them one after the other,
# stopping at the first failure. Each program has its own main: nothing is preloaded.
# Usage: bash tools/cs_host_sanitize.sh [scratch dir, default /tmp/ghx_cs_san]
set -e
S=${1:-/tmp/ghx_cs_san}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
mkdir -p "$S"
SAN="-Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -Xarch_host -fno-omit-frame-pointer"
FLAGS="-std=c++17 -O1 -g -Wall -Wno-unused-parameter -I$ROOT/include --offload-arch=gfx950 $SAN"
C="$ROOT/ghex_amd/csrc"
PROGS="cs_host_check cs_self_host_check cs_put_host_check uplan_segment_host_check uself_host_check umixed_host_check uaccum_host_check saccum_host_check sget_host_check cs_adjoint_host_check cs_get_host_check"
OBJS=""
PIDS=""
for f in ghx_kernels.hip ghx_epochs.hip ghx_copier.hip ghx_accum.hip ghx_accum_plan.cpp ghx_saccum_plan.cpp ghx_plan.cpp ghx_exchange.cpp ghx_cache.cpp ghx_abi.cpp \
         ghx_pattern.cpp ghx_cubed_sphere.cpp ghx_upattern.cpp ghx_pipeline.cpp; do
  o="$S/${f%.*}.o"
  if [ "${f##*.}" = hip ]; then x="-munsafe-fp-atomics"; else x=""; fi
  $HIPCC $FLAGS $x -c "$C/$f" -o "$o" &
  PIDS="$PIDS $!"
  OBJS="$OBJS $o"
done
for p in $PROGS; do
  $HIPCC $FLAGS -c "$ROOT/tests/cpp/$p.cpp" -o "$S/$p.o" &
  PIDS="$PIDS $!"
done
for pid in $PIDS; do wait "$pid"; done
for p in $PROGS; do
  $HIPCC --offload-arch=gfx950 -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -o "$S/$p" \
    "$S/$p.o" $OBJS -ldl -L/opt/rocm/lib -lhsa-runtime64
  ASAN_OPTIONS=detect_leaks=1:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 "$S/$p"
done
