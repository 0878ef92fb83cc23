#!/bin/bash
# A/B helper: build a variant of the library that differs only in compile-time knobs of the HIP sources
# (e.g. -DTWK_TRACE_WAVES=7 -DTWK_TRACE_STACK_LDS=20) into build/lib_<name>.so; the host objects are reused.
# usage: tools/ab_variant.sh <name> <extra hipcc flags...>     then on the GPU box:
#        TWK_LIB=build/lib_<name>.so python bench.py --no-cpu-baseline
# The sources, the host objects and the flags are the Makefile's own (its print-% target): every HIP source is compiled with
# the extra flags, so a knob in device_types.h reaches every object that reads it.
set -e
NAME=$1; shift
cd "$(dirname "$0")/../tweeker_raytracer_amd/csrc"
make -s > /dev/null
HIP_SRCS=$(make -s print-HIP_SRCS)
HOST_OBJS=$(make -s print-HOST_SRCS | sed 's/\.cpp/.o/g')
FLAGS=$(make -s print-HIPFLAGS)
OUT=../../build/$NAME
mkdir -p $OUT
OBJS=""
for f in $HIP_SRCS; do
  OBJS="$OBJS $OUT/${f%.hip}.o"
  ( hipcc $FLAGS "$@" -c $f -o $OUT/${f%.hip}.o 2>&1 | grep -E "error" || true ) &
done
wait
hipcc -shared -fPIC --offload-arch=gfx950 -o ../../build/lib_$NAME.so $OBJS $HOST_OBJS -lz
ls -la ../../build/lib_$NAME.so
