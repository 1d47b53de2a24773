#!/bin/bash
# Build libavvad_hip.so for gfx950 (MI355X).  Usage: csrc/build.sh [extra hipcc flags]
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
OUT="$HERE/../lib"
mkdir -p "$OUT" "$HERE/_obj"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -I$HERE/../../include -I$HERE $*"
# every source once: compiled in parallel, then linked
SRCS="gemm trunk lstm misc wavenet mcb stft target stats scores stoi spectral_loss mix lip stream stft_stream istft istft_stream resample"
pids=()
objs=()
for f in $SRCS; do
  ( hipcc $FLAGS -c "$HERE/$f.hip" -o "$HERE/_obj/$f.o" ) &
  pids+=($!)
  objs+=("$HERE/_obj/$f.o")
done
for p in "${pids[@]}"; do wait "$p"; done
hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT/libavvad_hip.so" "${objs[@]}"
echo "built $OUT/libavvad_hip.so"
