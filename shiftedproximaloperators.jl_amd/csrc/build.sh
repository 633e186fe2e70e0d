#!/bin/bash
# Builds libspx.so (HIP, gfx950 only) next to the package: shiftedproximaloperators.jl_amd/lib/libspx.so
# -ffp-contract=off: the reference (Julia) never fuses a*b+c; several kernels decide branches on such sums.
# One object per source file, compiled in parallel (no cross-file device calls, so no -fgpu-rdc), then one link.
# Each stem X of BATCH_LIBS (spx_X.hip, include/spx_X.h: a batched call) becomes a library of its own, lib/libspx_X.so -- for
# SPX_LIB_NAME=Y.so: Y_X.so -- linked against the first one (found next to it: rpath $ORIGIN).  The array names the keys of
# BATCH_LIBRARIES in _lib.py (tests/test_batch_libraries.py).
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
ROOT="$(cd "$HERE/../.." && pwd)"
OUT="$HERE/../lib"
NAME="${SPX_LIB_NAME:-libspx.so}"
OBJ="$OUT/obj_${NAME%.so}"
mkdir -p "$OUT" "$OBJ"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS=(--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fvisibility=hidden
       -Wall -Wno-unused-variable -Wno-unused-but-set-variable -I"$ROOT/include" -I"$HERE" "$@")
SRCS=(spx_ctx spx_separable spx_select spx_group spx_group_team spx_group_f32 spx_objective spx_b2 spx_host)
BATCH_LIBS=(batch ibatch gbatch gbinf_batch b2_batch topr_batch lhalf_batch)
pids=()
objs=()
for s in "${SRCS[@]}"; do
  "$HIPCC" "${FLAGS[@]}" -c "$HERE/$s.hip" -o "$OBJ/$s.o" &
  pids+=($!)
  objs+=("$OBJ/$s.o")
done
for b in "${BATCH_LIBS[@]}"; do
  "$HIPCC" "${FLAGS[@]}" -c "$HERE/spx_$b.hip" -o "$OBJ/spx_$b.o" &
  pids+=($!)
done
fail=0
for p in "${pids[@]}"; do wait "$p" || fail=1; done
[ "$fail" = 0 ] || { echo "compile failed" >&2; exit 1; }
"$HIPCC" --offload-arch=gfx950 -shared -fPIC -fvisibility=hidden "${objs[@]}" -o "$OUT/$NAME.tmp"
mv -f "$OUT/$NAME.tmp" "$OUT/$NAME"
for b in "${BATCH_LIBS[@]}"; do
  LIB="${NAME%.so}_$b.so"
  "$HIPCC" --offload-arch=gfx950 -shared -fPIC -fvisibility=hidden "$OBJ/spx_$b.o" -L"$OUT" -l:"$NAME" '-Wl,-rpath,$ORIGIN' \
    -o "$OUT/$LIB.tmp"
  mv -f "$OUT/$LIB.tmp" "$OUT/$LIB"
done
echo "built $OUT/$NAME"
