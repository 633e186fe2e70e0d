#!/bin/bash
# Builds libspx.so (HIP, gfx950 only) next to the package: shiftedproximaloperators.jl_amd/lib/libspx.so
# -ffp-contract=off: the reference (Julia) never fuses a*b+c; several kernels decide branches on such sums.
# One object per source file, compiled in parallel (no cross-file device calls, so no -fgpu-rdc), then one link.
# spx_batch.hip (the batched separable call, include/spx_batch.h) becomes a library of its own, lib/libspx_batch.so -- for
# SPX_LIB_NAME=X.so: X_batch.so -- linked against the first one (found next to it: rpath $ORIGIN).  spx_ibatch.hip (the batched
# iprox! call, include/spx_ibatch.h) becomes a third one in the same way: lib/libspx_ibatch.so, X_ibatch.so; spx_gbatch.hip (the
# batched group call, include/spx_gbatch.h) a fourth: lib/libspx_gbatch.so, X_gbatch.so; spx_gbinf_batch.hip (the batched Binf
# group call, include/spx_gbinf_batch.h) a fifth: lib/libspx_gbinf_batch.so, X_gbinf_batch.so; spx_b2_batch.hip (the batched
# ShiftedNormL1B2 call, include/spx_b2_batch.h) a sixth: lib/libspx_b2_batch.so, X_b2_batch.so; spx_topr_batch.hip (the batched
# top-r calls, include/spx_topr_batch.h) a seventh: lib/libspx_topr_batch.so, X_topr_batch.so; spx_lhalf_batch.hip (the batched
# RootNormLhalf(Box) calls, include/spx_lhalf_batch.h) an eighth: lib/libspx_lhalf_batch.so, X_lhalf_batch.so.
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
pids=()
objs=()
for s in "${SRCS[@]}"; do
  "$HIPCC" "${FLAGS[@]}" -c "$HERE/$s.hip" -o "$OBJ/$s.o" &
  pids+=($!)
  objs+=("$OBJ/$s.o")
done
"$HIPCC" "${FLAGS[@]}" -c "$HERE/spx_batch.hip" -o "$OBJ/spx_batch.o" &
pids+=($!)
"$HIPCC" "${FLAGS[@]}" -c "$HERE/spx_ibatch.hip" -o "$OBJ/spx_ibatch.o" &
pids+=($!)
"$HIPCC" "${FLAGS[@]}" -c "$HERE/spx_gbatch.hip" -o "$OBJ/spx_gbatch.o" &
pids+=($!)
"$HIPCC" "${FLAGS[@]}" -c "$HERE/spx_gbinf_batch.hip" -o "$OBJ/spx_gbinf_batch.o" &
pids+=($!)
"$HIPCC" "${FLAGS[@]}" -c "$HERE/spx_b2_batch.hip" -o "$OBJ/spx_b2_batch.o" &
pids+=($!)
"$HIPCC" "${FLAGS[@]}" -c "$HERE/spx_topr_batch.hip" -o "$OBJ/spx_topr_batch.o" &
pids+=($!)
"$HIPCC" "${FLAGS[@]}" -c "$HERE/spx_lhalf_batch.hip" -o "$OBJ/spx_lhalf_batch.o" &
pids+=($!)
fail=0
for p in "${pids[@]}"; do wait "$p" || fail=1; done
[ "$fail" = 0 ] || { echo "compile failed" >&2; exit 1; }
"$HIPCC" --offload-arch=gfx950 -shared -fPIC -fvisibility=hidden "${objs[@]}" -o "$OUT/$NAME.tmp"
mv -f "$OUT/$NAME.tmp" "$OUT/$NAME"
BATCH="${NAME%.so}_batch.so"
"$HIPCC" --offload-arch=gfx950 -shared -fPIC -fvisibility=hidden "$OBJ/spx_batch.o" -L"$OUT" -l:"$NAME" '-Wl,-rpath,$ORIGIN' \
  -o "$OUT/$BATCH.tmp"
mv -f "$OUT/$BATCH.tmp" "$OUT/$BATCH"
IBATCH="${NAME%.so}_ibatch.so"
"$HIPCC" --offload-arch=gfx950 -shared -fPIC -fvisibility=hidden "$OBJ/spx_ibatch.o" -L"$OUT" -l:"$NAME" '-Wl,-rpath,$ORIGIN' \
  -o "$OUT/$IBATCH.tmp"
mv -f "$OUT/$IBATCH.tmp" "$OUT/$IBATCH"
GBATCH="${NAME%.so}_gbatch.so"
"$HIPCC" --offload-arch=gfx950 -shared -fPIC -fvisibility=hidden "$OBJ/spx_gbatch.o" -L"$OUT" -l:"$NAME" '-Wl,-rpath,$ORIGIN' \
  -o "$OUT/$GBATCH.tmp"
mv -f "$OUT/$GBATCH.tmp" "$OUT/$GBATCH"
GBINF="${NAME%.so}_gbinf_batch.so"
"$HIPCC" --offload-arch=gfx950 -shared -fPIC -fvisibility=hidden "$OBJ/spx_gbinf_batch.o" -L"$OUT" -l:"$NAME" '-Wl,-rpath,$ORIGIN' \
  -o "$OUT/$GBINF.tmp"
mv -f "$OUT/$GBINF.tmp" "$OUT/$GBINF"
B2BATCH="${NAME%.so}_b2_batch.so"
"$HIPCC" --offload-arch=gfx950 -shared -fPIC -fvisibility=hidden "$OBJ/spx_b2_batch.o" -L"$OUT" -l:"$NAME" '-Wl,-rpath,$ORIGIN' \
  -o "$OUT/$B2BATCH.tmp"
mv -f "$OUT/$B2BATCH.tmp" "$OUT/$B2BATCH"
TOPRBATCH="${NAME%.so}_topr_batch.so"
"$HIPCC" --offload-arch=gfx950 -shared -fPIC -fvisibility=hidden "$OBJ/spx_topr_batch.o" -L"$OUT" -l:"$NAME" '-Wl,-rpath,$ORIGIN' \
  -o "$OUT/$TOPRBATCH.tmp"
mv -f "$OUT/$TOPRBATCH.tmp" "$OUT/$TOPRBATCH"
LHALFBATCH="${NAME%.so}_lhalf_batch.so"
"$HIPCC" --offload-arch=gfx950 -shared -fPIC -fvisibility=hidden "$OBJ/spx_lhalf_batch.o" -L"$OUT" -l:"$NAME" '-Wl,-rpath,$ORIGIN' \
  -o "$OUT/$LHALFBATCH.tmp"
mv -f "$OUT/$LHALFBATCH.tmp" "$OUT/$LHALFBATCH"
echo "built $OUT/$NAME"
