#!/bin/bash
# Builds libslu_hip.so and, next to it, libslu_decode.so (include/slu_decode.h), libslu_intents.so
# (include/slu_intents.h), libslu_resample.so (include/slu_resample.h) and libslu_room.so (include/slu_room.h) for gfx950 (MI355X) in-tree.  hipcc cross-compiles without a GPU.
# Out-of-date translation units are compiled in parallel (SLU_BUILD_JOBS, default = the host's cores, max 16).
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
OUT="$HERE/../lib"
mkdir -p "$OUT"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function ${SLU_EXTRA_FLAGS:-}"
JOBS="${SLU_BUILD_JOBS:-$(( $(nproc) < 16 ? $(nproc) : 16 ))}"
UNITS="slu_api slu_sinc slu_wconv slu_wconv_bf16 slu_gemm slu_gemm_bf16 slu_gru slu_gru_step slu_gru_bf16 slu_gru_proj slu_pool slu_head slu_optim slu_framece slu_comm slu_comm_ipc slu_seq2seq slu_beam slu_trie slu_augment slu_varlen slu_framepack slu_ctc"
# libslu_decode.so: its units see include/slu_decode.h as well
DECODE_UNITS="slu_ctc_beam"
# libslu_intents.so: its units see include/slu_intents.h as well
INTENTS_UNITS="slu_intent_set"
# libslu_resample.so: its units see include/slu_resample.h as well
RESAMPLE_UNITS="slu_resample"
# libslu_room.so: its units see include/slu_room.h as well
ROOM_UNITS="slu_room"
OBJS=()
DECODE_OBJS=()
INTENTS_OBJS=()
RESAMPLE_OBJS=()
ROOM_OBJS=()
STALE=()
for f in $UNITS $DECODE_UNITS $INTENTS_UNITS $RESAMPLE_UNITS $ROOM_UNITS; do
  if [ ! -f "$OUT/$f.o" ] || [ "$HERE/$f.hip" -nt "$OUT/$f.o" ] || [ "$HERE/slu_common.h" -nt "$OUT/$f.o" ] || [ "$HERE/slu_bf16.h" -nt "$OUT/$f.o" ] || [ "$HERE/slu_philox.h" -nt "$OUT/$f.o" ] || [ "$HERE/slu_gemm_tile.h" -nt "$OUT/$f.o" ] || [ "$HERE/slu_reduce.h" -nt "$OUT/$f.o" ] \
     || [ "$HERE/../../include/slu_hip.h" -nt "$OUT/$f.o" ]; then
    STALE+=("$f")
  elif [[ " $DECODE_UNITS " == *" $f "* ]] && [ "$HERE/../../include/slu_decode.h" -nt "$OUT/$f.o" ]; then
    STALE+=("$f")
  elif [[ " $INTENTS_UNITS " == *" $f "* ]] && [ "$HERE/../../include/slu_intents.h" -nt "$OUT/$f.o" ]; then
    STALE+=("$f")
  elif [[ " $RESAMPLE_UNITS " == *" $f "* ]] && [ "$HERE/../../include/slu_resample.h" -nt "$OUT/$f.o" ]; then
    STALE+=("$f")
  elif [[ " $ROOM_UNITS " == *" $f "* ]] && [ "$HERE/../../include/slu_room.h" -nt "$OUT/$f.o" ]; then
    STALE+=("$f")
  fi
  if [[ " $DECODE_UNITS " == *" $f "* ]]; then DECODE_OBJS+=("$OUT/$f.o")
  elif [[ " $INTENTS_UNITS " == *" $f "* ]]; then INTENTS_OBJS+=("$OUT/$f.o")
  elif [[ " $RESAMPLE_UNITS " == *" $f "* ]]; then RESAMPLE_OBJS+=("$OUT/$f.o")
  elif [[ " $ROOM_UNITS " == *" $f "* ]]; then ROOM_OBJS+=("$OUT/$f.o")
  else OBJS+=("$OUT/$f.o"); fi
done
if [ "${#STALE[@]}" -gt 0 ]; then
  printf '%s\n' "${STALE[@]}" | xargs -P "$JOBS" -I{} bash -c "echo '[build] {}.hip'; '$HIPCC' $FLAGS -c '$HERE/{}.hip' -o '$OUT/{}.o.tmp' && mv '$OUT/{}.o.tmp' '$OUT/{}.o'"
fi
"$HIPCC" --offload-arch=gfx950 -shared -fPIC "${OBJS[@]}" -ldl -o "$OUT/libslu_hip.so"
echo "[build] $OUT/libslu_hip.so"
# the decoder's SLU_REQUIRE / SLU_FAIL (slu_common.h) call slu::set_error, a C++ symbol that libslu_hip.so exports and
# slu_hip.h does not declare (slu_last_error reads what it wrote): it links against the library beside it
"$HIPCC" --offload-arch=gfx950 -shared -fPIC "${DECODE_OBJS[@]}" -L"$OUT" -lslu_hip -Wl,-rpath,'$ORIGIN' -o "$OUT/libslu_decode.so"
echo "[build] $OUT/libslu_decode.so"
# the closed-set decoder of the fixed-slot head: the same one undefined project symbol, the same link
"$HIPCC" --offload-arch=gfx950 -shared -fPIC "${INTENTS_OBJS[@]}" -L"$OUT" -lslu_hip -Wl,-rpath,'$ORIGIN' -o "$OUT/libslu_intents.so"
echo "[build] $OUT/libslu_intents.so"
# the sample-rate converter: the same one undefined project symbol, the same link
"$HIPCC" --offload-arch=gfx950 -shared -fPIC "${RESAMPLE_OBJS[@]}" -L"$OUT" -lslu_hip -Wl,-rpath,'$ORIGIN' -o "$OUT/libslu_resample.so"
echo "[build] $OUT/libslu_resample.so"
# reverberation and noise banks: the same one undefined project symbol, the same link
"$HIPCC" --offload-arch=gfx950 -shared -fPIC "${ROOM_OBJS[@]}" -L"$OUT" -lslu_hip -Wl,-rpath,'$ORIGIN' -o "$OUT/libslu_room.so"
echo "[build] $OUT/libslu_room.so"
