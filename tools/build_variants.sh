#!/bin/bash
# A/B libraries of the specialised kernel's geometry for tools/ab_bench.py (tools/prebuilt/, git-ignored; built libraries travel to the GPU box with the tree):
#   tools/build_variants.sh name:"-DVPT_FAST_CC=1024 -DVPT_FAST_WG=7" ...
# and of the cache policy of a class of its accesses (kernels_fast.hip, kPol*: 0 plain, 1 non-temporal, 2 agent scope):
#   tools/build_variants.sh nt_text:"-DVPT_POL_TEXT=1" sc1_out:"-DVPT_POL_SCORE=2 -DVPT_POL_LABEL=2" ...
# (the text's policy is the launch's choice unless a variant fixes it: -DVPT_POL_TEXT=0 plain, =1 non-temporal)
# A variant whose definitions are all VPT_POL_* differs in kernels_fast.hip only: the other sources (vaporetto_amd/build.py, SOURCES) are compiled
# once and shared by those.  Any other definition may reach every source (VPT_FAST_CAP is the host's too): such a variant is compiled whole.
set -e
cd "$(dirname "$0")/.."
mkdir -p tools/prebuilt/obj
SRC=$(python -c "from vaporetto_amd import build; print(' '.join(build.SOURCES))")
CC="/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function"
cd vaporetto_amd/csrc
OBJ=../../tools/prebuilt/obj
N=0
for F in $SRC; do
  [ "$F" = kernels_fast.hip ] && continue
  $CC -c "$F" -o "$OBJ/${F%.*}.o" &
  N=$((N + 1)); [ $((N % 8)) -eq 0 ] && wait
done
pol_only() { for D in $1; do case "$D" in -DVPT_POL_*) ;; *) return 1 ;; esac; done; return 0; }
for V in "$@"; do
  NAME="${V%%:*}"; DEFS="${V#*:}"
  pol_only "$DEFS" || { $CC -shared $DEFS -o ../../tools/prebuilt/libvaporetto_$NAME.so $SRC & continue; }
  $CC $DEFS -c kernels_fast.hip -o "$OBJ/kernels_fast_$NAME.o" &
  N=$((N + 1)); [ $((N % 8)) -eq 0 ] && wait
done
wait
SHARED=$(for F in $SRC; do [ "$F" = kernels_fast.hip ] || echo "$OBJ/${F%.*}.o"; done)
for V in "$@"; do
  NAME="${V%%:*}"; DEFS="${V#*:}"
  pol_only "$DEFS" || continue
  $CC -shared -o ../../tools/prebuilt/libvaporetto_$NAME.so $SHARED "$OBJ/kernels_fast_$NAME.o"
done
ls -la ../../tools/prebuilt/
