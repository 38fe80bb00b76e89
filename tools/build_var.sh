#!/bin/bash
# Build a library variant for tools/ab.sh: one unit of csrc recompiled (from an
# edited copy, or with extra flags such as -DMR_OP_PROF=1), linked with the
# product objects of build/obj.  The unit list and each unit's flags come from
# csrc/Makefile (its print-* targets).
# Usage: bash tools/build_var.sh NAME [hipcc flags...]   (after `make` in csrc)
# UNIT=serving (or any unit of csrc/Makefile; default kernels) is the rebuilt unit;
# SRC=path builds that file as the rebuilt unit (an edited copy, or a
# `git show REV:...` one);
# UNITS="kernels engine" recompiles several units with the same flags (needed
# when a flag changes a header both units use)
set -e
NAME=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
CSRC=$ROOT/movie_recommender_amd/csrc
OUT=$ROOT/var_libs/$NAME
mkdir -p "$OUT"
OBJ=$ROOT/build/obj
UNITS=${UNITS:-${UNIT:-kernels}}
OBJS=""
for U in $UNITS; do
  SRCU=$CSRC/$U.hip
  [ -n "$SRC" ] && SRCU=$SRC   # SRC: the source of the (single) rebuilt unit
  /opt/rocm/bin/hipcc $(make -s -C "$CSRC" print-flags-$U) "$@" -I"$CSRC" -c "$SRCU" -o "$OUT/$U.o"
  OBJS="$OBJS $OUT/$U.o"
done
for V in $(make -s -C "$CSRC" print-units); do
  case " $UNITS " in *" $V "*) ;; *) OBJS="$OBJS $OBJ/$V.o" ;; esac
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $OBJS -o "$OUT/cpp_ls_lib.so" \
  -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib -Wl,-z,defs
echo "$OUT/cpp_ls_lib.so"
