#!/bin/bash
# Builds tools/variants/lib_<name>.so: the library with one or more translation units rebuilt under extra flags (the timing-stamp
# and phase-timing builds of the probes, flag experiments), to be loaded through EDGL_LIB_PATH.  Every unit gets the flags of
# easydgl_amd/build.py (FLAGS + EXTRA_FLAGS[unit]) plus the extra ones; the other objects come from easydgl_amd/csrc/obj, so build
# the library first.
# usage: bash tools/build_variant.sh <name> "<extra flags>" <unit without .hip> ...
#   bash tools/build_variant.sh timing -DSTRIP_TIMING k_score_strip              (tools/strip_probe.py)
#   bash tools/build_variant.sh phase_k_tail -DEDGL_PHASE_TIMING k_tail_fwd      (tools/phase_probe*.py; k_tail_bwd for the backward)
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
N=$1; X=$2; shift 2
OUT="$ROOT/tools/variants"
mkdir -p "$OUT"
cd "$ROOT/easydgl_amd/csrc"
ask() { python -c "import sys; sys.path.insert(0, '$ROOT/easydgl_amd'); import build; print($1)" "$2"; }
HIPCC=$(ask "build._hipcc()")
SKIP=""; NEW=""
for F in "$@"; do
  $HIPCC $(ask "' '.join(build.FLAGS + build.EXTRA_FLAGS.get(sys.argv[1], []))" "$F.hip") $X -c "$F.hip" -o "$OUT/${F}_$N.o" &
  SKIP="$SKIP -e obj/$F.o"; NEW="$NEW $OUT/${F}_$N.o"
done
wait
OBJS=$(ls obj/*.o | grep -v -x $SKIP)
$HIPCC --offload-arch=gfx950 -shared -fPIC -o "$OUT/lib_$N.so" $OBJS $NEW
echo "$OUT/lib_$N.so"
