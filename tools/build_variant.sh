#!/bin/bash
# A/B builds: tools/build_variant.sh <name> <unit>[,<unit2>...] <extra hipcc flags...>
# compiles the named unit(s) -- names as in __graft_entry__.hip_units(): a file such as siegel_dist_big.hip, or a kernel instance
# of csrc/siegel_bwd_instances.hpp such as siegel_bwd_half_upper_8_scatter -- with the extra flags and links them with the
# product's other objects into build_ab/<name>.so (the product library is not touched).  Timed against each other by tools/fwd_ab.py.
set -e
NAME=$1; UNITS=$2; shift 2
ROOT=$(cd "$(dirname "$0")/.." && pwd)
CSRC=$ROOT/sympa_amd/csrc
mkdir -p $ROOT/build_ab/$NAME
OBJS=""
SKIP=""
for U in ${UNITS//,/ }; do
  # the unit's defines and source file
  SRC=$(cd $ROOT && python3 -c "import sys, __graft_entry__ as g; print(*[w for n, s, d in g.hip_units() if n == sys.argv[1] for w in d + [s]])" $U)
  [ -n "$SRC" ] || { echo "no unit named $U (see __graft_entry__.hip_units())"; exit 1; }
  (cd $CSRC && hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC "$@" -c -o $ROOT/build_ab/$NAME/${U%.hip}.o $SRC) &
  SKIP="$SKIP ${U%.hip}.o"
done
wait
for O in $CSRC/*.o; do
  B=$(basename $O)
  if [[ " $SKIP " == *" $B "* ]]; then OBJS="$OBJS $ROOT/build_ab/$NAME/$B"; else OBJS="$OBJS $O"; fi
done
hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -o $ROOT/build_ab/$NAME.so $OBJS
echo built build_ab/$NAME.so
