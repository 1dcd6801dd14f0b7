#!/bin/bash
# A variant of libfmx.so that differs in the literal search's units only (fmx_search.hip and fmx_search4_*.hip; the
# product's other objects are linked as they are -- OBJDIR=<dir>: another build's objects, which an older commit's units need
# when a struct they share with the rest has changed since):
#   tools/build_search_variant.sh <tag> [flags, e.g. -DFMX_SEARCH_WAVES=5]   ->  findex_amd/lib/variants/libfmx_<tag>.so
# SRCDIR=<dir>: other versions of those units and of their headers (all of csrc/*.h), e.g. an older commit's csrc
# (python -m findex_amd.build first: the product's objects must be current)
TAG=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
SRC=${SRCDIR:-$ROOT/findex_amd/csrc}
OUT=$ROOT/findex_amd/lib/variants; mkdir -p $OUT/search_$TAG
pids=()
for f in fmx_search.hip fmx_search4_onehot.hip fmx_search4_onehot_wide.hip fmx_search4_bytes.hip fmx_search4_onehot_kx.hip; do
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -I$ROOT/include -I$SRC "$@" -x hip -c $SRC/$f -o $OUT/search_$TAG/$f.o & pids+=($!)
done
for p in "${pids[@]}"; do wait $p || exit 1; done
objs=$(ls ${OBJDIR:-$ROOT/findex_amd/lib}/*.o | grep -v "fmx_search.hip.o\|fmx_search4_\|faults.o")
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o $OUT/libfmx_$TAG.so $objs $OUT/search_$TAG/*.o -ldl && rm -rf $OUT/search_$TAG && echo $OUT/libfmx_$TAG.so
