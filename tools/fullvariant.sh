#!/bin/bash
# Build a whole-library A/B variant: every source recompiled with the product's own flags (csm_mlx/_build.py)
# plus extra ones (e.g. a profiling switch of a shared header): lab/libcsm_hip_<name>.so.
# usage: tools/fullvariant.sh <name> <flags...>   (VARIANT_DIR=<dir> writes there)
set -e
name=$1; shift
OUT=${VARIANT_DIR:-lab}
cd "$(dirname "$0")/.."
b=/tmp/fv_$name; mkdir -p $b $OUT
pids=""
for src in csm-mlx_amd/csrc/*.hip csm-mlx_amd/csrc/*.cpp; do
  f=$(basename $src)
  python csm-mlx_amd/csm_mlx/_build.py compile $f $b/$f.o "$@" & pids="$pids $!"
done
for p in $pids; do wait $p; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $OUT/libcsm_hip_$name.so $b/*.o
echo $OUT/libcsm_hip_$name.so
