#!/bin/bash
# Builds tools/exp/librt_<name>.so from the tree's sources with extra -D flags (for tools/exp_libs.sh A/B runs):
#   tools/build_variant.sh <name> [-DFLAG=value ...]          the PRODUCT's objects (one kernel, no test entry points)
#   DIAG=1 tools/build_variant.sh <name> [-DFLAG ...]         the diagnostic library's objects (the same rt_kernels object + the
#                                                             unit-test kernels, the wavefront pipeline, host units with -DRT_DIAG_VARIANTS)
# The flags go to rt_kernels.hip and the host units; every other object is the Makefile's own.  WHAT is linked is the Makefile's
# lists (make print-<LIST>): no second copy of them here.
name=$1; shift
cd "$(dirname "$0")/../raytracing_c_amd/csrc" || exit 1
list() { make -s print-$1; }
F="--offload-arch=gfx950 -O3 -ffp-contract=off -fno-slp-vectorize -fPIC -std=c++17 -Wno-unused-function ${RAFLAGS--mllvm -greedy-regclass-priority-trumps-globalness=1 -mllvm -amdgpu-prealloc-sgpr-spill-vgprs}"      # RAFLAGS= for the build without the Makefile's register-allocation flags
tmp=$(mktemp -d)
/opt/rocm/bin/hipcc $F "$@" -c rt_kernels.hip -o $tmp/rt_kernels.o || exit 1      # (the one kernel object, never with -DRT_DIAG_VARIANTS)
objs="$tmp/rt_kernels.o"
rest="$(list DEV_OBJS) $(list C_OBJS)"
for u in $(list KERNEL_UNITS); do [ $u = rt_kernels ] || rest="$rest $u.o"; done
[ -n "$DIAG" ] && F="$F -DRT_DIAG_VARIANTS"
[ -n "$DIAG" ] && for f in $(list DIAG_KERNEL_UNITS); do /opt/rocm/bin/hipcc $F "$@" -c $f.hip -o $tmp/$f.o || exit 1; objs="$objs $tmp/$f.o"; done
units=$(list API_UNITS); [ -n "$DIAG" ] && units=$(list API_DIAG_UNITS)
for f in $units; do /opt/rocm/bin/hipcc $F "$@" -c $f.cpp -o $tmp/$f.o || exit 1; objs="$objs $tmp/$f.o"; done
make -s $rest || exit 1
mkdir -p ../../tools/exp
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../../tools/exp/librt_$name.so $objs $rest -lpthread || exit 1
rm -rf $tmp; ls -la ../../tools/exp/librt_$name.so
