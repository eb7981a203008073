#!/bin/bash
# usage: diag/build_variant.sh NAME "-DFLAG ..."   -> diag/libflo_NAME.so   (run from the repo root)
# lossy_kernels.hip and batch.cpp (the host side of the diagnostic switches) rebuilt under the flags, every other object
# from the working tree's build
set -e
name=$1; shift
src=flo_amd/csrc; bd=/tmp/w/bv_$name; mkdir -p $bd
make -s -j16 -C $src
F="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-slp-vectorize -ffp-contract=off -Wno-unused-function -Iinclude $*"
rm -f $bd/lk.o $bd/api.o
/opt/rocm/bin/hipcc $F -c $src/lossy_kernels.hip -o $bd/lk.o &
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O2 -std=c++17 -fPIC -w $* -c $src/batch.cpp -o $bd/api.o &
wait
test -f $bd/lk.o && test -f $bd/api.o
objs=$(ls $src/build/*.o | grep -v -e /lossy_kernels.o -e /batch.o)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o diag/libflo_$name.so $bd/lk.o $bd/api.o $objs -L/opt/rocm/lib -lrccl -lpthread
echo built diag/libflo_$name.so
