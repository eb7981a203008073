#!/bin/bash
# usage: diag/build_dec_variant.sh NAME "-DFLAG ..."   -> diag/libflo_NAME.so with decode_kernels.hip rebuilt under the flags
set -e
name=$1; shift
src=flo_amd/csrc; bd=/tmp/w/bvd_$name; mkdir -p $bd
make -s -j16 -C $src
F="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-slp-vectorize -ffp-contract=off -Wno-unused-function -Iinclude $*"
/opt/rocm/bin/hipcc $F -c $src/decode_kernels.hip -o $bd/dk.o
objs=$(ls $src/build/*.o | grep -v /decode_kernels.o)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o diag/libflo_$name.so $bd/dk.o $objs -L/opt/rocm/lib -lrccl -lpthread
echo built diag/libflo_$name.so
