#!/bin/bash
# diag/build_base.sh [rev]  -> diag/libflo_base.so: the library of a committed revision (default HEAD), built from that
# revision's own sources and Makefile, next to the working tree's library, for same-box A/B runs (diag/ab10k.sh base full).
set -e
rev=${1:-HEAD}
d=/tmp/w/base_src; rm -rf $d; mkdir -p $d
git archive $rev flo_amd/csrc include | tar -x -C $d
make -s -j16 -C $d/flo_amd/csrc
cp $d/flo_amd/libflo_hip.so diag/libflo_base.so
echo built diag/libflo_base.so from $rev
