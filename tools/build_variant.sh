#!/bin/bash
# build_variant.sh NAME [-DX=Y ...]: A/B builds of the kernels with different defines -> .ab/lib_NAME.so
# (every other object is the tree's own, brought up to date first; the list is the Makefile's)
set -e
name=$1; shift
cd "$(dirname "$0")/../dpgo_amd/csrc"
mkdir -p ../../.ab
others=$(make -s print-OBJS | tr ' ' '\n' | grep -vx kernels.o)
make -s $others
hipcc --offload-arch=gfx950 -std=c++17 -O3 -fPIC -fopenmp -Wno-unused-function "$@" -c kernels.hip -o /tmp/kernels_$name.o
hipcc --offload-arch=gfx950 -shared -fopenmp -o ../../.ab/lib_$name.so $others /tmp/kernels_$name.o -ldl
