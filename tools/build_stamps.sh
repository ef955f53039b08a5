#!/bin/bash
# Variant of the library whose selection kernels write phase stamps (tools/select_stamps.py).  Needs the objects of a normal build.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
P=$ROOT/embodied_object_detection_amd
mkdir -p $ROOT/tools/ablate
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -Wno-unused-function -ffp-contract=on -DEOD_STAMPS -c $P/csrc/select.hip -o $ROOT/tools/ablate/select_stamps.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $ROOT/tools/ablate/libeod_stamps.so $(ls $P/build/*.o | grep -v "select.o\|conv_glds\|conv_halo") $ROOT/tools/ablate/select_stamps.o
ls -la $ROOT/tools/ablate/libeod_stamps.so
