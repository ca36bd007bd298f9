#!/bin/sh
# The HOST translation units (scene validation + flattening, the BVH builders, tile dealing + the host merge) with AddressSanitizer + UBSan, linked with the normal device
# objects: nano-kazen_amd/csrc/variants/host_asan/libkazen_mi355x.so. GPU sanitizers do not exist on this pool; this covers the code that runs on the CPU.
#   sh scripts/dev/build_host_asan.sh && sh scripts/dev/run_host_asan.sh
set -e
cd "$(dirname "$0")/../../nano-kazen_amd/csrc"
OUT=variants/host_asan; mkdir -p $OUT
FLAGS="-O1 -g -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function"
DEV="--offload-arch=gfx950 -fgpu-flush-denormals-to-zero -fno-slp-vectorize"
DEVICE_UNITS="kz_render kz_replica kz_film kz_debug"; IEEE_UNITS="kz_refit"; HOST_UNITS="kz_multi kz_host kz_bvh kz_arena kz_plan kz_edit"      # (build.sh's lists)
for u in $DEVICE_UNITS $IEEE_UNITS $HOST_UNITS; do rm -f $OUT/$u.o; done
PIDS=""
for u in $DEVICE_UNITS; do hipcc -O3 -std=c++17 -fPIC -ffp-contract=off $DEV -c $u.hip -o $OUT/$u.o & PIDS="$PIDS $!"; done
for u in $IEEE_UNITS; do hipcc -O3 -std=c++17 -fPIC -ffp-contract=off --offload-arch=gfx950 -fno-slp-vectorize -c $u.hip -o $OUT/$u.o & PIDS="$PIDS $!"; done
for u in $HOST_UNITS; do hipcc $FLAGS -fsanitize=address,undefined -fno-omit-frame-pointer -c $u.cpp -o $OUT/$u.o & PIDS="$PIDS $!"; done
for p in $PIDS; do wait $p || { echo "build failed: a translation unit did not compile"; exit 1; }; done
hipcc -shared -fPIC -fsanitize=address,undefined -shared-libsan -o $OUT/libkazen_mi355x.so $(for u in $DEVICE_UNITS $IEEE_UNITS $HOST_UNITS; do echo $OUT/$u.o; done) -pthread
rm -f $OUT/*.o
echo "built $(pwd)/$OUT/libkazen_mi355x.so"
