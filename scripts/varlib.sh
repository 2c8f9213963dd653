#!/bin/bash
# measurement-only library variants: varlib/NAME/libgm.so = the SCALED kernel units (gm_scaled.hip, gm_band.hip
# with gm_band_fast.hip, gm_draw.hip with gm_pick.hip) built with the given -D flags into build_var/NAME/,
# linked with every other object of the in-tree build (run `make` first). usage: varlib.sh NAME -DFLAG...
set -e
cd "$(dirname "$0")/.."
V=$1; shift
mkdir -p build_var/$V varlib/$V
B=distributed-membership_amd/build
UNITS="gm_scaled gm_band gm_draw"
for u in $UNITS; do
  rm -f build_var/$V/$u.o
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Iinclude -Idistributed-membership_amd/csrc "$@" \
    -c -o build_var/$V/$u.o distributed-membership_amd/csrc/$u.hip &
done
wait
for u in $UNITS; do test -s build_var/$V/$u.o; done
/opt/rocm/bin/hipcc -O3 -fPIC --offload-arch=gfx950 -shared -o varlib/$V/libgm.so \
  $(for u in $UNITS; do echo build_var/$V/$u.o; done) \
  $(ls $B/*.o | grep -v -E "/($(echo $UNITS | tr ' ' '|'))\.o$") -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib
