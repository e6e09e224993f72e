#!/bin/bash
# Build an A/B variant of the library with extra device-compile flags: tools/build_variant.sh NAME "-DTRACE_WAVES=8 ..."
# -> pathtrace-on-cuda_amd/build_NAME/libptamd_NAME.so  (use with PTAMD_LIB=...).  Only the .hip objects are rebuilt.
set -e
NAME=$1; EXTRA=$2
PKG=$(dirname $(dirname $(readlink -f $0)))/pathtrace-on-cuda_amd
OD=$PKG/build/var_$NAME
mkdir -p $OD
FP="-ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt ${NOSLP--fno-slp-vectorize}"      # NOSLP= (empty) in the environment builds the variant with the SLP vectoriser on
for f in pt_kernels pt_wavefront pt_api pt_scene pt_probe pt_comm pt_denoise pt_stats pt_region pt_dynamic pt_rebuild pt_material pt_query pt_rays pt_aov pt_nearest pt_knearest pt_rayhits pt_lists pt_box pt_convex pt_sweep pt_tri; do
  # only pt_wavefront depends on the variant flags; reuse the others
  if [ $f = pt_wavefront ] || [ ! -f $OD/$f.o ]; then
    if [ $f = pt_wavefront ]; then /opt/rocm/bin/hipcc --offload-arch=gfx950 -std=c++17 -O3 -fPIC -fvisibility=hidden $FP $EXTRA -c $PKG/csrc/$f.hip -o $OD/$f.o;
    else cp $PKG/build/$f.o $OD/$f.o; fi
  fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $PKG/build/libptamd_$NAME.so $PKG/build/pt_host.o $PKG/build/bvh_build.o $PKG/build/scenes.o $PKG/build/obj_loader.o $PKG/build/accel_build.o $OD/pt_kernels.o $OD/pt_wavefront.o $OD/pt_api.o $OD/pt_scene.o $OD/pt_probe.o $OD/pt_comm.o $OD/pt_denoise.o $OD/pt_stats.o $OD/pt_region.o $OD/pt_dynamic.o $OD/pt_rebuild.o $OD/pt_material.o $OD/pt_query.o $OD/pt_rays.o $OD/pt_aov.o $OD/pt_nearest.o $OD/pt_knearest.o $OD/pt_rayhits.o $OD/pt_lists.o $OD/pt_box.o $OD/pt_convex.o $OD/pt_sweep.o $OD/pt_tri.o -ldl
echo built $PKG/build/libptamd_$NAME.so
