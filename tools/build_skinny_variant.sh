#!/bin/bash
# libswc_<tag>.so with other parameters of the skinny swc_gemm kernel (csrc/swc_gemm_skinny.hip), beside the product build:
#   tools/build_skinny_variant.sh <tag> <waves 4|8> <ring depth> <workgroups per CU> [extra flags for the skinny file, e.g. -DSWC_SKINNY_WREG=1]
# swc_gemm.hip is compiled with the same parameters (its plan reports them); every other object is the product build's.  Select the
# result with SWC_LIB=<path>; the product library libswc_hip.so is never overwritten.
set -e
cd "$(dirname "$0")/../simwhisper_codec_amd"
tag=$1; nw=$2; d=$3; wg=$4; shift 4
F="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=on -DSWC_SKINNY_WAVES=$nw -DSWC_SKINNY_DEPTH=$d -DSWC_SKINNY_WG_PER_CU=$wg -I ../include -I csrc"
/opt/rocm/bin/hipcc $F -mllvm -amdgpu-sched-strategy=max-ilp -c csrc/swc_gemm.hip -o /tmp/gemm_$tag.o &
/opt/rocm/bin/hipcc $F "$@" -c csrc/swc_gemm_skinny.hip -o /tmp/skinny_$tag.o &
wait
objs=""
for o in build/*.o; do case $o in build/swc_gemm.o|build/swc_gemm_skinny.o|build/flac_check*) ;; *) objs="$objs $o";; esac; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o libswc_$tag.so $objs /tmp/gemm_$tag.o /tmp/skinny_$tag.o
echo built libswc_$tag.so
