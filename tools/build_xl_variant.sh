#!/bin/bash
# Variant of libsais_hip.so in which only gemm_tn_xl.hip is rebuilt with extra flags (the other objects are the main build's):
#   tools/build_xl_variant.sh abl1 -DSAIS_XL_ABL=1   ->  tools/bin/abl1/libsais_hip.so   (A/B through SAIS_HIP_LIB)
name=$1; shift
exec "$(dirname "$0")/build_variant_file.sh" "$name" gemm_tn_xl "$@"
