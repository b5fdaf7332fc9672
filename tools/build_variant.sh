#!/bin/bash
# Build a variant of libsais_hip.so with extra compiler flags into tools/bin/<name>/ (git-ignored; travels with gpurun),
# for A/B runs inside the training step:  SAIS_HIP_LIB=tools/bin/<name>/libsais_hip.so python bench.py ...
#   tools/build_variant.sh clk -DSAIS_CLK_STAMP
# Per-file flags come from the Makefile; the extra ones go to every source.
set -e
name=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
out=$root/tools/bin/$name
mkdir -p $out
make -s -C $root/sais_amd/csrc -j8 OBJDIR=$out LIB=$out/libsais_hip.so VARIANT="$*"
rm -f $out/*.o
echo built $out/libsais_hip.so
