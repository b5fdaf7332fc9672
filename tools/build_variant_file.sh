#!/bin/bash
# Variant of libsais_hip.so in which ONE source is rebuilt with extra flags (the other objects are the main build's):
#   tools/build_variant_file.sh <name> <source stem> [flags...]   ->  tools/bin/<name>/libsais_hip.so  (SAIS_HIP_LIB=...)
# Per-file flags come from the Makefile.
set -e
name=$1; stem=$2; shift 2
root=$(cd "$(dirname "$0")/.." && pwd)
out=$root/tools/bin/$name
mkdir -p $out
make -s -C $root/sais_amd/csrc -j8 >/dev/null
cp $root/sais_amd/csrc/*.o $out/
rm -f $out/$stem.o
make -s -C $root/sais_amd/csrc OBJDIR=$out LIB=$out/libsais_hip.so VARIANT_$stem="$*"
rm -f $out/*.o
echo built $out/libsais_hip.so
