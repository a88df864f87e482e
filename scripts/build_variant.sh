#!/bin/bash
# build an A/B variant of libbhgeo.so: scripts/build_variant.sh <name> [extra hipcc flags]
# (the units and their flags are the Makefile's; the variant's objects go to a directory of their own)
set -e
name=$1; shift
cd "$(dirname "$0")/.."
mkdir -p build/variants
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
make -C blackhole_geodesic_calculator_amd/csrc -j8 O="$T" OUT="$PWD/build/variants/libbhgeo_$name.so" EXTRA="$*"
