#!/bin/bash
# Builds a variant of the engine library for A/B timing or diagnostics (never shipped):
#   tools/build_variant.sh NAME "-DWOS_DIAG=1 ..."   ->  neural-monte-carlo-fluid-simulation_amd/lib/var/libwos_NAME.so
# Select it at run time with WOS_LIB_PATH (tools/time_variants.py does).
# The unit list is the Makefile's: a variant is `make` with other defines, objects and output.
set -e
cd "$(dirname "$0")/../neural-monte-carlo-fluid-simulation_amd"
NAME=$1; DEFS=$2
SRC=${WOS_VARIANT_SRC:-csrc}  # an experimental copy of the sources (the shipped csrc/ stays untouched)
make -s -j"${MAX_JOBS:-16}" DEFS="-w $DEFS" SRC="$SRC" BUILD="build/var/$NAME" OUT="lib/var/libwos_$NAME.so" >&2
echo lib/var/libwos_$NAME.so
