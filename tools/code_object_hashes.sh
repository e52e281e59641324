#!/bin/bash
# sha-256 (first 16 hex digits) and size of the gfx950 code object inside every kernel-bearing object
# of two builds, as a markdown table (profiles/r9_kernel_variants.md, r10_capi_split.md § Code objects):
#   tools/code_object_hashes.sh PARENT_BUILD_DIR THIS_BUILD_DIR
# The object's .hip_fatbin section is an offload bundle; its hipv4-amdgcn-amd-amdhsa--gfx950 entry is the ELF.
set -e
LLVM=${LLVM:-/opt/rocm/llvm/bin}
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
co() {  # object -> "hash bytes"
  "$LLVM/llvm-objcopy" -O binary --only-section=.hip_fatbin "$1" "$TMP/fatbin"
  "$LLVM/clang-offload-bundler" --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 \
    --input="$TMP/fatbin" --output="$TMP/co"
  echo "$(sha256sum "$TMP/co" | cut -c1-16) $(stat -c%s "$TMP/co")"
}
echo "| object | parent | this | bytes parent / this |"
echo "|---|---|---|---|"
for u in wos_kernel wos_channels wos_channels_rb wos_robust wos_bvc wos_tape wos_tape_index wos_query wos_siren wos_siren_vjp wos_siren_fit wos_siren_train wos_selftest; do
  read -r hp bp <<<"$(co "$1/$u.o")"
  read -r ht bt <<<"$(co "$2/$u.o")"
  echo "| build/$u.o | $hp | $ht | $bp / $bt |"
done
