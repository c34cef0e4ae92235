#!/bin/bash
# compare_device_asm.sh TREE_A TREE_B [WORKDIR]: is the device code of two checkouts the same?
# Compiles every .hip file of walnuts_amd/csrc in both trees to gfx950 assembly with the Makefile's CODEGEN_FLAGS and
# compares it, leaving out what differs whenever a header's text does: the per-translation-unit __hip_cuid_<hash> symbol
# and the .file / .ident lines.  Exit status 0: identical.  JOBS (default 8) compilations run side by side.
set -u
A=$(realpath "$1") B=$(realpath "$2") W=${3:-$(mktemp -d)}
for T in "$A" "$B"; do
  [ "$T" = "$A" ] && O="$W/a" || O="$W/b"
  mkdir -p "$O"
  FLAGS=$(make -s -C "$T/walnuts_amd/csrc" -pn 2>/dev/null | sed -n 's/^CODEGEN_FLAGS := //p' | head -1)
  (cd "$T/walnuts_amd/csrc" && ls *.hip | xargs -P "${JOBS:-8}" -I{} \
    hipcc $FLAGS -I. "-DWN_CODEGEN_FLAGS=\"\"" "-DWN_COMPILER_VERSION=\"\"" --cuda-device-only -S {} -o "$O/{}.s") || exit 2
done
rc=0
for f in "$W"/a/*.s; do
  n=$(basename "$f")
  if diff -q <(grep -v -e __hip_cuid_ -e '^\s*\.file' -e '^\s*\.ident' "$f") \
             <(grep -v -e __hip_cuid_ -e '^\s*\.file' -e '^\s*\.ident' "$W/b/$n") > /dev/null; then
    echo "same    $n ($(grep -c '^\s*\.amdhsa_kernel ' "$f") kernels, $(wc -l < "$f") lines)"
  else
    echo "DIFFERS $n"
    rc=1
  fi
done
exit $rc
