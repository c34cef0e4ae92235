#!/bin/bash
# compare_device_asm.sh TREE_A TREE_B [WORKDIR]: is the device code of two checkouts the same?
# Compiles every .hip file of walnuts_amd/csrc in both trees to gfx950 assembly with the Makefile's CODEGEN_FLAGS and
# compares it, leaving out what differs whenever a header's text does: the per-translation-unit __hip_cuid_<hash> symbol
# and the .file / .ident lines.  Files that only one tree has, and wn_engine.hip if it differs, are then compared symbol
# by symbol across files (code that moved from one translation unit to another; only the text of each function and
# object is compared there, not the kernel-argument metadata or other section-level text).  Exit status 0: identical.  JOBS (default 8)
# compilations run side by side.
set -u
A=$(realpath "$1") B=$(realpath "$2") W=${3:-$(mktemp -d)}
for T in "$A" "$B"; do
  [ "$T" = "$A" ] && O="$W/a" || O="$W/b"
  mkdir -p "$O"
  FLAGS=$(make -s -C "$T/walnuts_amd/csrc" -pn 2>/dev/null | sed -n 's/^CODEGEN_FLAGS := //p' | head -1)
  (cd "$T/walnuts_amd/csrc" && ls *.hip | xargs -P "${JOBS:-8}" -I{} \
    hipcc $FLAGS -I. "-DWN_CODEGEN_FLAGS=\"\"" "-DWN_COMPILER_VERSION=\"\"" --cuda-device-only -S {} -o "$O/{}.s") || exit 2
done
unmarked() { grep -v -e __hip_cuid_ -e '^\s*\.file' -e '^\s*\.ident' "$1"; }
rc=0
moved=()   # files that only one tree has, and wn_engine.hip if it differs: their symbols are compared one by one below
for n in $(cd "$W" && ls a b | grep '\.s$' | sort -u); do
  f="$W/a/$n"
  if [ ! -f "$f" ] || [ ! -f "$W/b/$n" ]; then
    moved+=("$n")
  elif diff -q <(unmarked "$f") <(unmarked "$W/b/$n") > /dev/null; then
    echo "same    $n ($(grep -c '^\s*\.amdhsa_kernel ' "$f") kernels, $(wc -l < "$f") lines)"
  elif [ "$n" = wn_engine.hip.s ]; then
    moved+=("$n")   # (the unit the engine's other units were split from)
  else
    echo "DIFFERS $n"
    rc=1
  fi
done
[ ${#moved[@]} -eq 0 ] && exit $rc
# Code that moved between files: every function and object of those files (from its .type line to its .size line, the
# kernel descriptor included), matched by NAME across each tree's files.  Labels carry the function's number within
# its file (.LBB3_7, .Lfunc_end3), in the code and in the compiler's comments: the number and the comments are taken
# out.  A symbol that several files of a tree define (a static table)
# must have the same set of bodies in both trees.
echo "by symbol over: ${moved[*]}"
python3 - "$W" "${moved[@]}" <<'PY' || rc=1
import os, re, sys
W, names = sys.argv[1], sys.argv[2:]
SKIP = re.compile(r"__hip_cuid_|^\s*\.file|^\s*\.ident")
START = re.compile(r"\s*\.type\s+([^,\s]+),@(function|object)")
LABEL = re.compile(r"\.L(BB|func_begin|func_end|tmp|JTI|CPI)\d+")
def symbols(tree):
    out = {}
    for n in names:
        path = os.path.join(W, tree, n)
        if not os.path.exists(path):
            continue
        name, body = None, []
        for line in open(path):
            if SKIP.search(line):
                continue
            if name is None:
                m = START.match(line)
                if m:
                    name, body = m.group(1), [line]
                continue
            line = LABEL.sub(r".L\1", line.split(";")[0]).rstrip()   # (comments name basic blocks by number too)
            if line:
                body.append(line + "\n")
            if re.match(r"\s*\.size\s+" + re.escape(name) + ",", line):
                out.setdefault(name, set()).add("".join(body))
                name = None
    return out
a, b = symbols("a"), symbols("b")
kernel = lambda bodies: any(".amdhsa_kernel " in t for t in bodies)
bad = 0
for name in sorted(set(a) | set(b)):
    if name not in a or name not in b:
        print("ONLY IN %s %s" % ("A" if name in a else "B", name))
        bad += 1
    elif a[name] != b[name]:
        print("DIFFERS %s" % name)
        bad += 1
    else:
        print("same    %s%s" % (name, " (kernel)" if kernel(a[name]) else ""))
ka, kb = sum(map(kernel, a.values())), sum(map(kernel, b.values()))
print("%d symbols, kernels: %d in A, %d in B, %s" % (len(set(a) | set(b)), ka, kb, "all same" if bad == 0 else "%d NOT the same" % bad))
sys.exit(1 if bad else 0)
PY
exit $rc
