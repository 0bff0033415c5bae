#!/bin/bash
# scripts/compare_code_objects.sh <objdir A> <objdir B>: are the gfx950 code objects of two builds the
# same device code?  For every *.o of A (unbundled as in scripts/kernel_resources.sh) the sections
# .text, .rodata, .note (kernel metadata: VGPR, SGPR, LDS, scratch) byte for byte and .dynsym symbol
# for symbol are compared with those of the object of the same name in B.  One line per unit; exit status 1 on any difference.
#   make -C climatemachine.jl_amd/csrc OBJDIR=/tmp/a OUT=/tmp/a/libcmdg.so      (in each tree)
#   scripts/compare_code_objects.sh /tmp/a /tmp/b
# A plug-in object (plugins.build keeps none: compile its generated .hip with -c) compares the same way.
set -u
A=$(readlink -f "$1")
B=$(readlink -f "$2")
LLVM=/opt/rocm/lib/llvm/bin
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
sections() {  # <object> <out dir>: one file per section of its gfx950 code object
    mkdir -p "$2"
    objcopy -O binary --only-section=.hip_fatbin "$1" "$2/fat.bin" || return 1
    [ -s "$2/fat.bin" ] || return 0  # (no device code in this unit)
    $LLVM/clang-offload-bundler --type=o --input="$2/fat.bin" --unbundle \
        --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output="$2/dev.co" || return 1
    for s in text rodata note; do  # (a section the code object lacks leaves no file)
        $LLVM/llvm-readelf -S "$2/dev.co" | grep -q " \.$s " || continue
        $LLVM/llvm-objcopy --dump-section .$s="$2/$s" "$2/dev.co" "$2/stripped.co" || return 1
    done
    # .dynsym decoded: value, size, type, binding, visibility, section and name of every symbol, in
    # name order.  The table holds one symbol that is no code, __hip_cuid_<hash of the source path
    # and the command line>, whose place in the table moves the others: its hash is masked.
    $LLVM/llvm-readelf --dyn-syms -W "$2/dev.co" | awk '$1 ~ /^[0-9]+:$/ { $1 = ""; print }' |
        sed -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid_*/' | sort -k7 > "$2/dynsym"
}
status=0
for a in "$A"/*.o; do
    unit=$(basename "$a" .o)
    b="$B/$unit.o"
    if [ ! -f "$b" ]; then
        echo "$unit: MISSING in $B"
        status=1
        continue
    fi
    rm -rf "$tmp/a" "$tmp/b"
    sections "$a" "$tmp/a" && sections "$b" "$tmp/b" || { echo "$unit: cannot unbundle"; status=1; continue; }
    diffs=""
    for s in text rodata note dynsym; do
        [ -e "$tmp/a/$s" ] || [ -e "$tmp/b/$s" ] || continue
        cmp -s "$tmp/a/$s" "$tmp/b/$s" || diffs="$diffs .$s"
    done
    size=$(stat -c %s "$tmp/a/text" 2>/dev/null || echo 0)
    if [ -z "$diffs" ]; then
        echo "$unit: identical (.text $size bytes)"
    else
        echo "$unit: DIFFERS in$diffs"
        status=1
    fi
done
exit $status
