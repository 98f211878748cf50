#!/bin/bash
# tools/isa_diff.sh <obj-dir-a> <obj-dir-b>
#
# Are the kernels of two builds the same machine code?  Unbundles the gfx950 code object of every *.o in both directories (as
# check_spills.sh does) and compares, per kernel symbol, the disassembly (without the trailing "// address: encoding"
# comments and the zero padding between kernels, so a kernel that only moved inside its code object is the same) and its
# llvm-readelf --notes metadata block.
# Prints the symbols that differ or exist on one side only; exit 1 if there are any.
set -e -o pipefail
LLVM=${LLVM_BIN:-/opt/rocm/lib/llvm/bin}
T=$(mktemp -d); trap 'rm -rf $T' EXIT
dump() {   # <obj-dir> <out>: one line per instruction / metadata line, "<object>:<symbol><TAB>text", grouped by symbol
  for o in $1/*.o; do
    b=$(basename $o .o)
    $LLVM/llvm-objcopy -O binary --only-section=.hip_fatbin $o $T/x.fat 2>/dev/null || continue
    [ -s $T/x.fat ] || continue
    tgt=$($LLVM/clang-offload-bundler --list --input=$T/x.fat --type=o | grep amdgcn | head -1 || true)
    [ -n "$tgt" ] || continue
    $LLVM/clang-offload-bundler --unbundle --input=$T/x.fat --type=o --targets=$tgt --output=$T/x.co
    $LLVM/llvm-objdump -d $T/x.co | sed -e 's|[ \t]*//.*$||' -e '/^[ \t]*\.\.\.$/d' | awk -v o=$b '
      /^[0-9a-f]+ <.*>:$/ {sym=$2; gsub(/[<>:]/, "", sym); next} sym != "" && NF {print o ":" sym "\tisa " $0}'
    $LLVM/llvm-readelf --notes $T/x.co | awk -v o=$b '
      function flush(i) {for (i = 0; i < n; ++i) print o ":" name "\tmeta " buf[i]; n = 0}
      /^amdhsa\./ {flush(); on = /^amdhsa\.kernels:/; next} /^  - / {flush()} on {buf[n++] = $0} on && /^    \.name:/ {name=$NF} END {flush()}'
  done | sort -s -t"$(printf '\t')" -k1,1 > $2
}
dump $1 $T/a.txt
dump $2 $T/b.txt
kernels=$(grep -c "$(printf '\tmeta     \\.name:')" $T/a.txt || true)
differ=$(diff $T/a.txt $T/b.txt | grep '^[<>]' | cut -f1 | cut -c3- | sort -u || true)
if [ -n "$differ" ]; then
  echo "isa_diff: these symbols differ between $1 and $2 (object:symbol):"; echo "$differ" | sed 's/^/  /'
  exit 1
fi
echo "isa_diff: $kernels kernels in $(cut -d: -f1 $T/a.txt | sort -u | wc -l) objects, disassembly and metadata identical"
