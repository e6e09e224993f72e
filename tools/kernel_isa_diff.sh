#!/bin/bash
# Are the instruction streams of the kernels of two builds of one object file the same?  Compile only, no GPU needed:
#   tools/kernel_isa_diff.sh OLD.o NEW.o [regex over demangled kernel names, default: every kernel] [sed -E script]
# Takes the gfx950 code object out of each host object (.hip_fatbin section -> clang-offload-bundler), disassembles it and compares,
# kernel by kernel, the instructions with addresses and comments stripped.  Prints one line per kernel and exits 1 if any differs.
# The sed -E script, if given, renames kernels: it is applied to the demangled names of the OLD side (its whole disassembly: a name also
# appears in branch targets) before matching, so a renamed kernel is compared with its parent instead of being reported as "only in".
set -e
old=$1; new=$2; pat=${3:-.}; rename=${4:-}
LLVM=${ROCM_PATH:-/opt/rocm}/llvm/bin
tmp=$(mktemp -d); trap 'rm -rf "$tmp"' EXIT
for side in old new; do
    obj=$old; [ $side = new ] && obj=$new
    objcopy -O binary --only-section=.hip_fatbin "$obj" $tmp/$side.fb
    $LLVM/clang-offload-bundler --type=o --unbundle --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=$tmp/$side.fb --output=$tmp/$side.co
    $LLVM/llvm-objdump -d --no-show-raw-insn --no-leading-addr $tmp/$side.co | c++filt > $tmp/$side.s
done
[ -z "$rename" ] || sed -E -i "$rename" $tmp/old.s
python3 - $tmp/old.s $tmp/new.s "$pat" <<'PY'
import re, sys


def kernels(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r'^(?:[0-9a-f]+ )?<(.+)>:\s*$', line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        text = re.sub(r'//.*', '', line).strip()
        if cur is not None and text and text != '...':      # '...': objdump's mark for the zero padding between two kernels
            cur.append(text)
    return out


old, new, pat = kernels(sys.argv[1]), kernels(sys.argv[2]), re.compile(sys.argv[3])
bad = 0
for name in sorted(set(old) | set(new)):
    if not pat.search(name):
        continue
    short = name.split('(')[0]
    if name not in old or name not in new:
        print(f"{'only in ' + ('NEW' if name in new else 'OLD'):<10} {len((new if name in new else old)[name]):6d}  {short}")
    elif old[name] == new[name]:
        print(f"{'identical':<10} {len(old[name]):6d}  {short}")
    else:
        bad += 1
        print(f"{'DIFFERENT':<10} {len(old[name]):6d} -> {len(new[name])}  {short}")
sys.exit(1 if bad else 0)
PY
