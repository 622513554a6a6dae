#!/bin/bash
# One file per kernel symbol of a HIP shared library's gfx950 code objects, addresses / encodings / label numbers normalised, so that two
# builds can be compared symbol by symbol:  tools/kernel_disasm.sh old/libgmesh_hip.so /tmp/a; tools/kernel_disasm.sh new/libgmesh_hip.so /tmp/b;
# for f in /tmp/a/k/*; do cmp -s $f /tmp/b/k/$(basename $f) || echo "differs: $(basename $f)"; done
set -e
in=$(readlink -f ${1:?library}); out=${2:?output directory}; mkdir -p $out; cd $out; rm -rf k co*.elf all.s fatbin.bin
B=/opt/rocm/llvm/bin
$B/llvm-objcopy -O binary --only-section=.hip_fatbin $in fatbin.bin
python3 - <<'PY'
import re, struct, subprocess
d = open("fatbin.bin", "rb").read()
n = 0
for m in re.finditer(rb"__CLANG_OFFLOAD_BUNDLE__", d):
    o = m.start(); cnt = struct.unpack_from("<Q", d, o + 24)[0]; p = o + 32
    for _ in range(cnt):
        off, size, tl = struct.unpack_from("<QQQ", d, p); tid = d[p + 24:p + 24 + tl].decode(); p += 24 + tl
        if "gfx950" in tid:
            open("co%d.elf" % n, "wb").write(d[o + off:o + off + size]); n += 1
print("code objects:", n)
PY
for f in co*.elf; do $B/llvm-objdump -d --no-show-raw-insn --no-leading-addr --symbolize-operands $f; done > all.s
python3 - <<'PY'
import re, os
os.makedirs("k", exist_ok=True)
cur = None; buf = []
def flush():
    if not cur: return
    while buf and buf[-1].strip() in ("s_nop 0", "...", ""): buf.pop()     # padding behind the last s_endpgm
    names = {}
    text = re.sub(r"\bL\d+\b", lambda m: names.setdefault(m.group(0), "L%d" % len(names)), "".join(buf))
    open("k/" + cur[:200], "w").write(text)
for line in open("all.s"):
    m = re.match(r"^<(\S+)>:$", line.strip())
    if m and re.match(r"L\d+$", m.group(1)): m = None
    if m:
        flush(); cur = m.group(1); buf = []; continue
    if cur: buf.append(re.sub(r"\s*//.*$", "", line.rstrip("\n")) + "\n")
flush()
print("symbols:", len(os.listdir("k")))
PY
