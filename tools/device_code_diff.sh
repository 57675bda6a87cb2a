#!/bin/bash
# Did a host-only change leave the device code alone?  tools/device_code_diff.sh OBJDIR_BEFORE OBJDIR_AFTER
# Both object directories (change3d_amd/lib/obj or obj_tune) must come from builds at the SAME checkout path.  Per object
# and per kernel symbol (sorted by name: the order inside a code object may move): the disassembly (tools/isa_extract.sh,
# addresses stripped) and the register / scratch / spill / LDS line (tools/kernel_regs.sh).  Exit status 1 on any difference.
set -eu
A=$1; B=$2; HERE=$(dirname "$0"); TMP=$(mktemp -d); trap 'rm -rf "$TMP"' EXIT
bad=0
for oa in "$A"/*.o; do
  n=$(basename "$oa" .o); ob="$B/$n.o"
  [ -f "$ob" ] || { echo "$n: missing in $B"; bad=1; continue; }
  for s in a b; do
    [ $s = a ] && o=$oa || o=$ob
    bash "$HERE/isa_extract.sh" "$o" "$TMP/$n.$s" > /dev/null
    bash "$HERE/kernel_regs.sh" "$o" > "$TMP/$n.$s/regs.txt"
  done
  python3 - "$n" "$TMP/$n.a" "$TMP/$n.b" <<'EOF' || bad=1
import re, sys
def load(d):
    isa, cur = {}, None
    for line in open(d + "/k.s"):
        m = re.match(r"[0-9a-f]+ <(.+)>:$", line)
        if m: cur = isa.setdefault(re.sub(r"\.intern\.[0-9a-f]+|__intern__[0-9a-f]+", "", m.group(1)), [])
        elif cur is not None and line.strip(): cur.append(re.sub(r"\s*//.*$", "", line).strip())
    regs = {}   # kernel_regs.sh cuts names at 150 characters: keep every line of a cut name, sorted
    for f in (l.strip().split(None, 6) for l in open(d + "/regs.txt") if l.startswith("v=")): regs.setdefault(f[6], []).append(f[:6])
    return isa, {k: sorted(v) for k, v in regs.items()}
(ia, ra), (ib, rb) = load(sys.argv[2]), load(sys.argv[3])
added, missing = sorted(set(ib) - set(ia)), sorted(set(ia) - set(ib))
differ = [k for k in sorted(set(ia) & set(ib)) if ia[k] != ib[k]] + [k for k in sorted(set(ra) | set(rb)) if ra.get(k) != rb.get(k)]
print("%-14s %3d kernels, %7d instructions: %d differ, %d added, %d missing" % (sys.argv[1], len(ia), sum(map(len, ia.values())), len(differ), len(added), len(missing)))
for k in differ + added + missing: print("    " + k[:150])
sys.exit(1 if differ or added or missing else 0)
EOF
done
exit $bad
