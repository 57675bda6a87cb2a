#!/bin/bash
# Did a host-only change leave the device code alone?  tools/device_code_diff.sh OBJDIR_BEFORE OBJDIR_AFTER
# Both object directories (change3d_amd/lib/obj or obj_tune) must come from builds at the SAME checkout path.  Per object
# and per kernel symbol (sorted by name: the order inside a code object may move): the disassembly (tools/isa_extract.sh,
# addresses stripped) and the register / scratch / spill / LDS line (tools/kernel_regs.sh).  Exit status 1 on any difference.
# An object without device code on both sides (options.o) is named and skipped.
# A kernel whose template signature was renamed is compared under a common name when DCD_RENAME gives one: lines of
# `python-regex=>replacement`, applied to the demangled names of both sides, e.g.
#   DCD_RENAME='void old_kernel<(\w+)>\(.*=>K \1
#   void new_kernel<Policy<(\w+)>>\(.*=>K \1'
set -eu
A=$1; B=$2; HERE=$(dirname "$0"); TMP=$(mktemp -d); trap 'rm -rf "$TMP"' EXIT
bad=0
for oa in "$A"/*.o; do
  n=$(basename "$oa" .o); ob="$B/$n.o"
  [ -f "$ob" ] || { echo "$n: missing in $B"; bad=1; continue; }
  none=0
  for s in a b; do
    [ $s = a ] && o=$oa || o=$ob
    if bash "$HERE/isa_extract.sh" "$o" "$TMP/$n.$s" > /dev/null 2>&1; then
      bash "$HERE/kernel_regs.sh" "$o" > "$TMP/$n.$s/regs.txt"
    else
      none=$((none + 1))
    fi
  done
  [ $none = 2 ] && { echo "$n: no device code"; continue; }
  [ $none = 1 ] && { echo "$n: device code on one side only"; bad=1; continue; }
  python3 - "$n" "$TMP/$n.a" "$TMP/$n.b" <<'EOF' || bad=1
import os, re, subprocess, sys
ren = [tuple(r.strip().split("=>", 1)) for r in os.environ.get("DCD_RENAME", "").split("\n") if "=>" in r]
def common(name):   # demangled name -> the name it is compared under
    name = re.sub(r"\(anonymous namespace\)::", "", name)
    for pat, rep in ren:
        name = re.sub(pat, rep, name)
    return name
def load(d):
    isa, cur, names = {}, None, []
    for line in open(d + "/k.s"):
        m = re.match(r"[0-9a-f]+ <(.+)>:$", line)
        if m: names.append(re.sub(r"\.intern\.[0-9a-f]+|__intern__[0-9a-f]+", "", m.group(1))); cur = isa.setdefault(names[-1], [])
        elif cur is not None and line.strip(): cur.append(re.sub(r"\s*//.*$", "", line).strip())
    if ren:   # only then are the disassembly's (mangled) names rewritten
        dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
        isa = {common(dn): isa[mn] for mn, dn in zip(names, dem)}
    regs = {}   # kernel_regs.sh cuts names at 150 characters: keep every line of a cut name, sorted
    for f in (l.strip().split(None, 6) for l in open(d + "/regs.txt") if l.startswith("v=")): regs.setdefault(common(f[6]), []).append(f[:6])
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
