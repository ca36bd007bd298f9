#!/bin/sh
# Did the compiled device code stay? Compiles the device side of the device units of the working tree and of another revision with build.sh's flags
# (plain and -DKZ_EXPERIMENTS), disassembles the gfx950 code objects and compares them kernel by kernel. Needs no GPU. (kz_variance: a unit of the revisions
# before the denoiser's two became one; its kernels and kz_denoise's are compared as one set, by name. kz_responsive: the unit of kazen_mi355x_responsive.h, compiled
# like kz_denoise. kz_matte: the unit of kazen_mi355x_matte.h, compiled like the render units. kz_adaptive: the unit of kazen_mi355x_adaptive.h, compiled like kz_denoise.)
#   scripts/device_code_diff.sh <git-rev>
# Prints the kernels whose instructions differ - their own, or those of a device function they call (pathLi, matsLi, the texture filters ...) - with the
# kernel_resources.sh row of both sides, and exits non-zero if there is one. Instructions are compared as text without their addresses and encodings; the
# pc-relative literal behind an s_getpc_b64 is compared as the symbol it points to, so a kernel that only moved (because another one grew) counts as equal;
# so does one that became, or stopped being, the last of its code object (the padding behind it is left out). A kernel whose PARAMETER LIST changed has another
# mangled name on each side: the two are compared as one kernel when its name and template arguments are on both sides exactly once.
# (The code-object files themselves are no yardstick: two builds of equal instructions differ in a few hundred bytes of notes and hashes.)
set -e
[ -n "$1" ] || { echo "usage: $0 <git-rev>"; exit 2; }
REV=$1
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
LLVM=${ROCM_PATH:-/opt/rocm}/llvm/bin          # clang-offload-bundler, llvm-objdump, llvm-readelf: ROCm's own
OUT=$(mktemp -d /tmp/kzdcd.XXXXXX)
WT=$OUT/rev
git -C "$ROOT" worktree add --detach "$WT" "$REV" > /dev/null
trap 'git -C "$ROOT" worktree remove --force "$WT" > /dev/null 2>&1; rm -rf "$OUT"' EXIT
FLAGS="-O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function"
# one unit of one tree, device side only: <side> <tree> <build> <unit> <unit's device flags> -> $OUT/<side>.<build>.<unit>.{dis,sym,rem}
one() {
    B=$OUT/$1.$3.$4
    [ "$3" = exp ] && X=-DKZ_EXPERIMENTS || X=
    [ -f "$2/nano-kazen_amd/csrc/$4.hip" ] || { : > "$B.dis"; : > "$B.sym"; : > "$B.rem"; return 0; }      # (a unit the other revision does not have yet: every kernel of it is new)
    (cd "$2/nano-kazen_amd/csrc" && hipcc $FLAGS $5 $X ${KZ_EXTRA_HIPFLAGS} --cuda-device-only -Rpass-analysis=kernel-resource-usage -c $4.hip -o "$B.bundle" 2> "$B.rem") || { echo "$1 $3 $4: did not compile"; tail -5 "$B.rem"; return 1; }
    "$LLVM/clang-offload-bundler" --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input="$B.bundle" --output="$B.co" 2> /dev/null || cp "$B.bundle" "$B.co"      # (a compiler that does not bundle a lone device object)
    "$LLVM/llvm-objdump" -d --no-show-raw-insn "$B.co" > "$B.dis"
    "$LLVM/llvm-readelf" -sW "$B.co" > "$B.sym"
}
PIDS=""
for build in plain exp; do
    for side in this rev; do
        [ $side = this ] && TREE=$ROOT || TREE=$WT
        for u in kz_render kz_replica kz_film kz_film_moment kz_debug kz_motion kz_matte; do one $side "$TREE" $build $u "--offload-arch=gfx950 -fgpu-flush-denormals-to-zero -fno-slp-vectorize" & PIDS="$PIDS $!"; done
        for u in kz_refit kz_denoise kz_variance kz_responsive kz_adaptive; do one $side "$TREE" $build $u "--offload-arch=gfx950 -fno-slp-vectorize" & PIDS="$PIDS $!"; done      # (build.sh's IEEE units: no flush to zero)
    done
done
FAILED=0
for p in $PIDS; do wait $p || FAILED=1; done
[ $FAILED -eq 0 ] || { echo "device_code_diff: a unit did not compile"; exit 2; }
python3 - "$OUT" "$REV" <<'EOF'
import re, sys, subprocess, bisect
out, rev = sys.argv[1], sys.argv[2]

def symbols(path):          # FUNC / OBJECT symbols of the code object: sorted (value, size, name)
    syms = set()
    for l in open(path):
        f = l.split()
        if len(f) == 8 and f[3] in ("FUNC", "OBJECT") and f[6] != "UND": syms.add((int(f[1], 16), int(f[2]), f[7]))
    return sorted(syms)

def resolve(syms, addr):
    i = bisect.bisect_right(syms, (addr, 1 << 62, "")) - 1
    if i >= 0 and syms[i][0] <= addr < syms[i][0] + max(syms[i][1], 1): return "%s+%#x" % (syms[i][2], addr - syms[i][0])
    return "?+%#x" % addr

def functions(base):        # name -> (instruction texts, names of the functions it refers to)
    syms = symbols(base + ".sym")
    fns, cur, getpc = {}, None, False
    for l in open(base + ".dis"):
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", l)
        if m: cur = fns.setdefault(m.group(1), ([], set())); getpc = False; continue
        if cur is None or not l.startswith("\t"): continue
        text, _, note = l.partition("//")
        text = " ".join(text.split())
        m = re.match(r"s_add_u32 (s\d+), \1, (0x[0-9a-f]+|-?\d+)$", text) if getpc else None
        if m:               # s_getpc_b64 leaves this instruction's address; + the literal = what the pair points to
            lit = int(m.group(2), 0); lit -= (lit >> 31 & 1) << 32
            target = resolve(syms, int(note.split(":")[0], 16) + lit)
            text = "s_add_u32 %s, %s, <%s>" % (m.group(1), m.group(1), target)
            cur[1].add(target.rsplit("+", 1)[0])
        getpc = text.startswith("s_getpc_b64")
        cur[0].append(text)
    for text, _ in fns.values():          # the padding behind the last function of a code object is not that function's: a kernel may be the last on one side only
        while text and text[-1] in ("s_nop 0", "s_code_end", "..."): text.pop()
    kernels = {s[2][:-3] for s in syms if s[2].endswith(".kd")}
    return fns, kernels

def resources(path):        # kernel_resources.sh's row of every function
    cur, rows = None, {}
    for l in open(path, errors="replace"):
        m = re.search(r"remark: (?:.*?:\d+:\d+: )?\s*Function Name: (\S+)", l)
        if m: cur = m.group(1); rows[cur] = {}; continue
        m = re.search(r"remark: (?:.*?:\d+:\d+: )?\s*([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", l)
        if m and cur: rows[cur][m.group(1).strip()] = int(m.group(2))
    return {k: "VGPR %3d  SGPR %3d  spill v%-3d s%-3d scratch %4d  LDS %6d  occ %d" % (r.get("VGPRs", -1), r.get("TotalSGPRs", r.get("SGPRs", -1)), r.get("VGPRs Spill", 0),
                r.get("SGPRs Spill", 0), r.get("ScratchSize", 0), r.get("LDS Size", 0), r.get("Occupancy", 0)) for k, r in rows.items()}

def demangle(names):
    names = list(names)
    return dict(zip(names, subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.splitlines())) if names else {}

def side(which, build, units):          # functions, kernels and resource rows of one side's "unit+unit": one set
    fns, kernels, rows = {}, set(), {}
    for u in units.split("+"):
        base = "%s/%s.%s.%s" % (out, which, build, u)
        f, k = functions(base)
        fns.update(f); kernels |= k; rows.update(resources(base + ".rem"))
    return fns, kernels, rows

differing = 0
for build in ("plain", "exp"):
    for unit in ("kz_render", "kz_replica", "kz_film", "kz_film_moment", "kz_debug", "kz_motion", "kz_matte", "kz_refit", "kz_denoise+kz_variance", "kz_responsive", "kz_adaptive"):
        (fa, ka, ra), (fb, kb, rb) = side("this", build, unit), side("rev", build, unit)
        # kernels on one side only, paired by their demangled name without the parameter list: the other revision's takes this tree's mangled name
        lone = demangle((ka - kb) | (kb - ka))
        head = lambda n: lone[n].split("(")[0]
        for n in sorted(kb - ka):
            twins = [m for m in ka - kb if head(m) == head(n)]
            if len(twins) == 1 and sum(head(m) == head(n) for m in kb - ka) == 1:
                m = twins[0]
                fb[m] = fb.pop(n); kb = (kb - {n}) | {m}
                if n in rb: rb[m] = rb.pop(n)
        own = {n for n in set(fa) | set(fb) if n not in fa or n not in fb or fa[n][0] != fb[n][0]}
        # a kernel also differs through a device function it calls: close over the references
        why = {n: "its own instructions" for n in own}
        changed = True
        while changed:
            changed = False
            for n in set(fa) & set(fb):
                if n in why: continue
                for c in sorted(fa[n][1] | fb[n][1]):
                    if c in why and c not in (ka | kb): why[n] = "calls " + c; changed = True; break
        kernels = ka | kb
        names = demangle(set(why) | kernels | {w[6:] for w in why.values() if w.startswith("calls ")})
        short = lambda n: names.get(n, n).split("(")[0].replace("void ", "")
        bad = sorted(n for n in why if n in kernels)
        print("%-5s %-22s %3d kernels, %d differ from %s%s" % (build, unit, len(kernels), len(bad), rev, "".join("; device function %s differs" % short(n) for n in sorted(own - kernels))))
        for n in bad:
            differing += 1
            reason = why[n] if not why[n].startswith("calls ") else "calls " + short(why[n][6:])
            if n not in fa or n not in fb: reason = "only in " + ("this tree" if n in fa else rev)
            else: reason += ", %d -> %d instructions" % (len(fb[n][0]), len(fa[n][0]))
            print("  %s: %s" % (short(n), reason))
            print("      %-10s %s" % (rev[:10], rb.get(n, "-")))
            print("      %-10s %s" % ("this tree", ra.get(n, "-")))
print("device_code_diff: %d kernel(s) differ" % differing if differing else "device_code_diff: every kernel's instructions are those of " + rev)
sys.exit(1 if differing else 0)
EOF
