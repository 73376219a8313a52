#!/bin/bash
# asm_vs_rev.sh <rev> <file.hip>...: is the gfx950 code of these translation units the code they had at <rev>?
# Both versions (the working tree's and `git archive <rev>`'s, each with its own headers and its own Makefile's flags for that
# file) are compiled with -S --cuda-device-only; comment lines and the __hip_cuid_* symbol are dropped, function-local LDS symbols
# (_ZZ<function>E<name>) are renamed to <name> and the function ordinal of block labels (.LBB<n>_<m> -> .LBB_<m>: it moves when a
# function is added or removed anywhere before in the file) is dropped; then the text of every kernel is compared, one line per kernel
# with both instruction counts:
#   identical           the same text
#   same instructions   the same multiset of (mnemonic, non-register operands: immediates, offsets, modifiers, s_waitcnt fields), and
#                       therefore the same count: register numbers, the order of operands and the order of instructions may differ
#   differs             anything else
# A kernel of one side only is listed as such.  Only the text between a
# function's label and its end is compared: the .amdhsa_* metadata (LDS size, register counts) is not, so read the result together
# with tools/kernel_resources.sh at both revisions.
# ASM_KEEP=<dir> keeps the normalised listings (<dir>/{old,new}/<file>.s) for a closer look with diff.
set -euo pipefail
[ $# -ge 2 ] || { echo "usage: $0 <rev> <file.hip>..." >&2; exit 2; }
rev=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
tmp=$(mktemp -d); trap 'rm -rf "$tmp"' EXIT
mkdir -p "$tmp/old" "$tmp/out/old" "$tmp/out/new"
git -C "$root" archive "$rev" dj_brdf_amd/csrc include | tar -x -C "$tmp/old"

# the Makefile's own command line for <file>.o, with -c turned into -S --cuda-device-only
compile() {   # <csrc dir> <file.hip> <out.s>
	local cmd
	cmd=$(make -C "$1" -s -n -B "build/${2%.hip}.o" | grep -- ' -c ' | head -1 | sed -e 's/ -c / -S --cuda-device-only /' -e "s| -o .*| -o $3|")
	(cd "$1" && eval "$cmd")
}
for f in "$@"; do
	f=$(basename "$f")
	compile "$tmp/old/dj_brdf_amd/csrc" "$f" "$tmp/out/old/$f.s" &
	compile "$root/dj_brdf_amd/csrc" "$f" "$tmp/out/new/$f.s" &
	wait
	python3 - "$f" "$tmp/out/old/$f.s" "$tmp/out/new/$f.s" "${ASM_KEEP:-}" <<'EOF'
import re, subprocess, sys, os
name, keep = sys.argv[1], sys.argv[4]
def local_name(m):      # _ZZ<function>E<len><name>[_<n>] -> <name>: the rightmost E<len> whose <len> is the length of what follows
    t = m.group(0)
    for e in reversed(list(re.finditer(r'E(\d+)', t))):
        n, rest = int(e.group(1)), t[e.end():]
        if len(rest) >= n and re.fullmatch(r'(_\d*)?', rest[n:]): return rest[:n]
    return t
def kernels(path, side):
    lines = []
    for l in open(path):
        l = l.rstrip()
        if not l.strip() or l.lstrip().startswith(';') or '__hip_cuid_' in l: continue
        l = re.sub(r'\s*;.*$', '', l)                                   # trailing comments (register-pressure notes and the like)
        l = re.sub(r'_ZZ\w+', local_name, l)
        l = re.sub(r'\.LBB\d+_', '.LBB_', l)                          # the function's ordinal in the file
        lines.append(l)
    if keep:
        os.makedirs(os.path.join(keep, side), exist_ok=True)
        open(os.path.join(keep, side, name + '.s'), 'w').write('\n'.join(lines) + '\n')
    funcs = {m.group(1) for l in lines for m in [re.match(r'\s*\.type\s+(\w+),@function', l)] if m}
    out, cur = {}, None
    for l in lines:
        m = re.match(r'^(\w+):$', l)
        if m and m.group(1) in funcs: cur = m.group(1); out[cur] = []; continue
        if cur is not None:
            if l.startswith('.Lfunc_end'): cur = None
            else: out[cur].append(l)
    return out
REG = re.compile(r'^-?\|?(?:[vsa]\d+|[vsa]\[\d+:\d+\]|vcc(?:_lo|_hi)?|exec(?:_lo|_hi)?|scc|m0|off|null|\.LBB_\d+)\|?$')
def bag(body):          # the multiset of (mnemonic, sorted non-register operands)
    out = []
    for l in body:
        if not l.startswith('\t') or l.lstrip().startswith('.'): continue
        t = l.split(None, 1)
        ops = [o for o in re.split(r'[,\s]+', t[1]) if o and not REG.match(o)] if len(t) > 1 else []
        out.append((t[0], tuple(sorted(ops))))
    return sorted(out)
def count(body): return sum(1 for l in body if l.startswith('\t') and not l.lstrip().startswith('.'))
old, new = kernels(sys.argv[2], 'old'), kernels(sys.argv[3], 'new')
names = list(dict.fromkeys(list(old) + list(new)))
pretty = subprocess.run(['c++filt'] + names, capture_output=True, text=True).stdout.splitlines()
n_diff = 0
for k, p in zip(names, pretty):
    p = re.sub(r'\(anonymous namespace\)::', '', p); p = re.sub(r'\(.*', '', p).replace('void ', '')
    if k not in old: print(f'{name}: {p:60s} only in the working tree ({count(new[k])} instructions)'); n_diff += 1
    elif k not in new: print(f'{name}: {p:60s} only at the revision ({count(old[k])} instructions)'); n_diff += 1
    else:
        verdict = 'identical' if old[k] == new[k] else 'same instructions' if bag(old[k]) == bag(new[k]) else 'differs'
        n_diff += verdict == 'differs'
        print(f"{name}: {p:60s} {verdict:17s} {count(old[k]):6d} {count(new[k]):6d}")
print(f'{name}: {len(names)} kernels, {n_diff} differ')
EOF
done
