"""Compare the instruction streams of the kernels two device assembly listings have in common (labels and comments dropped):
    python profiles/tools/isa_diff.py /tmp/base.s build/obj/trm_launch_column_f64_euler_rich.s
Used to show that moving kernel instantiations between translation units leaves their code unchanged.  Kernels are paired by name; an
optional third argument OLD=NEW pairs the one kernel of the first listing whose mangled name contains OLD with the one of the second
whose name contains NEW (a kernel that was renamed, or became a template):
    python profiles/tools/isa_diff.py parent.s branch.s 17k_closure_tangentE=17k_closure_tangentI
or @FILE, a file of such pairs, one per line (blank lines and # comments skipped); the pairs whose OLD occurs in the first listing are
applied, each to exactly one kernel on either side, and with --resources the .amdhsa_kernarg_size, .amdhsa_next_free_vgpr and
.amdhsa_next_free_sgpr of every common kernel are compared as well:
    python profiles/tools/isa_diff.py parent.s branch.s @profiles/r19/kernel_pairs.txt --resources
The exit status is 1 if a common kernel differs or the two listings do not hold the same kernels after pairing."""
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r'^(_Z\S+):', line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        s = line.strip()
        if s.startswith('.Lfunc_end'):
            out[name] = body
            name = None
            continue
        if line.startswith('\t') and not s.startswith(('.', ';')):
            body.append(re.sub(r'\.LBB\d+_', '.LBB_', re.sub(r'\s*;.*$', '', s)))   # (block labels carry the function's index in its file)
    return out


def resources(path):
    out, name = {}, None
    for line in open(path):
        m = re.match(r'^\s*\.amdhsa_kernel\s+(\S+)', line)
        if m:
            name = m.group(1)
            out[name] = {}
        m = re.match(r'^\s*\.amdhsa_(kernarg_size|next_free_vgpr|next_free_sgpr)\s+(\S+)', line)
        if m and name:
            out[name][m.group(1)] = m.group(2)
    return out


args = [x for x in sys.argv[1:] if x != '--resources']
a, b = kernels(args[0]), kernels(args[1])
ra, rb = resources(args[0]), resources(args[1])
pairs = []
if len(args) > 2:
    spec = args[2]
    text = open(spec[1:]).read().splitlines() if spec.startswith('@') else [spec]
    pairs = [tuple(l.split('=')) for l in (l.strip() for l in text) if l and not l.startswith('#')]
renamed = 0
for old, new in pairs:
    ka = [k for k in a if old in k]
    if spec.startswith('@') and not ka:
        continue                                     # (a pair of another translation unit)
    (ka,), (kb,) = ka, [k for k in b if new in k]
    a[kb] = a.pop(ka)
    ra[kb] = ra.pop(ka)
    renamed += 1
same = [k for k in b if k in a and a[k] == b[k]]
diff = [k for k in b if k in a and a[k] != b[k]]
only = sorted(set(a) ^ set(b))
print(f"{len(a)} / {len(b)} kernels; common {len(same) + len(diff)} ({renamed} paired by rename): identical {len(same)}, different {len(diff)}")
for k in diff:
    print("  DIFF", k[:110], len(a[k]), len(b[k]))
for k in only:
    print("  ONLY IN", "FIRST" if k in a else "SECOND", k[:110])
bad = len(diff) + len(only)
if '--resources' in sys.argv:
    moved = [k for k in b if k in a and ra.get(k) != rb.get(k)]
    print(f"  resources (kernarg_size, next_free_vgpr, next_free_sgpr): equal {len([k for k in b if k in a]) - len(moved)}, different {len(moved)}")
    for k in moved:
        print("  RESOURCES", k[:110], ra.get(k), rb.get(k))
    bad += len(moved)
sys.exit(1 if bad else 0)
