"""Compare the instruction streams of the kernels two device assembly listings have in common (labels and comments dropped):
    python profiles/tools/isa_diff.py /tmp/base.s build/obj/trm_launch_column_f64_euler_rich.s
Used to show that moving kernel instantiations between translation units leaves their code unchanged.  Kernels are paired by name; an
optional third argument OLD=NEW pairs the one kernel of the first listing whose mangled name contains OLD with the one of the second
whose name contains NEW (a kernel that was renamed, or became a template):
    python profiles/tools/isa_diff.py parent.s branch.s 17k_closure_tangentE=17k_closure_tangentI"""
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


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
if len(sys.argv) > 3:
    old, new = sys.argv[3].split('=')
    (ka,), (kb,) = [k for k in a if old in k], [k for k in b if new in k]
    a[kb] = a.pop(ka)
same = [k for k in b if k in a and a[k] == b[k]]
diff = [k for k in b if k in a and a[k] != b[k]]
print(f"{len(a)} / {len(b)} kernels; common {len(same) + len(diff)}: identical {len(same)}, different {len(diff)}")
for k in diff:
    print("  DIFF", k[:110], len(a[k]), len(b[k]))
