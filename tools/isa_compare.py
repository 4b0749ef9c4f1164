#!/usr/bin/env python3
"""Function-by-function comparison of two device assembly files of the library (hipcc --cuda-device-only -S with the Makefile's
flags): which device functions exist in both, which differ in their instructions.  Comments, directives and the numbers of
basic-block labels are dropped, as profiles/r8a_draft_resources.txt did.  With the two -Rpass-analysis=kernel-resource-usage
logs it also prints every kernel's registers / LDS / scratch / occupancy whose row differs, and the rows of the new kernels.

    tools/isa_compare.py parent.s branch.s [parent.res branch.res]
"""
import re
import sys


def functions(path):
    out, name, body = {}, None, []
    for ln in open(path, errors="replace"):
        s = ln.split(";")[0].rstrip()
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", s)
        if m and not m.group(1).startswith((".L", "BB", ".Ltmp")):
            if name:
                out[name] = body
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        t = s.strip()
        if t.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        if not t or t.startswith(".") and not re.match(r"^\.LBB\d+_\d+:", t):
            continue
        t = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", t)
        t = re.sub(r"\s+", " ", t)
        body.append(t)
    if name:
        out[name] = body
    # (not code: the code object's metadata block and the translation unit's id symbol)
    return {k: v for k, v in out.items() if v and not k.startswith(("amdhsa.", "__hip_cuid_"))}


def resources(path):
    rows, cur = {}, None
    for ln in open(path, errors="replace"):
        m = re.search(r"remark:\s+Function Name: (\S+)", ln)
        if m:
            cur = m.group(1)
            rows[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", ln)
        if m and cur:
            rows[cur][m.group(1).strip()] = m.group(2)
    return rows


def main(argv):
    a, b = functions(argv[1]), functions(argv[2])
    same = [k for k in a if k in b and a[k] == b[k]]
    diff = [k for k in a if k in b and a[k] != b[k]]
    print("device functions: parent %d, branch %d; in both %d, instruction-identical %d, different %d" % (len(a), len(b), len(same) + len(diff), len(same), len(diff)))
    for k in diff:
        print("  DIFFERENT  %s: %d -> %d instructions" % (k, len(a[k]), len(b[k])))
    for k in sorted(set(a) - set(b)):
        print("  ONLY IN PARENT  %s (%d instructions)" % (k, len(a[k])))
    for k in sorted(set(b) - set(a)):
        print("  ONLY IN BRANCH  %s (%d instructions)" % (k, len(b[k])))
    if len(argv) >= 5:
        ra, rb = resources(argv[3]), resources(argv[4])
        keys = ["VGPRs", "AGPRs", "TotalSGPRs", "LDS Size", "ScratchSize", "VGPRs Spill", "SGPRs Spill", "Occupancy"]
        changed = [k for k in ra if k in rb and ra[k] != rb[k]]
        print("kernels with resource remarks: parent %d, branch %d; rows that differ: %d" % (len(ra), len(rb), len(changed)))
        for k in changed:
            print("  CHANGED  %s: %s -> %s" % (k, ra[k], rb[k]))
        for k in sorted(set(rb) - set(ra)):
            print("  NEW  %s: %s" % (k, ", ".join("%s %s" % (q, rb[k].get(q, "?")) for q in keys)))
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
