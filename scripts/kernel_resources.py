"""Tabulate hipcc's -Rpass-analysis=kernel-resource-usage remarks: one line per kernel with its SGPRs, VGPRs,
AGPRs, scratch bytes per lane, LDS bytes per block and occupancy (waves per SIMD).

  hipcc <the Makefile's flags> -Rpass-analysis=kernel-resource-usage -c bn.hip -o /dev/null 2> bn.txt
  python scripts/kernel_resources.py bn.txt inorm.txt ...          # the table
  python scripts/kernel_resources.py --compare OLD.tab NEW.tab [MAP]   # rows side by side; exit 1 on a difference

MAP holds "old name<TAB>new name" lines for kernels that were renamed (a kernel that became a template
instantiation); names are the demangled ones without their parameter lists."""
import re
import subprocess
import sys

FIELDS = [("TotalSGPRs", "sgpr"), ("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("ScratchSize [bytes/lane]", "scratch"),
          ("LDS Size [bytes/block]", "lds"), ("Occupancy [waves/SIMD]", "occ")]


def short(name):
    """demangled name without the parameter list: stc::k<float, true>(View, ...) -> k<float, true>"""
    depth, out = 0, []
    for ch in name:
        if ch == "(" and depth == 0:
            break
        depth += ch == "<"
        depth -= ch == ">"
        out.append(ch)
    s = "".join(out).replace("void ", "").replace("stc::", "").replace("__hip_bfloat16", "bf16")
    return s.replace("(anonymous namespace)::", "").strip()


def table(paths):
    rows = {}
    for path in paths:
        cur = None
        for line in open(path):
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                cur = rows.setdefault(m.group(1), {})
                continue
            for key, col in FIELDS:
                m = re.search(r"remark:\s+" + re.escape(key) + r": (\d+)", line)
                if m and cur is not None:
                    cur[col] = int(m.group(1))
    names = list(rows)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    out = sorted((short(d), rows[n]) for n, d in zip(names, dem))
    print(f"{'kernel':<64} " + " ".join(f"{c:>7}" for _, c in FIELDS))
    for name, r in out:
        print(f"{name:<64} " + " ".join(f"{r.get(c, -1):>7}" for _, c in FIELDS))


def load(path):
    rows = {}
    for line in open(path).read().splitlines()[1:]:
        m = re.match(r"(.*?)\s+((?:-?\d+\s*){%d})$" % len(FIELDS), line)
        if m:
            rows[m.group(1)] = tuple(int(v) for v in m.group(2).split())
    return rows


def compare(a, b, mapping=None):
    A, B = load(a), load(b)
    ren = dict(l.rstrip("\n").split("\t") for l in open(mapping) if "\t" in l) if mapping else {}
    bad, seen = 0, set()
    print(f"{'kernel (old -> new)':<100} " + " ".join(f"{c:>7}" for _, c in FIELDS) + "  verdict")
    for name, ra in A.items():
        new = ren.get(name, name)
        seen.add(new)
        rb = B.get(new)
        same = ra == rb
        bad += not same
        label = name if new == name else f"{name} -> {new}"
        print(f"{label:<100} " + " ".join(f"{v:>7}" for v in ra) + ("  equal" if same else f"  DIFFERENT: new {rb}"))
    for name in B:
        if name not in seen:
            print(f"{name:<100} only in {b}: {B[name]}")
            bad += 1
    print(f"{len(A)} kernels, {bad} differing")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        compare(*sys.argv[2:5])
    else:
        table(sys.argv[1:])
