"""Compare the device assembly of two builds of one .hip file, function by function.

  hipcc <the Makefile's flags> --cuda-device-only -S bn.hip -o new.s        (and the same for the other tree)
  python scripts/isa_compare.py OLD.s NEW.s

A function is the text between its label and its .Lfunc_end, without comments, blank lines and debug directives; local
labels (.LBBn_m) carry the function's ordinal in the file, which moves when functions are added, so that ordinal is
blanked.  Prints one line per function (demangled, without the parameter list): identical / DIFFERENT / only in one
file, and exits 1 when a function both files have differs."""
import re
import subprocess
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path):
        line = line.split(";")[0].rstrip()
        if not line.strip():
            continue
        if name is None:
            m = re.match(r"^([A-Za-z_][\w$.]*):", line)
            if m and not m.group(1).startswith(".L"):
                name, body = m.group(1), []
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        s = line.strip()
        if s.startswith((".loc", ".file", ".cfi", ".p2align")):
            continue
        body.append(re.sub(r"\.L(BB|tmp|JTI)\d+_", r".L\1N_", s))
    return out


def short(name):
    depth, out = 0, []
    for ch in name:
        if ch == "(" and depth == 0:
            break
        depth += ch == "<"
        depth -= ch == ">"
        out.append(ch)
    return "".join(out).replace("void ", "").replace("stc::", "").replace("__hip_bfloat16", "bf16").strip()


def main(old, new):
    A, B = functions(old), functions(new)
    names = sorted(set(A) | set(B))
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    bad = 0
    for n, d in sorted(zip(names, dem), key=lambda p: p[1]):
        if n not in A or n not in B:
            print(f"{short(d):<72} only in {new if n in B else old} ({len(B.get(n) or A.get(n))} lines)")
            continue
        same = A[n] == B[n]
        bad += not same
        print(f"{short(d):<72} {'identical' if same else 'DIFFERENT'} ({len(A[n])} / {len(B[n])} lines)")
    both = sum(n in A and n in B for n in names)
    print(f"{both} functions in both files, {bad} differing; {len(B) - both} only in {new}, {len(A) - both} only in {old}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
