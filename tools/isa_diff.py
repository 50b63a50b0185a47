"""Compare the gfx950 code of selected kernels between two assembly listings (hipcc -save-temps=obj: *-gfx950.s).

    python tools/isa_diff.py OLD.s NEW.s [name-substring ...]      (default: k_scan)

For every kernel whose DEMANGLED name contains one of the substrings: the instruction stream between its label and its
s_endpgm-terminated body's .Lfunc_end, with local labels (.LBB<n>_<m>) renumbered per kernel, compared as text.  Prints one
line per kernel -- same / DIFFERENT (with the first differing lines) / only in OLD / only in NEW -- and exits 1 when a kernel
present in both differs.  Needs no GPU.
"""
import re
import subprocess
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = body
                name = None
                continue
            t = line.split(";")[0].rstrip()
            if t.strip() and not t.strip().startswith((".p2align", ".loc", ".cfi", ".file")):
                body.append(t.strip())
    return out


def normalise(body):
    seen = {}

    def lab(m):
        return seen.setdefault(m.group(0), f".L{len(seen)}")
    return [re.sub(r"\.LBB\d+_\d+", lab, t) for t in body]


def demangle(names):
    if not names:
        return {}
    txt = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, txt))


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    subs = sys.argv[3:] or ["k_scan"]
    dm = demangle(sorted(set(old) | set(new)))
    bad = 0
    for n in sorted(set(old) | set(new), key=lambda n: dm[n]):
        if not any(s in dm[n] for s in subs):
            continue
        short = dm[n].split("(")[0].replace("void ", "")
        if n not in new:
            print(f"only in OLD   {short}")
        elif n not in old:
            print(f"only in NEW   {short}  ({len(new[n])} lines)")
        else:
            a, b = normalise(old[n]), normalise(new[n])
            if a == b:
                print(f"same          {short}  ({len(a)} lines)")
            else:
                bad += 1
                first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
                print(f"DIFFERENT     {short}  ({len(a)} / {len(b)} lines; first difference at line {first}: {a[first:first + 1]} / {b[first:first + 1]})")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
