#!/usr/bin/env python3
"""Are the kernels of two builds the same code?  Compares the device assembly that
`hipcc --save-temps` leaves (*-hip-amdgcn-amd-amdhsa-gfx950.s) kernel by kernel: the instruction
stream of each, without comments and directives and with the basic-block labels renumbered in
order of appearance.

    tools/compare_kernels.py parent/tsdf_dense-hip-amdgcn-amd-amdhsa-gfx950.s new/tsdf_dense-...gfx950.s

Prints the kernel counts and the names that differ; exit status 1 if any does."""
import re
import sys


def kernels(path):
    text = open(path).read()
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out, cur, body = {}, None, []
    for line in text.splitlines():
        m = re.match(r"^([A-Za-z_$][\w$.]*):", line)
        if cur is None:
            if m and m.group(1) in names:
                cur, body = m.group(1), []
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            out[cur], cur = body, None
            continue
        code = line.split(";", 1)[0].strip()
        if not code or (code.startswith(".") and not code.endswith(":")):
            continue
        body.append(code)
    for name, body in out.items():  # renumber the labels in order of appearance
        ids = {}
        def ren(m):
            return ids.setdefault(m.group(0), ".L%d" % len(ids))
        out[name] = [re.sub(r"\.L[A-Za-z_]*\d+(?:_\d+)?", ren, c) for c in body]
    return out


def main(a, b):
    ka, kb = kernels(a), kernels(b)
    differ = sorted(n for n in set(ka) | set(kb) if ka.get(n) != kb.get(n))
    print(f"{a}: {len(ka)} kernels, {sum(map(len, ka.values()))} instructions")
    print(f"{b}: {len(kb)} kernels, {sum(map(len, kb.values()))} instructions")
    print(f"identical: {len(set(ka) & set(kb)) - sum(n in ka and n in kb for n in differ)}, differ: {len(differ)}")
    for n in differ:
        print("  differs:", n, len(ka.get(n, [])), "->", len(kb.get(n, [])))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
