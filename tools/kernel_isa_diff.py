"""Compares the gfx950 device code of two source trees kernel by kernel (text only, no GPU).

    python tools/kernel_isa_diff.py PARENT_TREE HEAD_TREE [--work DIR] [-j N]

Every csrc/*.hip of a tree's build.py SOURCES is compiled with that build.py's flags for the file plus
--cuda-device-only -S.  The assembly is cut into one piece per kernel (body and .amdhsa_kernel block) and what
depends only on a function's position in its module is normalised: the function index in local labels (and in the
loop comments that quote them) and the __hip_cuid_* symbol.  Prints the counts of equal, differing and only-in-parent
kernels and the names of the last two groups and of kernels only in the head; exits 1 if a kernel differs or exists only in the head.
--work keeps the .s files, and a file newer than all of its tree's sources is not compiled again.
"""
import argparse
import os
import re
import runpy
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

NORMALISE = [(re.compile(r"\bL?BB\d+_"), "BB_"), (re.compile(r"\.LJTI\d+_"), ".LJTI_"),
             (re.compile(r"\.L(func_end|func_begin|tmp)\d+"), r".L\1"), (re.compile(r"__hip_cuid_\w+"), "__hip_cuid"),
             (re.compile(r"[ \t]+;"), " ;")]     # a comment's column follows the length of the label in front of it


def compile_tree(tree, out, jobs):
    pkg = os.path.join(tree, "mri_superresolution_amd")
    b = runpy.run_path(os.path.join(pkg, "build.py"), run_name="build")
    csrc = os.path.join(pkg, "csrc")
    newest = max(os.path.getmtime(os.path.join(d, f)) for d in (csrc, os.path.join(tree, "include")) for f in os.listdir(d))
    os.makedirs(out, exist_ok=True)

    def one(src):
        asm = os.path.join(out, src + ".s")
        if not (os.path.exists(asm) and os.path.getmtime(asm) >= newest):
            cmd = [b["HIPCC"], *b["FLAGS"], *b["FILE_FLAGS"].get(src, []), "--cuda-device-only", "-S", os.path.join(csrc, src), "-o", asm]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError(f"hipcc failed for {src}:\n{r.stderr}")
        return asm

    with ThreadPoolExecutor(max_workers=jobs) as ex:
        return list(ex.map(one, [s for s in b["SOURCES"] if s.endswith(".hip")]))


def kernels(asm_files):
    """{kernel symbol: normalised text from its label to .end_amdhsa_kernel}"""
    out = {}
    for path in asm_files:
        lines = open(path).read().split("\n")
        label = {m.group(1): i for i, l in enumerate(lines) if (m := re.match(r"(\w+):", l))}
        for i, l in enumerate(lines):
            if not l.startswith("\t.amdhsa_kernel "):
                continue
            name = l.split()[1]
            end = next(j for j in range(i, len(lines)) if lines[j].startswith("\t.end_amdhsa_kernel"))
            text = "\n".join(lines[label[name]:end + 1])
            for rx, to in NORMALISE:
                text = rx.sub(to, text)
            if out.setdefault(name, text) != text:
                raise RuntimeError(f"{name} is defined twice with different code ({path})")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("head")
    ap.add_argument("--work")
    ap.add_argument("-j", type=int, default=8)
    a = ap.parse_args()
    work = a.work or tempfile.mkdtemp(prefix="kernel_isa_diff_")
    parent = kernels(compile_tree(a.parent, os.path.join(work, "parent"), a.j))
    head = kernels(compile_tree(a.head, os.path.join(work, "head"), a.j))
    equal = [k for k in head if parent.get(k) == head[k]]
    differing = [k for k in head if k in parent and parent[k] != head[k]]
    only_parent = [k for k in parent if k not in head]
    only_head = [k for k in head if k not in parent]
    for title, names in (("differing", differing), ("only in parent", only_parent), ("only in head", only_head)):
        for k in sorted(names):
            print(f"{title}: {k}")
    print(f"equal {len(equal)}  differing {len(differing)}  only-in-parent {len(only_parent)}  only-in-head {len(only_head)}")
    return 1 if differing or only_head else 0


if __name__ == "__main__":
    sys.exit(main())
