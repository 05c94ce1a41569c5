#!/usr/bin/env python3
"""dev: per-kernel diff of the gfx950 device assembly of two source trees.

    python tools/kernel_asm_diff.py OLD_TREE NEW_TREE [kernels/file.hip ...]

Compiles each .hip source (default: the halo conv kernels) of both trees to device assembly with
the library's flags (openpose_amd/build.py), cuts the assembly at the kernel symbols and compares
the instruction streams, ignoring comments, directives and the numbering of local labels.  Prints
one line per kernel symbol: same / DIFF (with the count of differing lines) / only in one tree.
Exit status 1 if any kernel present in both trees differs.  It only compiles and compares.
"""
import concurrent.futures as cf
import difflib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from openpose_amd.build import ARCH, COMMON, DEVICE, HIPCC  # noqa: E402

DEFAULT = ["conv3.hip", "conv3w.hip", "conv3w8.hip", "conv_head.hip"]
KDIR = os.path.join("openpose_amd", "csrc", "kernels")


def device_asm(tree, src, out):
    flags = [f for f in COMMON if not f.startswith("-I")] + ["-I" + os.path.join(tree, "include")]
    cmd = [HIPCC] + flags + ["-x", "hip"] + DEVICE + ["--cuda-device-only", "-S",
                                                     os.path.join(tree, KDIR, src), "-o", out]
    subprocess.run(cmd, check=True)
    with open(out) as f:
        return f.read()


def kernels(asm):
    """{symbol: [normalised instruction lines]} of every .amdhsa_kernel of the assembly text"""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    out, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^(\S+):", line)
        if m and m.group(1) in names:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        line = line.split(";")[0].strip()
        if not line or (line.startswith(".") and not line.startswith(".LBB")):
            continue
        cur.append(re.sub(r"\.LBB\d+_", ".LBB_", line))
    return out


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    old, new = sys.argv[1], sys.argv[2]
    srcs = sys.argv[3:] or DEFAULT
    bad = 0
    def one(job):
        i, tree, src = job
        if not os.path.exists(os.path.join(tree, KDIR, src)):
            return {}
        return kernels(device_asm(tree, src, os.path.join(tmp, "%d_%s.s" % (i, src))))

    with tempfile.TemporaryDirectory() as tmp, cf.ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
        jobs = [(i, tree, src) for src in srcs for i, tree in enumerate((old, new))]
        res = dict(zip([(i, src) for i, _, src in jobs], ex.map(one, jobs)))
        for src in srcs:
            ks = [res[(0, src)], res[(1, src)]]
            for name in sorted(set(ks[0]) | set(ks[1])):
                short = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
                short = short.replace("opk::(anonymous namespace)::", "").replace("(opk::ConvArgs)", "")
                if name not in ks[0] or name not in ks[1]:
                    print("%-12s %s (%d instructions)" % ("only old" if name in ks[0] else "only new", short,
                                                          len(ks[0].get(name) or ks[1].get(name))))
                elif ks[0][name] == ks[1][name]:
                    print("%-12s %s (%d instructions)" % ("same", short, len(ks[0][name])))
                else:
                    d = [x for x in difflib.unified_diff(ks[0][name], ks[1][name], lineterm="", n=0)
                         if x[:1] in "+-" and x[:3] not in ("+++", "---")]
                    print("%-12s %s (%d differing lines)" % ("DIFF", short, len(d)))
                    bad += 1
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
