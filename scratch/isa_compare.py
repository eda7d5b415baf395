"""Per-kernel comparison of two builds of one HIP source: device assembly (--save-temps) and the figures of
-Rpass-analysis=kernel-resource-usage.

    python scratch/isa_compare.py SOURCE.hip PARENT_CSRC_DIR THIS_CSRC_DIR WORK_DIR

compiles SOURCE.hip from both directories for gfx950 with the flags of nbdt/_build.py, splits each device .s into its
kernels, and prints per kernel "identical" or a unified diff of the instruction streams, then the resource figures of
both sides.  Kernels are matched by demangled name without namespaces; block labels are renumbered per kernel (their
numbers count the functions in front of them in the file)."""
import difflib
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "neural-backed-decision-trees_amd"))
from nbdt import _build  # noqa: E402

RENAMED = {"mb_bwd_finalize_kernel": "bn_bwd_finalize_kernel"}


def compile_side(src, csrc, work):
    os.makedirs(work, exist_ok=True)
    cmd = [_build.hipcc()] + _build.COMMON + _build.FLAGS.get(src, []) + [
        "-I", _build.INCLUDE, "--save-temps", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.abspath(os.path.join(csrc, src)),
        "-o", "out.o"]
    r = subprocess.run(cmd, cwd=work, capture_output=True, text=True)
    if r.returncode:
        raise SystemExit(r.stderr)
    asm = [f for f in os.listdir(work) if f.endswith(".s") and "amdgcn" in f]
    assert len(asm) == 1, asm
    return open(os.path.join(work, asm[0])).read(), r.stderr


def plain(mangled):
    name = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
    name = name.replace("(anonymous namespace)::", "").replace("nbdt::", "")
    name = re.sub(r"^void ", "", name)
    name = re.sub(r"\(.*$", "", name) if "<" not in name else re.sub(r">\(.*$", ">", name)
    for a, b in RENAMED.items():
        name = name.replace(a, b)
    return name


def kernels(asm):
    """{plain name: [instruction lines]} of every .amdhsa kernel of a device assembly file."""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    out = {}
    for sym in names:
        m = re.search(r"^" + re.escape(sym) + r":[^\n]*\n(.*?)^\.Lfunc_end\d+:", asm, re.M | re.S)
        body = []
        for line in m.group(1).splitlines():
            line = re.sub(r"\s*;.*$", "", line).strip()
            if not line or line.startswith("."):
                if not re.match(r"\.LBB\d+_\d+:", line):
                    continue
            line = re.sub(r"\.LBB\d+_", ".LBB_", line)
            body.append(line)
        out[plain(sym)] = body
    return out


def resources(remarks):
    """{plain name: {figure: value}} from the kernel-resource-usage remarks."""
    out, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark: (?:.*?: )?Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(plain(m.group(1)), {})
            continue
        m = re.search(r"remark: (?:.*?: )?\s*(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" ")[0].replace("Total", "")] = int(m.group(2))
    return out


def main():
    src, parent, this, work = sys.argv[1:5]
    a_asm, a_rem = compile_side(src, parent, os.path.join(work, "parent_" + src))
    b_asm, b_rem = compile_side(src, this, os.path.join(work, "this_" + src))
    a, b = kernels(a_asm), kernels(b_asm)
    ra, rb = resources(a_rem), resources(b_rem)
    print(f"== {src}: {len(a)} kernels at the parent, {len(b)} in this tree")
    same = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print(f"{name}: only {'at the parent' if name in a else 'in this tree'}")
            continue
        fig = lambda r: " ".join(f"{k} {v}" for k, v in sorted(r.get(name, {}).items()))
        if a[name] == b[name]:
            same += 1
            verdict = f"identical ({len(a[name])} lines)"
        else:
            verdict = "DIFFERS"
        print(f"{name}: {verdict} | parent: {fig(ra)} | this tree: {fig(rb)}")
        if a[name] != b[name]:
            for d in difflib.unified_diff(a[name], b[name], "parent", "this tree", lineterm="", n=2):
                print("    " + d)
    print(f"== {src}: {same} of {len(set(a) | set(b))} kernels identical")


if __name__ == "__main__":
    main()
