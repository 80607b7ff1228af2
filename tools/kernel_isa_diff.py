"""Compare the gfx950 code of kernels in the tree with that of a git revision.  Host only: it cross-compiles, nothing runs.

    python tools/kernel_isa_diff.py manus_amd/csrc/fk.hip HEAD k_fk_apply k_fk_backward_terms:'k_fk_backward_t<1>' ...

Each further argument is OLD[:NEW], the kernel's name at the revision and in the tree (NEW = OLD when left out) as the
demangler prints it in front of the argument list: `k_fk_adam`, `k_fk_backward_t<2>`.  A name matches one kernel exactly; a
template's instantiation is named with its arguments.  Both versions are compiled to assembly with the flags of
manus_amd/build.py (device only, `-fPIC` dropped), the revision's from a `git archive` of manus_amd/csrc and include, so its
headers are the revision's too.  Per pair it prints the number of instructions, the number of differing lines after dropping
comments and directives and renumbering the `.LBB` labels, and whether the sequence of fp32 arithmetic opcodes (`v_*_f32`
but compares and conversions) is equal.  The exit status is non-zero on any difference or missing kernel.  Two streams are
compared with each other: no particular instruction is looked for.
"""
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from manus_amd.build import FLAGS, HIPCC  # noqa: E402

HOST_ONLY = {"-fPIC"}
LABEL = re.compile(r"\.LBB\d+_(\d+)")
FP32 = re.compile(r"^(v_(?!cmp|cvt)\w*_f32)(_e32|_e64|_dpp|_sdwa)?$")


def assembly(src):
    out = src + ".s"
    flags = [f for f in FLAGS if f not in HOST_ONLY] + ["--cuda-device-only", "-S"]
    subprocess.check_call([HIPCC] + flags + [src, "-o", out])
    return open(out).read()


def kernels(text):
    """-> {demangled name in front of '(': normalised lines of its body}"""
    bodies, name, body = {}, None, None
    for line in text.splitlines():
        m = re.match(r"^(\w+):", line)
        if name is None and m and (".type\t%s,@function" % m.group(1)) in text:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            bodies[name] = body
            name = None
            continue
        line = line.split(";")[0].strip()
        if not line or (line.startswith(".") and not LABEL.match(line)):
            continue
        body.append(LABEL.sub(r".LBB_\1", line))
    filt = os.path.join(os.path.dirname(os.path.realpath(HIPCC)), "..", "llvm", "bin", "llvm-cxxfilt")
    names = list(bodies)
    plain = subprocess.run([filt if os.path.exists(filt) else "c++filt"] + names, check=True, capture_output=True, text=True).stdout.split("\n")
    return {re.sub(r"^void ", "", d).split("(")[0]: bodies[n] for n, d in zip(names, plain)}


def fp32_ops(body):
    ops = [FP32.match(l.split()[0]) for l in body]
    return [m.group(1) for m in ops if m]


def main(argv):
    if len(argv) < 3:
        print(__doc__)
        return 2
    path, rev, pairs = argv[0], argv[1], [(p.split(":") * 2)[:2] for p in argv[2:]]
    rel = os.path.relpath(os.path.abspath(path), ROOT)
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "manus_amd/csrc", "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        old = kernels(assembly(os.path.join(tmp, rel)))
        for d in (os.path.join("manus_amd", "csrc"), "include"):      # a copy, so that the .s lands outside the tree
            shutil.copytree(os.path.join(ROOT, d), os.path.join(tmp, "tree", d))
        new = kernels(assembly(os.path.join(tmp, "tree", rel)))
    bad = 0
    for a, b in pairs:
        if a not in old or b not in new:
            print("%-28s -> %-28s MISSING (%s: %s; tree: %s)" % (a, b, rev, ", ".join(sorted(old)), ", ".join(sorted(new))))
            bad += 1
            continue
        x, y = old[a], new[b]
        count = lambda body: sum(1 for l in body if not l.endswith(":"))
        differing = sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, x, y, autojunk=False).get_opcodes() if tag != "equal")
        fx, fy = fp32_ops(x), fp32_ops(y)
        print("%-28s -> %-28s instructions %5d / %5d   differing lines %5d   fp32 ops %4d / %4d %s"
              % (a, b, count(x), count(y), differing, len(fx), len(fy), "equal" if fx == fy else "DIFFERENT"))
        bad += differing != 0 or fx != fy
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
