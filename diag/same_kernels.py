#!/usr/bin/env python3
"""Do the kernels of the working tree compile to the same code objects as at another commit?  No GPU needed.

    diag/same_kernels.py [REV] [--kernels REGEX] [--files REGEX] [-j N] [-- EXTRA HIPCC FLAGS]

Exports REV (default HEAD) to a temporary directory, compiles every .hip file of flo_amd/csrc at both trees device-only
to assembly with the Makefile's DEVFLAGS (plus the extra flags, e.g. -DFLO_STAMPS -DFLO_MARKS), and compares per kernel
symbol from its label through .end_amdhsa_kernel: the instructions and the descriptor (VGPRs, SGPRs, LDS, scratch).
Before comparing, comments (; to the end of the line) and empty lines are dropped and the function index is taken out of
.LBB<n>_ and .Lfunc_end<n>, so a kernel that merely moved inside its file, or to another file, compares equal.
Exit status 0: same set of kernel symbols, every kernel equal.  --kernels narrows both to the symbols REGEX finds.
"""
import argparse
import concurrent.futures
import pathlib
import re
import subprocess
import sys
import tempfile

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = pathlib.Path("flo_amd") / "csrc"


def devflags(tree):
    mk = (tree / CSRC / "Makefile").read_text()
    var = lambda name: re.search(rf"^{name}\s*[:?]?=\s*(.*)$", mk, re.M).group(1)
    hipcc = var("HIPCC").replace("$(ROCM)", var("ROCM"))
    return hipcc, var("DEVFLAGS").replace("$(ARCH)", var("ARCH")).split()


def compile_asm(tree, hip, out, extra):
    hipcc, flags = devflags(tree)
    r = subprocess.run([hipcc, *flags, *extra, "--cuda-device-only", "-S", hip.name, "-o", str(out)],
                       cwd=tree / CSRC, capture_output=True, text=True)
    if r.returncode:
        sys.exit(f"{tree / CSRC / hip.name}: does not compile\n{r.stderr}")
    return out


def kernels(asm):
    """{symbol: normalised lines from its label through .end_amdhsa_kernel}"""
    lines = asm.read_text().splitlines()
    label = {m.group(1): i for i, l in enumerate(lines) if (m := re.match(r"([A-Za-z_$][\w$.]*):", l))}
    found = {}
    for i, l in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if not m:
            continue
        end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
        body = []
        for t in lines[label[m.group(1)]:end + 1]:
            t = t.split(";", 1)[0].rstrip()
            t = re.sub(r"\.LBB\d+_", ".LBB_", t)
            t = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", t)
            if t.strip():
                body.append(t)
        found[m.group(1)] = body
    return found


def main():
    argv, extra = sys.argv[1:], []
    if "--" in argv:
        extra = argv[argv.index("--") + 1:]
        argv = argv[:argv.index("--")]
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("rev", nargs="?", default="HEAD")
    ap.add_argument("--kernels", default="", help="compare only the kernel symbols this regex finds")
    ap.add_argument("--files", default="", help="compile only the .hip files this regex finds")
    ap.add_argument("-j", type=int, default=8)
    a = ap.parse_args(argv)

    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        old = tmp / "old"
        old.mkdir()
        tar = subprocess.run(["git", "-C", str(ROOT), "archive", a.rev, str(CSRC), "include"], capture_output=True, check=True)
        subprocess.run(["tar", "-x", "-C", str(old)], input=tar.stdout, check=True)
        sides = {"old": old, "new": ROOT}
        names = {s: sorted(p.name for p in (t / CSRC).glob("*.hip") if re.search(a.files, p.name)) for s, t in sides.items()}
        with concurrent.futures.ThreadPoolExecutor(a.j) as pool:
            jobs = {(s, n): pool.submit(compile_asm, sides[s], pathlib.Path(n), tmp / f"{s}_{n}.s", extra)
                    for s in sides for n in names[s]}
            got = {s: {} for s in sides}
            for (s, n), job in jobs.items():
                for sym, body in kernels(job.result()).items():
                    if re.search(a.kernels, sym):
                        got[s][sym] = body

    bad = 0
    for sym in sorted(set(got["old"]) ^ set(got["new"])):
        print(f"ONLY IN {'old' if sym in got['old'] else 'new'}: {sym}")
        bad += 1
    both = sorted(set(got["old"]) & set(got["new"]))
    for sym in both:
        o, n = got["old"][sym], got["new"][sym]
        if o != n:
            at = next((i for i, (x, y) in enumerate(zip(o, n)) if x != y), min(len(o), len(n)))
            print(f"DIFFERS: {sym}: {len(o)} -> {len(n)} lines, first at line {at}:")
            print(f"    old: {o[at].strip() if at < len(o) else '(end)'}")
            print(f"    new: {n[at].strip() if at < len(n) else '(end)'}")
            bad += 1
    flags = " ".join(extra) or "(none)"
    print(f"{len(both)} kernels compared against {a.rev}, extra flags {flags}: "
          + ("all equal, same set of symbols" if not bad else f"{bad} NOT EQUAL"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
