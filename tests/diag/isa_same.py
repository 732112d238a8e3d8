"""Is the device code of a HIP source the same as at another revision?  CPU only: compiles, never launches.

    python tests/diag/isa_same.py REV file.hip [file.hip ...] [--flag=-DX ...]

For every named source of groma_amd/csrc and every build of csrc/build.py VARIANTS, the source is compiled twice with the product's
flags (COMMON, the variant's defines, the source's extra flags from SOURCES, every --flag): once from the tree at REV (`git archive`
of groma_amd/csrc and include into a temporary directory, so REV's headers are used) and once from the working tree.  The gfx950
code object is taken out of each object file (`llvm-objdump --offloading`) and three texts are compared whole:

  * `llvm-objdump -d` without its "file format" line,
  * `llvm-readelf --notes` (kernel names, VGPR / SGPR counts, LDS and scratch sizes, kernel arguments),
  * the sorted list of kernel symbols.

One line per (file, variant, flags): SAME or DIFF (with the texts that differ).  Exit status 1 if any line reads DIFF.
A refactor of a kernel source that is meant to change no instruction is proved by this before any GPU run.
"""
import difflib
import glob
import importlib.util
import os
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.path.join("groma_amd", "csrc")


def _build_module():
    spec = importlib.util.spec_from_file_location("_csrc_build", os.path.join(ROOT, CSRC, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _tool(name):
    """an LLVM binutil: on PATH, or next to the clang that hipcc drives"""
    path = shutil.which(name)
    if path:
        return path
    hipcc = shutil.which("hipcc")
    if hipcc:
        for rel in ("../llvm/bin", "../lib/llvm/bin"):
            cand = os.path.join(os.path.dirname(os.path.realpath(hipcc)), rel, name)
            if os.path.exists(cand):
                return cand
    raise SystemExit(f"isa_same: {name} not found")


def _run(cmd, cwd=None):
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(" ".join(cmd) + "\n" + r.stdout + r.stderr)
    return r.stdout


def _device_texts(src, flags, workdir):
    """compile src into workdir and return {what: text} of its gfx950 code object"""
    os.makedirs(workdir)
    obj = os.path.join(workdir, "unit.o")
    _run(["hipcc"] + flags + ["-c", src, "-o", obj])
    _run([_tool("llvm-objdump"), "--offloading", obj], cwd=workdir)
    cos = glob.glob(obj + ".*amdgcn*")
    if not cos:  # a unit without kernels in this build (decode.hip in the pair build)
        return {"disassembly": [], "notes": [], "kernels": []}
    if len(cos) != 1:
        raise RuntimeError(f"{src}: expected one device code object, found {cos}")
    disasm = _run([_tool("llvm-objdump"), "-d", cos[0]]).splitlines()
    disasm = [l for l in disasm if "file format" not in l]
    notes = _run([_tool("llvm-readelf"), "--notes", cos[0]]).splitlines()
    syms = []
    for l in _run([_tool("llvm-readelf"), "--symbols", "--wide", cos[0]]).splitlines():
        f = l.split()
        if len(f) == 8 and f[7].endswith(".kd"):  # one kernel descriptor per kernel
            syms.append(f[7][:-3])
    return {"disassembly": disasm, "notes": notes, "kernels": sorted(set(syms))}  # (.symtab and .dynsym list each)


def main(argv):
    flags = [a[len("--flag="):] for a in argv if a.startswith("--flag=")]
    pos = [a for a in argv if not a.startswith("--")]
    if len(pos) < 2 or len(flags) + len(pos) != len(argv):
        raise SystemExit(__doc__)
    rev, files = pos[0], [os.path.basename(f) for f in pos[1:]]
    b = _build_module()
    for f in files:
        if f not in b.SOURCES:
            raise SystemExit(f"isa_same: {f} is not in csrc/build.py SOURCES")
    sha = _run(["git", "rev-parse", "--short", rev], cwd=ROOT).strip()
    with tempfile.TemporaryDirectory(prefix="isa_same_") as tmp:
        old = os.path.join(tmp, "rev")
        os.makedirs(old)
        ar = subprocess.Popen(["git", "archive", rev, CSRC, "include"], cwd=ROOT, stdout=subprocess.PIPE)
        subprocess.run(["tar", "-x", "-C", old], stdin=ar.stdout, check=True)
        if ar.wait() != 0:
            raise SystemExit(f"isa_same: git archive {rev} failed")
        jobs = []
        for f in files:
            for suffix, defs, _ in b.VARIANTS:
                fl = b.COMMON + defs + b.SOURCES[f] + flags
                tag = f.replace(".hip", suffix)
                jobs.append((f, suffix, os.path.join(old, CSRC, f), fl, os.path.join(tmp, "o_rev_" + tag)))
                jobs.append((f, suffix, os.path.join(ROOT, CSRC, f), fl, os.path.join(tmp, "o_new_" + tag)))
        with ThreadPoolExecutor(max_workers=min(os.cpu_count() or 8, 16)) as ex:
            texts = list(ex.map(lambda j: _device_texts(j[2], j[3], j[4]), jobs))
    print(f"# device code of the working tree against {rev} ({sha}); flags beyond the product's: {' '.join(flags) or 'none'}")
    bad = 0
    for i in range(0, len(jobs), 2):
        f, suffix = jobs[i][0], jobs[i][1]
        a, c = texts[i], texts[i + 1]
        differ = [k for k in a if a[k] != c[k]]
        bad += bool(differ)
        n = len(c["kernels"])
        print(f"{'DIFF' if differ else 'SAME'}  {f:<16} {'lib' + suffix:<8} {' '.join(flags):<14} {n} kernels, {len(c['disassembly'])} lines"
              + (": " + ", ".join(differ) if differ else ""))
        for k in differ:
            d = list(difflib.unified_diff(a[k], c[k], rev, "working tree", lineterm="", n=1))
            print("\n".join("    " + l for l in d[:40]))
            if len(d) > 40:
                print(f"    ... {len(d) - 40} more lines")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
