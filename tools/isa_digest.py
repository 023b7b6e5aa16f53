#!/usr/bin/env python3
"""Compare the gfx950 code of the library between a git revision and the working tree, kernel by kernel.

A device function whose instruction stream and kernel descriptor (.amdhsa_*: VGPRs, SGPRs, LDS, scratch) are
byte-identical to the other side's runs exactly as fast, so a refactor of the kernel source is checked here on a
machine without a GPU:

    python tools/isa_digest.py [REV]      # REV defaults to HEAD, or to HEAD~1 when csrc/ and include/ are clean

Both sides are compiled with the flags of their own csrc/Makefile plus -save-temps, each into a temporary directory
outside the tree (csrc/liblgconv_hip.so is never touched).  Per function symbol of every device .s file: the lines
between `symbol:` and `.Lfunc_end*`, without `;` comments and .p2align / .cfi* / .loc / .file lines, local labels
stripped of their per-function index (.LBB12_3 -> .LBB_3), plus the symbol's .amdhsa_kernel block, hashed.  Several
translation units are merged by symbol name.  Prints the symbols only one side has and, for every symbol whose digest
differs, the demangled name, both instruction counts and the descriptor lines that differ.  Exit status 0 only if the
two tables are equal.  --keep DIR keeps the two build directories (DIR/ref, DIR/new) for a closer look at the .s files.
"""
import argparse
import concurrent.futures
import glob
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("gnn-ecommerce_amd", "csrc")
MAX_JOBS = 16

_LOCAL_LABEL = re.compile(r"\.L([A-Za-z_]+?)\d+(_\d+)?\b")
_DROPPED = (".p2align", ".cfi", ".loc", ".file")
# what the Makefiles take from the environment besides HIPCC: an EXTRA or OPT left there would change the flags of one side
# only (a revision whose Makefile does not know the variable ignores it), so both sides are asked with these cleared
_MAKE_VARS = ("ARCH", "OPT", "EXTRA", "OUT", "JOBS")


def _run(cmd, cwd):
    proc = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if proc.returncode != 0:
        sys.exit(f"{' '.join(cmd)} failed in {cwd}:\n{proc.stdout}")
    return proc.stdout


def make_var(csrc, name):
    """A variable of the Makefile in `csrc`, as make expands it (works for a Makefile that has no such target)."""
    cmd = ["make", "-s", "--no-print-directory", "--eval", f"isa-digest-print: ; @echo $({name})", "isa-digest-print"]
    env = {k: v for k, v in os.environ.items() if k not in _MAKE_VARS and not k.startswith(("MAKE", "MFLAGS"))}
    proc = subprocess.run(cmd, cwd=csrc, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if proc.returncode != 0:
        sys.exit(f"{' '.join(cmd)} failed in {csrc}:\n{proc.stdout}")
    return proc.stdout.strip().split()


def compile_side(tree, out):
    """Every csrc/*.hip of the source tree `tree` -> device assembly under `out`; returns the .s paths."""
    csrc = os.path.join(tree, CSRC)
    hipcc, flags = make_var(csrc, "HIPCC"), make_var(csrc, "CXXFLAGS")
    sources = sorted(glob.glob(os.path.join(csrc, "*.hip")))
    if not sources:
        sys.exit(f"no .hip source under {csrc}")
    os.makedirs(out, exist_ok=True)
    jobs = []
    for src in sources:
        stem = os.path.splitext(os.path.basename(src))[0]
        jobs.append(hipcc + flags + ["-save-temps", "-c", src, "-o", os.path.join(out, stem + ".o")])
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(MAX_JOBS, os.cpu_count() or 1)) as pool:
        list(pool.map(lambda cmd: _run(cmd, out), jobs))
    return sorted(glob.glob(os.path.join(out, "*-hip-amdgcn-*.s")))


def is_instruction(line):
    return not line.startswith(".") and not line.endswith(":")


def digest_file(path, table):
    """table[symbol] = (sha256, instruction count, descriptor lines) for every function symbol of one .s file."""
    with open(path) as f:
        lines = f.read().split("\n")
    functions = {m.group(1) for m in (re.match(r"\s*\.type\s+(\S+),@function", ln) for ln in lines) if m}
    bodies, descriptors = {}, {}
    current, desc = None, None    # the function whose body is open; the kernel whose descriptor block is open
    for raw in lines:
        line = raw.split(";", 1)[0].strip()
        if desc is not None:      # hipcc puts the block inside symbol: ... .Lfunc_end*, after s_endpgm
            if line == ".end_amdhsa_kernel":
                desc = None
            elif line:
                descriptors[desc].append(line)
        elif line.startswith(".amdhsa_kernel "):
            desc = line.split()[1]
            descriptors[desc] = []
        elif current is None:
            if line.endswith(":") and line[:-1] in functions and line[:-1] not in bodies:
                current = line[:-1]
                bodies[current] = []
        elif re.match(r"\.Lfunc_end\d+:", line):
            current = None
        elif line and not line.startswith(_DROPPED):
            bodies[current].append(_LOCAL_LABEL.sub(lambda m: f".L{m.group(1)}{m.group(2) or ''}", line))
    for sym, body in bodies.items():
        desc = descriptors.get(sym, [])
        sha = hashlib.sha256("\n".join(body + ["--"] + desc).encode()).hexdigest()
        if sym in table and table[sym][0] != sha:
            sys.exit(f"{sym} is defined differently in two translation units of one side ({path})")
        table[sym] = (sha, sum(is_instruction(ln) for ln in body), desc)


def digest_side(tree, out):
    table = {}
    for path in compile_side(tree, out):
        digest_file(path, table)
    return table


def compare(ref, new, rev):
    """The report lines for two digest tables; the last line is the summary, and the only one when they are equal."""
    only_ref, only_new = sorted(set(ref) - set(new)), sorted(set(new) - set(ref))
    changed = sorted(s for s in set(ref) & set(new) if ref[s][0] != new[s][0])
    names = demangle(only_ref + only_new + changed)
    out = [f"only in {rev}: {names[s]}" for s in only_ref] + [f"only in the working tree: {names[s]}" for s in only_new]
    for s in changed:
        out.append(f"changed: {names[s]}: {ref[s][1]} -> {new[s][1]} instructions")
        a, b = ref[s][2], new[s][2]
        out += [f"    {x}  ->  {y.split(None, 1)[-1]}" for x, y in zip(a, b) if x != y]
        if len(a) != len(b):
            out.append(f"    descriptor: {len(a)} -> {len(b)} lines")
    same = len(set(ref) & set(new)) - len(changed)
    out.append(f"{rev}: {len(ref)} device functions, working tree: {len(new)}; {same} equal, {len(changed)} changed, "
               f"{len(only_ref)} missing, {len(only_new)} extra")
    return out


def demangle(symbols):
    if not symbols:
        return {}
    tool = shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin" + os.pathsep + os.environ.get("PATH", "")) or \
        shutil.which("c++filt")
    if tool is None:
        return {s: s for s in symbols}
    out = subprocess.run([tool], input="\n".join(symbols), stdout=subprocess.PIPE, text=True).stdout.split("\n")
    return dict(zip(symbols, out))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("rev", nargs="?", help="revision to compare the working tree against (default: HEAD while csrc/ or include/ has "
                    "uncommitted changes, else HEAD~1)")
    ap.add_argument("--keep", metavar="DIR", help="keep the build directories DIR/ref and DIR/new")
    args = ap.parse_args()
    rev = args.rev
    if rev is None:
        dirty = subprocess.run(["git", "status", "--porcelain", "--", CSRC, "include"], cwd=ROOT, stdout=subprocess.PIPE,
                               text=True).stdout.strip()
        rev = "HEAD" if dirty else "HEAD~1"
    work = os.path.abspath(args.keep) if args.keep else tempfile.mkdtemp(prefix="isa_digest_")
    if os.path.commonpath([work, ROOT]) == ROOT:
        sys.exit("the build directory must lie outside the repository")
    try:
        ref_tree = os.path.join(work, "ref_src")
        shutil.rmtree(ref_tree, ignore_errors=True)
        os.makedirs(ref_tree)
        archive = subprocess.run(["git", "archive", rev, CSRC, "include"], cwd=ROOT, stdout=subprocess.PIPE)
        if archive.returncode != 0:
            sys.exit(f"git archive {rev} failed")
        subprocess.run(["tar", "-x", "-C", ref_tree], input=archive.stdout, check=True)
        with concurrent.futures.ThreadPoolExecutor(max_workers=2) as pool:
            ref_f = pool.submit(digest_side, ref_tree, os.path.join(work, "ref"))
            new_f = pool.submit(digest_side, ROOT, os.path.join(work, "new"))
            ref, new = ref_f.result(), new_f.result()
    finally:
        if not args.keep:
            shutil.rmtree(work, ignore_errors=True)

    report = compare(ref, new, rev)
    print("\n".join(report))
    return 0 if len(report) == 1 else 1


if __name__ == "__main__":
    sys.exit(main())
