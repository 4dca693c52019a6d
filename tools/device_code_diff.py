r"""Proof that a refactor left the device code alone: compile the device side of every kernel source of two revisions and
compare them kernel by kernel.
    python tools/device_code_diff.py <rev_a> <rev_b> [--only REGEX] [--rename PATTERN=REPLACEMENT ...]
A revision is anything `git archive` takes, or WORKTREE for the files as they are. Sources are niftymatch_amd/csrc/*.hip
(--only: those whose name matches), compiled with the build's FLAGS plus --cuda-device-only -S. Kernels are paired by base
name and template arguments, whatever file or namespace holds them. For every kernel of <rev_a> there must be exactly one in
<rev_b>, with the same
  * instruction stream (labels renumbered in order of appearance, comments dropped, mangled symbol names ignored);
  * kernel descriptor (.amdhsa_* fields) and metadata (register counts, LDS and scratch sizes, both spill counts).
--rename PATTERN=REPLACEMENT (may be repeated) is re.sub(PATTERN, REPLACEMENT, key) on the kernel keys of <rev_b>, nothing else: a
kernel whose template list was shortened can still be paired with its parent, e.g. with <rev_b> the parent
  --rename 'conv_sep_kernel<(\d+), 32, (\w+, \w+, \w+), false>=conv_sep_kernel<\1, \2>'
Prints one verdict per kernel; exit status 1 unless every kernel of <rev_a> is IDENTICAL."""
import argparse, difflib, os, re, shutil, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
from niftymatch_amd import build as B

META = (".vgpr_count", ".sgpr_count", ".agpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
        ".vgpr_spill_count", ".sgpr_spill_count")


def checkout(rev, dst):
    """niftymatch_amd/ and include/ of the revision under dst (the sources include ../../include/nm_abi.h)"""
    if rev == "WORKTREE":
        for d in ("niftymatch_amd/csrc", "niftymatch_amd/nm", "include"):
            shutil.copytree(os.path.join(root, d), os.path.join(dst, d))
    else:
        tar = subprocess.run(["git", "-C", root, "archive", rev, "niftymatch_amd/csrc", "niftymatch_amd/nm", "include"],
                             check=True, stdout=subprocess.PIPE).stdout
        subprocess.run(["tar", "-x", "-C", dst], input=tar, check=True)
    return os.path.join(dst, "niftymatch_amd", "csrc")


def device_asm(src):
    out = src + ".s"
    r = subprocess.run([B.HIPCC] + B.FLAGS + ["--cuda-device-only", "-S", src, "-o", out], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for %s:\n%s" % (src, r.stderr))
    with open(out) as f:
        return f.read()


def demangle(names):
    filt = os.path.join(os.path.dirname(os.path.realpath(B.HIPCC)), "..", "llvm", "bin", "llvm-cxxfilt")
    filt = filt if os.path.exists(filt) else "c++filt"
    out = subprocess.run([filt], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.split("\n")))


def kernel_key(demangled):
    """base name + template arguments: 'void ns::(anonymous namespace)::f<2, true>(args)' -> 'f<2, true>'"""
    s = demangled.replace("(anonymous namespace)::", "")
    depth, start, colon = 0, 0, 0
    for i, ch in enumerate(s):
        if ch == "<": depth += 1
        elif ch == ">": depth -= 1
        elif depth == 0 and ch == " ": start = colon = i + 1
        elif depth == 0 and ch == ":": colon = i + 1
        elif depth == 0 and ch == "(": return s[max(start, colon):i]
    return s[max(start, colon):]


def normalise(body):
    labels, out = {}, []
    for line in body.split("\n"):
        line = line.split(";")[0].rstrip()
        if not line.strip(): continue
        line = re.sub(r"\.L[A-Za-z_]+\d+(_\d+)?", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), line)
        out.append(re.sub(r"\b_Z\w+", "SYM", line))
    return out


def kernels_of(asm):
    """mangled name -> (instruction lines, descriptor lines, metadata fields)"""
    res = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", asm, re.M | re.S):
        name = m.group(1)
        begin = asm.index("\n%s:" % name) + len(name) + 2
        end = asm.rindex(".section", begin, m.start())
        res[name] = [normalise(asm[begin:end]), sorted(l.strip() for l in m.group(2).split("\n") if l.strip()), {}]
    meta = asm[asm.index("amdhsa.kernels:"):asm.index(".end_amdgpu_metadata")]
    for entry in re.split(r"^  - ", meta, flags=re.M)[1:]:
        fields = dict(re.findall(r"^\s*(\.\w+):\s+(\S+)$", entry, re.M))
        if ".name" in fields: res[fields[".name"]][2] = {k: fields.get(k) for k in META}      # (amdhsa.version's list follows)
    return res


def collect(rev, only, renames=()):
    tmp = tempfile.mkdtemp(prefix="devdiff_")
    try:
        csrc = checkout(rev, tmp)
        srcs = sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hip") and re.search(only, f))
        with ThreadPoolExecutor(max_workers=8) as ex:
            asms = list(ex.map(device_asm, srcs))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    found = {}
    for src, asm in zip(srcs, asms):
        ks = kernels_of(asm)
        names = demangle(list(ks)) if ks else {}
        for mangled, parts in ks.items():
            key = kernel_key(names[mangled])
            for pattern, replacement in renames: key = re.sub(pattern, replacement, key)
            found.setdefault(key, []).append((os.path.basename(src), parts))
    return found


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("rev_a"); ap.add_argument("rev_b")
    ap.add_argument("--only", default="", help="regex on the source file names")
    ap.add_argument("--diff", action="store_true", help="print the first differing instruction lines")
    ap.add_argument("--rename", action="append", default=[], metavar="PATTERN=REPLACEMENT", help="regex substitution on the kernel keys of rev_b")
    a = ap.parse_args()
    A, Bk = collect(a.rev_a, a.only), collect(a.rev_b, a.only, [r.split("=", 1) for r in a.rename])
    bad = 0
    for key in sorted(A):
        for file_a, pa in A[key]:
            cands = [c for c in Bk.get(key, [])]
            # a name that several files of <rev_a> define (file-local kernels) is paired within the file of the same name
            if len(A[key]) > 1: cands = [c for c in cands if c[0] == file_a]
            if len(cands) != 1:
                verdict = "MISSING" if not cands else "AMBIGUOUS (%d candidates)" % len(cands)
            else:
                file_b, pb = cands[0]
                what = [n for n, x, y in zip(("instructions", "descriptor", "metadata"), pa, pb) if x != y]
                verdict = "IDENTICAL" if not what else "DIFFERS: " + ", ".join(what)
                verdict += "  (%d instructions; %s -> %s)" % (len([l for l in pa[0] if not l.endswith(":")]), file_a, file_b)
                if what and a.diff:
                    verdict += "\n" + "\n".join(list(difflib.unified_diff(pa[0] + pa[1], pb[0] + pb[1], lineterm="", n=1))[:40])
            bad += not verdict.startswith("IDENTICAL")
            print("%-48s %s" % (key, verdict))
    new = sorted(k for k in Bk if k not in A)
    if new: print("only in %s: %s" % (a.rev_b, ", ".join(new)))
    print("%d kernels of %s compared, %d not identical" % (sum(len(v) for v in A.values()), a.rev_a, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
