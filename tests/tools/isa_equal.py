"""Do two checkouts compile to the same gfx950 device code?  For a change that claims to touch device SOURCE only (helpers moved
between headers, copies folded into one function): every translation unit of csrc/Makefile's OBJS is compiled device-only to assembly
in both trees with the Makefile's flags (FLAGS_<unit> included), and per kernel symbol the instruction text (labels included) and the
`.amdhsa_*` descriptor block are compared. Assembler comments are dropped; the function index of local labels (`.LBB<n>_`: emission
order) and the `__hip_cuid_<hash>` name (a hash of the source path) are masked. No GPU needed: hipcc cross-compiles.

usage: python3 tests/tools/isa_equal.py <tree A> <tree B> [--jobs N] [--out DIR] [--reuse-a] [--only unit ...]
  --out DIR   keep the assembly files there (DIR/a/<unit>.s, DIR/b/<unit>.s; default: a temporary directory)
  --reuse-a   do not recompile a unit of tree A whose DIR/a/<unit>.s exists (tree A = a fixed parent commit, compiled once)
Exit status 0: same kernel symbols, no differing kernel."""
import argparse
import concurrent.futures
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_hazards import device_asm, kernels  # noqa: E402

_MASKS = ((re.compile(r"\.LBB\d+_"), ".LBB_"), (re.compile(r"__hip_cuid_[0-9a-f]+"), "__hip_cuid_"))
_IN_DEVICE_ASM = {"-O3", "-std=c++17", "-MMD", "-MP", "$(EXTRA)"}          # device_asm's own flags; dependency files and EXTRA: not wanted


def makefile_units(tree):
    """[(unit, [flags beyond device_asm's own])] from csrc/Makefile: OBJS, CXXFLAGS and the per-unit FLAGS_<unit>."""
    var = {}
    with open(os.path.join(tree, "pytorchcv_amd", "csrc", "Makefile")) as f:
        for line in f:
            m = re.match(r"^(\w+)\s*\??=\s*(.*)$", line)
            if m:
                var[m.group(1)] = m.group(2).strip()
    common = [w for w in var["CXXFLAGS"].split() if w not in _IN_DEVICE_ASM and not w.startswith("--offload-arch")]
    return [(o[:-2], common + var.get("FLAGS_" + o[:-2], "").split()) for o in var["OBJS"].split()]


def kernel_texts(asm):
    """{kernel symbol: (body lines: instructions and labels, descriptor lines)} with comments dropped and the masks applied."""
    def norm(s):
        s = s.split(";")[0].split("//")[0].strip()
        for rx, to in _MASKS:
            s = rx.sub(to, s)
        return " ".join(s.split())
    syms = set(kernels(asm))
    body, desc, cur, dcur = {}, {}, None, None
    for line in asm.split("\n"):
        m = re.match(r"^(_Z\w+):", line)
        if m and m.group(1) in syms:
            cur = body.setdefault(m.group(1), [])
            continue
        s = norm(line)
        if s.startswith(".amdhsa_kernel "):
            dcur = desc.setdefault(s.split()[1], [])
        elif s.startswith(".end_amdhsa_kernel"):
            dcur = None
        elif dcur is not None and s:
            dcur.append(s)
        if cur is not None:
            if s.startswith((".section", ".end_amdhsa_kernel")) or re.match(r"^\.Lfunc_end", s):
                cur = None
            elif s and (not s.startswith(".") or s.endswith(":")) and "ASMSTART" not in line and "ASMEND" not in line:
                cur.append(s)
    return {k: (body[k], desc.get(k, [])) for k in syms}


def compile_unit(tree, unit, flags, out, reuse):
    if not (reuse and os.path.exists(out)):
        device_asm(os.path.join(tree, "pytorchcv_amd", "csrc", unit + ".hip"), out, flags)
    with open(out) as f:
        return kernel_texts(f.read())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--out")
    ap.add_argument("--reuse-a", action="store_true")
    ap.add_argument("--only", nargs="*")
    a = ap.parse_args()
    out = a.out or tempfile.mkdtemp(prefix="isa_equal_")
    for side in "ab":
        os.makedirs(os.path.join(out, side), exist_ok=True)
    ua, ub = makefile_units(a.tree_a), makefile_units(a.tree_b)
    if ua != ub:
        print("the two Makefiles differ in OBJS or flags:\n  {}\n  {}".format(ua, ub))
        return 1
    units = [u for u in ub if not a.only or u[0] in a.only]
    with concurrent.futures.ThreadPoolExecutor(a.jobs) as ex:
        fa = {u: ex.submit(compile_unit, a.tree_a, u, fl, os.path.join(out, "a", u + ".s"), a.reuse_a) for u, fl in units}
        fb = {u: ex.submit(compile_unit, a.tree_b, u, fl, os.path.join(out, "b", u + ".s"), False) for u, fl in units}
        bad = total = 0
        for u, _ in units:
            ka, kb = fa[u].result(), fb[u].result()
            only = sorted(set(ka) ^ set(kb))
            differ = sorted(k for k in set(ka) & set(kb) if ka[k] != kb[k])
            total += len(kb)
            bad += len(only) + len(differ)
            print("{:12s} {:4d} / {:4d} kernels, {} only on one side, {} differ".format(u, len(ka), len(kb), len(only), len(differ)))
            for k in only:
                print("    only in {}: {}".format("A" if k in ka else "B", k))
            for k in differ:
                what = [n for n, i in (("instructions", 0), ("descriptor", 1)) if ka[k][i] != kb[k][i]]
                first = next((i for i, (x, y) in enumerate(zip(ka[k][0], kb[k][0])) if x != y), min(len(ka[k][0]), len(kb[k][0])))
                print("    differs ({}; {} / {} lines, first at {}): {}".format(", ".join(what), len(ka[k][0]), len(kb[k][0]), first, k))
    print("{} units, {} kernels, {} differing or unmatched (assembly kept in {})".format(len(units), total, bad, out))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
