"""Device assembly of two trees, kernel by kernel (CPU only: hipcc cross-compiles without a GPU).

    python scripts/isa_ab.py REV          # REV against the working tree
    python scripts/isa_ab.py REV_A REV_B  # two git revisions

Takes oavif_amd/csrc and include of each side into a temporary directory, compiles the three translation units that
hold kernels with the device flags of oavif_amd/build.py plus -S --cuda-device-only, and compares every kernel's text
(its label up to the end of the function, and its kernel descriptor).  Prints each kernel that differs with the change
in its per-opcode counts and exits 1 if there is one: a refactor that means to leave the kernels alone shows it so."""
import collections
import concurrent.futures
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oavif_amd.build import DEVICE_FLAGS, _hipcc  # noqa: E402

UNITS = ("ssimu2_hip.hip", "ssimu2_instrument.hip", "ssimu2_ext.hip")
DIRS = ("oavif_amd/csrc", "include")
MAX_COMPILES = 6


def take_tree(rev, dst):
    """`rev`'s copy of DIRS (None: the working tree's) under dst."""
    if rev is None:
        for d in DIRS:
            shutil.copytree(os.path.join(ROOT, d), os.path.join(dst, d))
        return
    tar = subprocess.run(["git", "-C", ROOT, "archive", rev, *DIRS], check=True, capture_output=True).stdout
    subprocess.run(["tar", "-x", "-C", dst], input=tar, check=True)


def compile_unit(tree, unit):
    # relative paths from inside the tree, so that neither side's text carries its directory
    out = unit + ".s"
    subprocess.run([_hipcc(), *DEVICE_FLAGS, "-S", "--cuda-device-only", "-o", out, os.path.join(DIRS[0], unit)],
                   cwd=tree, check=True)
    with open(os.path.join(tree, out)) as f:
        return f.read()


def kernels(asm):
    """{kernel symbol: its lines}: code from the label to the end of the function, then the descriptor."""
    lines = [s for s in asm.split("\n") if not re.match(r"\s*\.(file|loc|ident)\b", s)]
    found = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M):
        start = next(i for i, s in enumerate(lines) if s.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        d0 = next(i for i, s in enumerate(lines) if s.split() == [".amdhsa_kernel", name])
        d1 = next(i for i in range(d0, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
        found[name] = lines[start:end] + lines[d0:d1]
    return found


def opcodes(lines):
    ops = (s.split()[0] for s in map(str.strip, lines) if s and not s.startswith((";", ".")) and not s.endswith(":"))
    return collections.Counter(ops)


def main(argv):
    if len(argv) not in (1, 2):
        sys.exit(__doc__)
    revs = (argv[0], argv[1] if len(argv) == 2 else None)
    names = [r or "working tree" for r in revs]
    with tempfile.TemporaryDirectory() as tmp:
        trees = [os.path.join(tmp, side) for side in "ab"]
        for rev, tree in zip(revs, trees):
            os.mkdir(tree)
            take_tree(rev, tree)
        with concurrent.futures.ThreadPoolExecutor(MAX_COMPILES) as pool:
            asm = {(t, u): pool.submit(compile_unit, t, u) for t in trees for u in UNITS}
        differing = 0
        for unit in UNITS:
            a, b = (kernels(asm[t, unit].result()) for t in trees)
            diff = [k for k in sorted(a.keys() | b.keys()) if a.get(k) != b.get(k)]
            print(f"{unit}: {len(a)} kernels in {names[0]}, {len(b)} in {names[1]}, {len(diff)} differ")
            for k in diff:
                if k not in a or k not in b:
                    print(f"  {k}: only in {names[k in b]}")
                    continue
                oa, ob = opcodes(a[k]), opcodes(b[k])
                delta = {op: ob[op] - oa[op] for op in sorted(oa.keys() | ob.keys()) if ob[op] != oa[op]}
                print(f"  {k}: " + (" ".join(f"{op}{n:+d}" for op, n in delta.items()) or "same opcode counts, other text"))
            differing += len(diff)
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
