"""Device assembly of two trees, kernel by kernel (CPU only: hipcc cross-compiles without a GPU).

    python scripts/isa_ab.py REV          # REV against the working tree
    python scripts/isa_ab.py REV_A REV_B  # two git revisions

Takes oavif_amd/csrc and include of each side into a temporary directory, compiles the translation units that hold
kernels (those of UNITS a side has) with the device flags of oavif_amd/build.py plus -S --cuda-device-only, and compares
every kernel's text (its label up to the end of the function, and its kernel descriptor) by the kernel's name across all
units of a side: a kernel that moved to another unit with the same text is unchanged.  Local labels carry the number
of their function within its unit, which a move changes and which is taken out.  Prints each kernel that differs with
the change in its per-opcode counts, each kernel that one side defines in two units with different text, and exits 1
if there is either: a refactor that means to leave the kernels alone shows it so."""
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

UNITS = ("ssimu2_hip.hip", "ssimu2_instrument.hip", "ssimu2_ext.hip", "ssimu2_yuv.hip", "ssimu2_map.hip",
         "ssimu2_chroma.hip", "ssimu2_yuva.hip", "ssimu2_rbatch.hip", "ssimu2_hbatch.hip", "ssimu2_abatch.hip")
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
        # BB<function>_<block> in labels and comments, and the padding behind a label: the function's number within its
        # unit is not the kernel's text
        found[name] = [re.sub(r"\s+", " ", re.sub(r"BB\d+_", "BB_", s)) for s in lines[start:end] + lines[d0:d1]]
    return found


def side_kernels(name, by_unit):
    """{kernel: its lines} over every unit of one side, {kernel: its units}, and the kernels whose text differs between
    two units of that side (reported)."""
    text, where, clashes = {}, collections.defaultdict(list), 0
    for unit, found in by_unit.items():
        for k, lines in found.items():
            where[k].append(unit)
            if text.setdefault(k, lines) != lines:
                clashes += 1
                print(f"  {k}: {name} defines it in {where[k][0]} and, with other text, in {unit}")
    return text, where, clashes


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
        units = [[u for u in UNITS if os.path.exists(os.path.join(t, DIRS[0], u))] for t in trees]
        with concurrent.futures.ThreadPoolExecutor(MAX_COMPILES) as pool:
            asm = [{u: pool.submit(compile_unit, t, u) for u in us} for t, us in zip(trees, units)]
        sides = [side_kernels(n, {u: kernels(job.result()) for u, job in jobs.items()}) for n, jobs in zip(names, asm)]
        (a, where_a, clash_a), (b, where_b, clash_b) = sides
        for n, where in zip(names, (where_a, where_b)):
            per_unit = collections.Counter(u for us in where.values() for u in us)
            print(f"{n}: {len(where)} kernels (" + ", ".join(f"{u} {per_unit[u]}" for u in UNITS if per_unit[u]) + ")")
            shared = collections.Counter(" and ".join(us) for us in where.values() if len(us) > 1)
            for us, count in shared.items():  # compiled more than once on that side
                print(f"  {count} kernel{'s'[:count != 1]} in {us}")
        diff = [k for k in sorted(a.keys() | b.keys()) if a.get(k) != b.get(k)]
        moved = sorted(k for k in a.keys() & b.keys() if a[k] == b[k] and sorted(where_a[k]) != sorted(where_b[k]))
        print(f"{len(diff)} kernels differ; {len(moved)} have the same text in other units")
        moves = collections.defaultdict(list)
        for k in moved:
            moves[f"{', '.join(where_a[k])} -> {', '.join(where_b[k])}"].append(k)
        for move, ks in moves.items():
            print(f"  {move}: " + (" ".join(ks) if len(ks) <= 5 else f"{len(ks)} kernels"))
        for k in diff:
            if k not in a or k not in b:
                print(f"  {k}: only in {names[k in b]}")
                continue
            oa, ob = opcodes(a[k]), opcodes(b[k])
            delta = {op: ob[op] - oa[op] for op in sorted(oa.keys() | ob.keys()) if ob[op] != oa[op]}
            print(f"  {k}: " + (" ".join(f"{op}{n:+d}" for op, n in delta.items()) or "same opcode counts, other text"))
        differing = len(diff) + clash_a + clash_b
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
