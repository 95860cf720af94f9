"""What the LDS-path kernels compile to, kernel by kernel (no GPU needed): the three units of lds_kernels.h (lds_launch.hip,
lds_launch_ps.hip, lds_launch_pp.hip) compiled to gfx950 assembly as tools/spill_table.py compiles them, and of every
k_admm_lds / k_admm_lds_ps / k_admm_lds_pp instance one record: unit, name, sha256 of its instructions and the registers,
spills and scratch of its descriptor.  tests/golden/lds_kernel_isa.json is the manifest of the committed tree, and
tests/test_lds_adapt_cpu.py compares the tree under test with it.

    python tools/kernel_isa.py                        # write tests/golden/lds_kernel_isa.json from this tree
    python tools/kernel_isa.py TREE -o FILE           # ... the manifest of another checkout, to FILE
    python tools/kernel_isa.py A B                    # the kernels that differ between two manifests or two trees

A kernel's text runs from its label to .Lfunc_end.  Comments are dropped, and the labels that carry the number of the function
within its file (.LBBn_m, .Lfunc_endn, ...) lose that number, so a kernel that only moved within its unit keeps its hash.
"""
import argparse, hashlib, json, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from spill_table import HIPCC, LDS_UNITS, ROOT, compile_asm, demangle, descriptors      # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "lds_kernel_isa.json")
COLUMNS = ("vgpr", "vgpr_spill", "sgpr_spill", "scratch")


def hipcc_version():
    return subprocess.run([HIPCC, "--version"], capture_output=True, text=True, check=True).stdout.splitlines()[0].strip()


def kernel_text(body):
    """The text of one function that is hashed: no comments, no blank lines, no function numbers in local labels."""
    out = []
    for line in body.splitlines():
        line = line.split(";", 1)[0].rstrip()
        if line.strip():
            out.append(re.sub(r"\.L(BB|JTI|func_begin|func_end|tmp)\d+", r".L\1", line))
    return "\n".join(out) + "\n"


def records(unit, asm_text):
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", asm_text, re.M | re.S)}
    desc = descriptors(asm_text)
    names = demangle([d[0] for d in desc])
    out = []
    for mangled, scratch, sspill, vgpr, vspill in desc:
        name = re.sub(r"\s+", " ", names[mangled]).split("(")[0].replace("void ", "")
        if name.startswith("k_admm_lds"):
            out.append({"unit": unit, "kernel": name, "sha256": hashlib.sha256(kernel_text(bodies[mangled]).encode()).hexdigest(),
                        "vgpr": int(vgpr), "vgpr_spill": int(vspill), "sgpr_spill": int(sspill), "scratch": int(scratch)})
    return out


def manifest(root=ROOT):
    """The manifest of the source tree at `root`: the three units compile side by side."""
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(len(LDS_UNITS)) as pool:
        texts = list(pool.map(lambda tu: compile_asm(tu, os.path.join(tmp, tu + ".s"), root), LDS_UNITS))
    recs = [r for tu, text in zip(LDS_UNITS, texts) for r in records(tu, text)]
    return {"hipcc": hipcc_version(), "kernels": sorted(recs, key=lambda r: (r["unit"], r["kernel"]))}


def load(path):
    return manifest(path) if os.path.isdir(path) else json.load(open(path))


def difference(a, b):
    """Lines that name the records of manifests a and b that differ; none when the two are equal."""
    ka, kb = ({(r["unit"], r["kernel"]): r for r in m["kernels"]} for m in (a, b))
    lines = []
    for key in sorted(set(ka) | set(kb)):
        ra, rb = ka.get(key), kb.get(key)
        if ra != rb:
            cols = "  ".join(f"{c} {ra[c] if ra else '-'}->{rb[c] if rb else '-'}" for c in COLUMNS)
            what = "only in A" if rb is None else "only in B" if ra is None else "text differs" if ra["sha256"] != rb["sha256"] else "registers differ"
            lines.append(f"{key[0]:18s} {key[1]:58s} {what:16s} {cols}")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("trees", nargs="*", help="one source tree: write its manifest; two manifests or trees: compare them")
    ap.add_argument("-o", "--out", default=None, help="where the manifest goes (default: tests/golden/lds_kernel_isa.json of this tree)")
    args = ap.parse_args()
    if len(args.trees) == 2:
        a, b = (load(p) for p in args.trees)
        lines = difference(a, b)
        print(f"# A = {args.trees[0]} ({a['hipcc']})  B = {args.trees[1]} ({b['hipcc']})")
        print("\n".join(lines + [f"# {len(a['kernels'])} | {len(b['kernels'])} kernels, {len(lines)} differ"]))
        return 1 if lines else 0
    m = manifest(args.trees[0] if args.trees else ROOT)
    out = args.out or GOLDEN
    with open(out, "w") as f:
        json.dump(m, f, indent=0)
        f.write("\n")
    print(f"{out}: {len(m['kernels'])} kernels, {m['hipcc']}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
