"""Compare the generated gfx950 code of two source trees, kernel by kernel.

    python tools/isa_compare.py dump OUTDIR          # compile this tree's kernel sources to OUTDIR/*.s
    python tools/isa_compare.py compare DIR_A DIR_B  # per kernel: metadata equal? instruction stream identical?

`compare` counts as a difference: a kernel whose metadata or instruction stream differs, a kernel symbol on one side only, a
source file present in A only.  A source file present in B only (a source B added) is listed as "new in B" with its kernel
count and NOT counted; `dump` skips product sources the tree does not have (an older tree).
`dump` uses the command of tests/test_codegen_cpu.py (build.FLAGS without -fPIC, -S --cuda-device-only), once plain
for the product sources -- build.SOURCES of the tree it lies in, without the host layer -- and once with
-DSQLLM_ABLATION_BUILD for those and the kernel sources of the measurement library.
To dump a commit that does not have this script yet, copy the script into that tree's tools/ first (it reads the
sources and the flags of the tree it lies in).
"""
import collections
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from squeezellm_amd import build as B  # noqa: E402

# every kernel source of the product: build.SOURCES without the host layer (its last entry), so that a new kernel file cannot be forgotten
PRODUCT = B.SOURCES[:-1]
assert B.SOURCES[-1] == "sqllm_capi.hip"
META = (".vgpr_count", ".sgpr_count", ".agpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
        ".vgpr_spill_count", ".sgpr_spill_count")
CLASSES = ("v_mfma", "ds_read", "global_load", "buffer_load", "s_load", "s_barrier", "s_waitcnt")


def dump(outdir):
    os.makedirs(outdir, exist_ok=True)
    jobs = [(s, "product", []) for s in PRODUCT]
    # (sqllm_experimental.hip is host code only: no kernels to compare)
    jobs += [(s, "ablation", ["-DSQLLM_ABLATION_BUILD"]) for s in PRODUCT + [e for e in B.EXPERIMENT_SOURCES if "sqllm_experimental" not in e]]
    procs = []
    for src, tag, extra in jobs:
        if not os.path.exists(os.path.join(B.CSRC, src)):  # (an older tree: the source came later)
            continue
        out = os.path.join(outdir, f"{tag}__{os.path.basename(src)}.s")
        cmd = [B.hipcc(), f"--offload-arch={B.ARCH}", *[f for f in B.FLAGS if f != "-fPIC"], *extra, "-S",
               "--cuda-device-only", f"-I{B.INCLUDE}", f"-I{B.CSRC}", f"-I{B.EXPERIMENTAL}", os.path.join(B.CSRC, src), "-o", out]
        procs.append((out, subprocess.Popen(cmd)))
    bad = [o for o, p in procs if p.wait() != 0]
    if bad:
        sys.exit(f"failed: {bad}")


def parse(path):
    """-> {kernel symbol: (metadata dict, normalised instruction list)}"""
    text = open(path).read()
    kernels = set(re.findall(r"^\s+\.amdhsa_kernel\s+(\S+)", text, re.M))
    meta = {}
    for block in text.split("  - .agpr_count:")[1:]:
        block = ".agpr_count:" + block
        name = re.search(r"^\s+\.name:\s+(\S+)", block, re.M).group(1)
        meta[name] = {k: re.search(rf"{re.escape(k)}:\s+(\S+)", block).group(1) for k in META}
    out = {}
    for m in re.finditer(r"^(\w+):.*?^\.Lfunc_end\d+:", text, re.S | re.M):
        if m.group(1) not in kernels:
            continue
        ins = []
        for line in m.group(0).split("\n")[1:]:
            line = re.sub(r"\s*;.*", "", line).strip()
            if not line or line.startswith(".") or line.endswith(":"):
                continue
            ins.append(re.sub(r"\.L\w+", ".L", re.sub(r"\s+", " ", line)))
        out[m.group(1)] = (meta[m.group(1)], ins)
    # every kernel the file declares has a body and metadata here, and there is at least one: never succeed on nothing
    assert kernels and set(out) == kernels, f"{path}: declared {len(kernels)} kernels, parsed {len(out)}"
    assert all(len(md) == len(META) for md, _ in out.values()), path
    return out


def classes(ins):
    c = collections.Counter()
    for i in ins:
        for k in CLASSES:
            if i.startswith(k):
                c[k] += 1
    return dict(c)


def compare(a, b):
    same = diff = 0
    lines = []
    for f in sorted(set(os.listdir(a)) | set(os.listdir(b))):
        if not f.endswith(".s"):
            continue
        pa, pb = os.path.join(a, f), os.path.join(b, f)
        if os.path.exists(pb) and not os.path.exists(pa):  # a source B added: nothing to compare it with
            lines.append(f"{f}: new in B, {len(parse(pb))} kernels (not compared)")
            continue
        if not os.path.exists(pb):
            lines.append(f"{f}: present in A only")
            diff += 1
            continue
        ka, kb = parse(pa), parse(pb)
        if set(ka) != set(kb):
            lines.append(f"{f}: kernel symbols differ: only A {sorted(set(ka) - set(kb))} only B {sorted(set(kb) - set(ka))}")
            diff += 1
        n_id = 0
        for k in sorted(set(ka) & set(kb)):
            (ma, ia), (mb, ib) = ka[k], kb[k]
            if ma == mb and ia == ib:
                n_id += 1
                continue
            diff += 1
            lines.append(f"{f}: {k}: DIFFERENT")
            if ma != mb:
                lines.append(f"    metadata A {ma}\n    metadata B {mb}")
            lines.append(f"    instructions A {len(ia)} B {len(ib)}; classes A {classes(ia)} B {classes(ib)}")
        same += n_id
        lines.append(f"{f}: {len(ka)} kernels, {n_id} identical (metadata and instruction stream)")
    print("\n".join(lines))
    print(f"SUMMARY: {same} kernels identical, {diff} differences")
    return 1 if diff else 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
