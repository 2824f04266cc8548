"""Guards on the generated gfx950 code of the column-lane kernel's ONE-ROW instantiations (csrc/sqllm_kernels.hip: dense_role_cols,
BT == 1; hipcc cross-compiles without a GPU): four 8-wave workgroups per CU (<= 64 VGPRs), no scratch, and in the decode loops at
most one full drain of the LDS / scalar-load counter (s_waitcnt lgkmcnt(0)) per 32 weights -- the other waits are counted ones."""
import os
import re
import shutil
import subprocess

import pytest

from squeezellm_amd import build as B

PREFIX = "_ZN5sqllm16sqllm_fused_colsILi"


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("asm_cols1") / "k.s"
    cmd = [hipcc, f"--offload-arch={B.ARCH}", *[f for f in B.FLAGS if f != "-fPIC"], "-S", "--cuda-device-only",
           f"-I{B.INCLUDE}", f"-I{B.CSRC}", os.path.join(B.CSRC, "sqllm_kernels.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True)
    return out.read_text()


def _batch1_bodies(asm):
    out = {}
    for m in re.finditer(r"^(" + PREFIX + r"[34]ELi1ELi8E\w+):.*?^\.Lfunc_end", asm, re.S | re.M):
        out[m.group(1)] = m.group(0).split("\n")
    return out


def _loops(body):
    """(start, end) line ranges of the backward branches of a kernel body."""
    labels = {l.split(":")[0]: i for i, l in enumerate(body) if l.startswith(".LBB")}
    out = []
    for i, l in enumerate(body):
        m = re.search(r"s_cbranch_\w+ (\.LBB\S+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            out.append((labels[m.group(1)], i))
    return out


def test_batch1_occupancy_and_no_scratch(asm):
    meta = re.findall(r"\.name:\s+(" + PREFIX + r"[34]ELi1ELi8E\w+).*?\.private_segment_fixed_size:\s+(\d+).*?"
                      r"\.sgpr_spill_count:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", asm, re.S)
    assert len(meta) == 2
    for name, scratch, sspill, vgpr, vspill in meta:
        assert int(scratch) == 0 and int(vspill) == 0 and int(sspill) == 0, (name, scratch, sspill, vspill)
        assert int(vgpr) <= 64, (name, vgpr)


def test_batch1_decode_loops_drain_once_per_32_weights(asm):
    ks = _batch1_bodies(asm)
    assert len(ks) == 2
    for name, body in ks.items():
        # innermost decode loops: a loop with packed FMAs that contains no other such loop
        dec = [(a, b) for a, b in _loops(body) if any(re.match(r"\s+v_pk_fma_f32", l) for l in body[a:b])]
        inner = [(a, b) for a, b in dec if not any((c, d) != (a, b) and a <= c and d <= b for c, d in dec)]
        assert len(inner) >= 2, (name, inner)  # the unguarded chunk pairs and the guarded tail
        for a, b in inner:
            loop = body[a:b]
            weights = 2 * sum(1 for l in loop if re.match(r"\s+v_pk_fma_f32", l))
            drains = sum(1 for l in loop if re.search(r"s_waitcnt\s+(vmcnt\(\d+\)\s+)?lgkmcnt\(0\)", l) or re.search(r"s_waitcnt\s+0\b", l))
            counted = sum(1 for l in loop if re.search(r"s_waitcnt\s+lgkmcnt\([1-9]\d*\)", l))
            assert weights >= 64, (name, weights)
            assert drains * 32 <= weights, (name, weights, drains)
            assert counted >= 3 * drains, (name, counted, drains)  # the stages between two drains wait by count
            # vec: one SGPR pair per packed FMA, fed by scalar loads of 8 floats -- 32 k's per drain
            assert sum(1 for l in loop if re.match(r"\s+s_load_dwordx8 ", l)) * 8 == weights, name
