"""The head of the column-lane kernel's ONE-ROW instantiations in the generated gfx950 code (csrc/sqllm_kernels.hip: dense_role_cols,
BT == 1; hipcc cross-compiles without a GPU): vec's first group of 32 k's -- four s_load_dwordx8 -- is requested WITH the piece's first
loads (codebook values, the first weight chunks), in front of the table barrier.  Behind the barrier it was a second, dependent memory
round trip in front of the piece's first FMA, paid by every workgroup of a launch at once.
Compiled as tests/test_codegen_cols_batch1_cpu.py compiles (the product flags); that file keeps the register and drain guards."""
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
    out = tmp_path_factory.mktemp("asm_cols_head") / "k.s"
    cmd = [hipcc, f"--offload-arch={B.ARCH}", *[f for f in B.FLAGS if f != "-fPIC"], "-S", "--cuda-device-only",
           f"-I{B.INCLUDE}", f"-I{B.CSRC}", os.path.join(B.CSRC, "sqllm_kernels.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True)
    return out.read_text()


def _batch1_bodies(asm):
    out = {}
    for m in re.finditer(r"^(" + PREFIX + r"[34]ELi1ELi8E\w+):.*?^\.Lfunc_end", asm, re.S | re.M):
        out[m.group(1)] = [re.sub(r"\s*;.*", "", l) for l in m.group(0).split("\n")]
    return out


def test_first_vec_group_is_requested_in_front_of_the_table_barrier(asm):
    ks = _batch1_bodies(asm)
    assert len(ks) == 2
    for name, body in ks.items():
        # the dense role: from the role's first weight load (the sparse roles in front of it use no buffer loads)
        start = next(i for i, l in enumerate(body) if re.match(r"\s+buffer_load_dword ", l))
        role = body[start:]
        vec = [i for i, l in enumerate(role) if re.match(r"\s+s_load_dwordx8 ", l)]
        barrier = next(i for i, l in enumerate(role) if re.match(r"\s+s_barrier\b", l))
        fma = next(i for i, l in enumerate(role) if re.match(r"\s+v_pk_fma_f32 ", l))
        assert len(vec) >= 4, (name, len(vec))
        assert vec[3] < barrier, f"{name}: vec's first group is requested behind the table barrier (s_load_dwordx8 at +{vec[:4]}, s_barrier at +{barrier})"
        assert barrier < fma, (name, barrier, fma)
        # the codebook wait stays a counted one: the table build must not wait for the weight chunks
        waits = [l for l in role[:barrier] if re.match(r"\s+s_waitcnt ", l)]
        assert not any(re.search(r"vmcnt\(0\)", l) or re.search(r"s_waitcnt\s+0\b", l) for l in waits), (name, waits)
