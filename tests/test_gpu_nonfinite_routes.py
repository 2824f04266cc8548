"""Non-finite operands on EVERY route, at shapes where the masked code runs.

README and DESIGN.md say that NaN and +-inf follow the reference on every route.  Nearly every kernel here reads unconditionally from
clamped addresses and neutralises the dead lane ("Clamp sites"); tests/test_gpu_nonfinite.py runs at K = 512, N = 320, a
whole number of everything, where no such lane exists.  Here: K = 544 / 1056 and ragged N (tests/nonfinite_cases.py: why these), every
route label of tests/test_gpu_precision.py (one table: labels, options, entries), both bit widths, every kind a route serves, and one
poison CLASS per launch -- vec, codebook, CSR values, full rows, mul -- with clean rows / columns beside the poisoned ones as the leak
check.  tests/test_nonfinite_cases_cpu.py proves on the CPU that the expected pattern of every case does not depend on the order of
summation and that each case names outputs that are +-inf, not NaN, in the reference: a dead lane whose zero meets an infinity shows
NaN there.  tests/test_precision_cpu.py::test_route_manifest plans these shapes and batches for every label.

Asserted against helpers.oracle_ref, as _same_pattern of tests/test_gpu_nonfinite.py does: the NaN, +inf and -inf masks are equal; the
finite outputs are within the project's 2e-5 (max-norm relative over the finite outputs)."""
import numpy as np
import pytest

from tests import nonfinite_cases as NC
from tests import test_gpu_precision as G

pytestmark = pytest.mark.gpu

TOL_FP64 = 2e-5

# the routes' own batches, thinned
THIN = {
    "fused batch-1": (0, 1),
    "batch-1 column-lane": (0, 1),
    "batch tiles of exactly 2..8 rows": (2, 3, 6),
    "column-lane passes of 2..8 rows": (2, 3, 6),
    "fused small launch, planes + transposed vec": (7, 13, 16),
    "fused small launch, in-register split (small_planes = 0)": (7, 13, 16),
    "fused small launch, in-register split (no workspace)": (7, 13, 16),
    "fused small launch, stream-ordered scratch": (7, 13, 16),
    "tile form, 1 / 2 / 4 row blocks, sparse workgroups in the grid": (17, 65),
    "tile form, 1 / 2 / 4 row blocks, sparse launch of its own": (17, 65),
    "wide form, planes": (17, 130),
    "wide form, in-register split": (17, 130),
    "fp32 matrix instruction (control)": (9, 17, 65),
}
assert set(THIN) == {r["label"] for r in G.ROUTES} and all(set(THIN[r["label"]]) <= set(r["batches"]) for r in G.ROUTES)

_COLS1 = next(r for r in G.ROUTES if r["label"] == "batch-1 column-lane")
# the batch-1 column-lane route under the cuts of tests/test_gpu_cols_batch1_cut.py: by slots alone, and on a pretended part of 3 CUs
CUT_ROUTES = [dict(_COLS1, label="batch-1 column-lane, cols_slot_cut = 1", options=dict(_COLS1["options"], cols_slot_cut=1)),
              dict(_COLS1, label="batch-1 column-lane, cu_count = 3", options=dict(_COLS1["options"], cu_count=3))]
THIN.update({r["label"]: (0, 1) for r in CUT_ROUTES})
NF_ROUTES = G.ROUTES + CUT_ROUTES + G.GROUP_ROUTES


def route_launches(route, bits):
    """(K, batch, widths) of a route here: what this file runs and the route manifest plans"""
    if "cases" in route:
        return [(NC.GROUP_K, batch, NC.GROUP_WIDTHS[:n]) for batch, n in route["cases"]]
    return [(K, batch, (N,)) for K, N in NC.SHAPES[bits] for batch in THIN[route["label"]]]


@pytest.fixture(scope="module")
def qc():
    from squeezellm_amd import quant_cuda

    return quant_cuda


# Class C (codebook) on these routes: the narrower contract of include/sqllm_hip.h -- the column of a +-inf codebook entry is NaN or that
# infinity in every row, nothing else is touched.  Their dense roles (dense_role of the fp32 chain kernels, dense_role_mfma of the fp32
# matrix-instruction kernel) zero the VEC of a dead slot and still multiply the re-read weights of the slice's last unit.  A second copy
# of the decode step that zeroes the weights too was built and measured: the 3-bit batch-1 kernel spills 435 registers and 7b-w3-s0 loses
# 11.8 % ("Clamp sites"; profiles/nonfinite_fix_ab.txt).  Classes V, S, F, M: exact.
NARROW_C = ("fused batch-1", "batch tiles of exactly 2..8 rows", "grouped batch tiles", "fp32 matrix instruction (control)")
assert set(NARROW_C) <= {r["label"] for r in NF_ROUTES}


def _compare(got, ref, what):
    """None, or what differs: the first mismatch of this launch, named"""
    got = np.asarray(got).reshape(ref.shape)
    for name, g, r in zip(("NaN", "+inf", "-inf"), NC.pattern_of(got), NC.pattern_of(ref)):
        if not np.array_equal(g, r):
            row, col = np.argwhere(g != r)[0]
            return (f"{what}: {name} pattern differs in {int((g != r).sum())} outputs ({int(g.sum())} got, {int(r.sum())} in the "
                    f"reference); first at row {row} col {col}: got {got[row, col]!r}, reference {ref[row, col]!r}")
    fin = np.isfinite(ref)
    if fin.any():
        scale = np.abs(ref[fin]).max() or 1.0
        err = np.where(fin, np.abs(np.where(fin, got, 0) - np.where(fin, ref, 0)), 0) / scale
        row, col = np.unravel_index(int(np.argmax(err)), err.shape)
        if not err.max() <= TOL_FP64:
            return f"{what}: finite outputs off by {err.max():.3g} (max-norm relative) at row {row} col {col}"
    return None


@pytest.mark.parametrize("cls", NC.CLASSES)
@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("route", NF_ROUTES, ids=[r["label"] for r in NF_ROUTES])
def test_nonfinite_operands_follow_the_reference_on_every_route(qc, gpu, route, bits, cls):
    ran, bad = 0, []
    narrow = cls == "C" and route["label"] in NARROW_C
    for kind in NC.KINDS:
        if not NC.applies(cls, kind):
            continue
        for K, batch, widths in route_launches(route, bits):
            for variant in NC.variants(cls, batch):
                keys = [(bits, K, N, kind, batch, cls, variant) for N in widths]
                ops = [NC.make(*k) for k in keys]
                x = ops[0]["x"]
                assert all(np.array_equal(o["x"], x, equal_nan=True) for o in ops)  # (the ops of a group share vec)
                one_d = batch == 0
                ys = G.launch(qc, gpu, route, [NC.writable(o["case"]) for o in ops], kind, (x[0] if one_d else x).copy(),
                              [(o["mul"][0] if one_d else o["mul"]).copy() for o in ops])  # (copies: the shared arrays are read-only)
                for key, op, y in zip(keys, ops, ys):
                    if narrow:
                        y = NC.admit_nan_for_codebook_infinity(y, op["named"])
                    bad.append(_compare(y, NC.reference(*key), f"{kind} K={K} N={key[2]} of {widths} batch={batch} variant {variant}"))
                ran += 1
    assert ran >= len(route_launches(route, bits))  # (every class has at least the hybrid kind)
    bad = [b for b in bad if b]
    assert not bad, f"route '{route['label']}' w{bits} class {cls}: {len(bad)} of {ran} launches differ:\n" + "\n".join(bad[:12])
