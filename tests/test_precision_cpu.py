"""The accuracy gates of tests/test_gpu_precision.py, proved on the CPU before they judge a kernel: the numpy model of the split
arithmetic (tests/precision.py) passes them, every model of a subtly wrong kernel -- one of the six partial products missing, the
vec's lo plane lost -- fails them by a wide margin, and the suite's older gate (max|y - ref| / max|ref| <= 2e-5 on fp16-born vec)
lets the same mutants through.  Also here: the route manifest, which checks on the host layer (no GPU) that every labelled
route of the GPU file reaches the launcher and instantiation its label names."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import precision as P

U = P.U


def test_split3_is_exact():
    """hi + mid + lo == v and lo fits bf16 (asserted inside split3) on normals, powers of two, single low bits, the ends of the normal
    range and both zeros.  Values whose residuals would be subnormal: below |v| = 2^-110 the last bits of v lie under bf16's subnormal
    grid (2^-133), the masks then keep fewer than 8 significant bits and lo no longer fits bf16 -- the kernels' `>> 16` would drop bits.
    The model refuses such a value (asserted); GPU operands stay above 2^-103, where every non-zero plane is a NORMAL bf16 too (a
    matrix instruction may flush subnormal inputs)."""
    rng = np.random.default_rng(0)
    P.split3(rng.normal(size=100000).astype(np.float32) * np.exp2(rng.integers(-60, 60, 100000)).astype(np.float32))
    hi, mid, lo = P.split3(np.exp2(np.arange(-126, 128)).astype(np.float32))
    assert not mid.any() and not lo.any()
    one_bit = (np.float32(1.0).view(np.uint32) | (np.uint32(1) << np.arange(23, dtype=np.uint32))).view(np.float32)
    hi, mid, lo = P.split3(one_bit)
    # (mid is the top 8 significant bits of the RESIDUAL v - hi, wherever they lie: a lone low bit is all of it, and lo is empty)
    assert (mid[:16] == one_bit[:16] - np.float32(1.0)).all() and not lo.any() and (hi[16:] == one_bit[16:]).all() and not mid[16:].any()
    hi, mid, lo = P.split3((one_bit.view(np.uint32) | np.uint32(0x8000)).view(np.float32)[:7])  # ... bit 15 and a bit below bit 7: that one is lo's
    assert (lo == one_bit[:7] - np.float32(1.0)).all() and (mid == np.float32(2.0 ** -8)).all()
    flt_max, flt_min = np.float32(np.finfo(np.float32).max), np.float32(np.finfo(np.float32).tiny)
    hi, mid, lo = P.split3(np.array([flt_max, -flt_max, flt_min, -flt_min, 0.0, -0.0], np.float32))
    assert hi[0].view(np.uint32) == 0x7F7F0000 and mid[0] != 0 and lo[0] != 0 and not mid[2:].any() and not lo[2:].any()
    assert np.signbit(hi[5]) and not np.signbit(hi[4])
    sub = (np.float32(flt_min).view(np.uint32) | np.uint32(0x8081)).view(np.float32)  # smallest normal exponent, residuals subnormal
    with pytest.raises(AssertionError, match="lo does not fit bf16"):
        P.split3(np.array([sub], np.float32))
    hi, mid, lo = P.split3(np.array([sub], np.float32) * np.float32(2.0 ** 23))  # 2^-103: exact, every plane normal
    assert min(abs(hi[0]), abs(mid[0]), abs(lo[0])) >= flt_min


def _dense_figures(K, x, rows=16, cols=256, seed=1):
    rng = np.random.default_rng(seed + K)
    w = P.fp32_born(rng, (K, cols), 0.02)  # codebook values: N(0, 0.02) kept as fp32 (tests/helpers.py: make_case)
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    ref, scale = x64 @ w64, np.sqrt((x64 * x64) @ (w64 * w64))
    fig = {"chain": P.scaled_rms(P.model_chain(x, w), ref, scale), "split": P.scaled_rms(P.model_split(x, w), ref, scale)}
    for i in range(6):
        fig[f"drop{i}"] = P.scaled_rms(P.model_split(x, w, drop=i), ref, scale)
    fig["zero_vec_lo"] = P.scaled_rms(P.model_split(x, w, zero_vec_lo=True), ref, scale)
    return fig, w


@pytest.mark.parametrize("K", [128, 256, 1024])
def test_dense_gate_separates_the_mutants(K):
    """Gate (c).  fp32-born vec and codebook values: the six-product model is no worse than the fp32 FMA chain; a missing SMALL product
    (Am Bm, Ah Bl, Al Bh) or a zeroed vec lo plane costs >= 8 x the chain's error, a missing large one >= 5000 x.  The GPU cap, 2 x the
    chain model, therefore stays a factor >= 4 under the weakest mutant."""
    fig, _ = _dense_figures(K, P.fp32_born(np.random.default_rng(K), (16, K)))
    assert fig["split"] <= fig["chain"], fig
    weakest = min(fig[f"drop{i}"] for i in P.SMALL_PRODUCTS)
    weakest = min(weakest, fig["zero_vec_lo"])
    assert weakest >= 8 * fig["chain"], fig
    assert min(fig[f"drop{i}"] for i in P.LARGE_PRODUCTS) >= 5000 * fig["chain"], fig
    assert P.GATE_DENSE_X_CHAIN * fig["chain"] <= weakest / 4, fig


def test_one_hot_gate_separates_the_mutants():
    """Gate (a) for the split routes, 16 u with u = 2^-24.  One non-zero product p = w x per output, operands split exactly:
      * dropped products: |v - hi| < 2^-7 |v| and |v - hi - mid| < 2^-15 |v|, so |wm xl| + |wl xm| + |wl xl| < (2^-22 + 2^-22 + 2^-30) |p|
        = 8 (1 + 2^-9) u |p|;
      * accumulator roundings: the kept products are exact in fp32 and enter smallest first; a partial sum is rounded relative to ITS
        magnitude: the first (Am Bm, < 2^-14 |p|) is exact, two at < 2^-13 |p|, two at < 2^-6 |p|, the last at |p|: < (1 + 2^-5) u |p|
        if the matrix instruction rounds to nearest, twice that if it truncates.
    Together < 10.1 u |p| either way (the model, rounding to nearest, shows ~6 u); the gate is set at 16 u and holds for a correct kernel
    whatever the instruction's rounding.  Forced planes (mid >= 2^-8, lo >= 2^-16 of the leading power of two) make EVERY element of
    every mutant miss it: a dropped small product or a zeroed lo plane is >= 2^-18 |p| = 64 u per element, four times the gate."""
    rng = np.random.default_rng(3)
    K, rows, cols = 256, 64, 192
    w = P.forced_planes(rng.normal(0, 0.02, (K, cols)).astype(np.float32))
    x = P.one_hot_rows(rows, K, rng.integers(0, K, rows), P.hot_values(rng, rows))
    ref = x.astype(np.float64) @ w.astype(np.float64)
    A = np.abs(ref)
    good = P.worst_over_abs(P.model_split(x, w), ref, A)
    assert good <= 10.1 * U <= P.GATE_ONE_HOT_U * U, good / U
    mutants = {f"drop{i}": P.model_split(x, w, drop=i) for i in range(6)}
    mutants["zero_vec_lo"] = P.model_split(x, w, zero_vec_lo=True)
    for name, y in mutants.items():
        assert P.over_abs(y, ref, A).min() >= 4 * P.GATE_ONE_HOT_U * U, (name, P.over_abs(y, ref, A).min() / U)
    chain = P.model_chain(x, w)  # the chain routes' claim: one product, every other k adds zero -- bit for bit fl32(w x)
    assert np.array_equal(chain, (w[np.nonzero(x)[1]] * x[x != 0][:, None]))


def test_the_blind_spot_fp16_born_vec_and_the_2e5_gate():
    """Why tests/test_gpu_precision.py exists, and why its vec must not be "simplified" back to fp16-born values: at K = 1024, 16 rows x
    256 columns, mul ~ N(0, 0.5), under the neighbouring files' gate rel_err = max|y - ref| / max|ref| <= 2e-5
      * fp16-born vec: a zeroed vec lo plane is BIT-IDENTICAL to the correct sum (there is no lo plane), and every small-product mutant
        passes;
      * fp32-born vec: every small-product mutant and the zeroed lo plane still pass
    -- while gate (c) rejects each of them that changes the sum at all."""
    K = 1024
    for born in (P.fp16_born, P.fp32_born):
        rng = np.random.default_rng(11)
        x = born(rng, (16, K))
        fig, w = _dense_figures(K, x)
        mul = rng.normal(0, 0.5, (16, 256)).astype(np.float32)
        ref = mul.astype(np.float64) + x.astype(np.float64) @ w.astype(np.float64)
        out = lambda d: (mul.astype(np.float64) + d).astype(np.float32)  # noqa: E731
        good = P.model_split(x, w)
        for name, y in [(f"drop{i}", P.model_split(x, w, drop=i)) for i in P.SMALL_PRODUCTS] + [("zero_vec_lo", P.model_split(x, w, zero_vec_lo=True))]:
            assert H.rel_err(out(y), ref) <= 2e-5, (born.__name__, name)  # the old gate stays green
            if born is P.fp16_born and name in ("zero_vec_lo", "drop2"):  # (Al x Bh: the lo plane is zero)
                assert np.array_equal(y, good)
            else:
                assert fig[name] > 4 * P.GATE_DENSE_X_CHAIN * fig["chain"], (born.__name__, name, fig)


# ---- the route manifest ----

DENSE_LAUNCHERS = ("launch_fused", "launch_batched_mfma", "launch_batched_mfma_split", "launch_batched_mfma_split_all", "launch_batched_cols",
                   "launch_small_split")


def _fields(line):
    name, rest = line.split(" ", 1)
    head = rest.split(" seg0{")[0]
    f = dict(kv.split("=", 1) for kv in head.split() if "=" in kv)
    f["name"] = name
    gm = rest.split(" gm{")[1].split("}")[0]
    f["gm"] = dict(kv.split("=") for kv in gm.split())
    return f


def test_route_manifest(tmp_path):
    """Every plannable row of the GPU file's route tables, both bit widths, both kinds, every shape and batch, through the host layer
    (csrc/sqllm_capi.hip) linked against the recording launchers of tests/native/launch_recorder.cpp on a part of 256 CUs: the dense
    launch is the launcher the label names, with the fields that pick its instantiation -- planes / transposed vec / flags null or not,
    wide, blocks of 16 rows per pass, ops per launch -- and the kernels in front of it (prepare_small, split_vec, the sparse launch)
    are there when the label says so.  Rows whose scratch is allocated on the stream cannot be planned without a device: skipped, and
    counted, so that the skip cannot grow unnoticed."""
    from squeezellm_amd import build as B
    from tests import nonfinite_cases as NC
    from tests import test_gpu_nonfinite_routes as R
    from tests import test_gpu_precision as G

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found: the launch recorder cannot be built")
    native = os.path.join(H.ROOT, "tests", "native")
    exe = str(tmp_path / "route_manifest")
    r = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-DSQLLM_RECORDER_NO_MAIN", f"-I{B.INCLUDE}", f"-I{B.CSRC}",
                        os.path.join(B.CSRC, "sqllm_capi.hip"), os.path.join(native, "launch_recorder.cpp"), os.path.join(native, "route_manifest.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    unplannable = [r["label"] for r in G.ALL_ROUTES if not r["plannable"]]
    assert unplannable == ["fused small launch, stream-ordered scratch", "grouped fused small launch, no workspace"]
    assert all(r["entry"] == "named" and r["expect"]["dense"]["launcher"] == "launch_small_split" for r in G.ALL_ROUTES if not r["plannable"])
    cases, lines = {}, []
    for route in G.ALL_ROUTES:
        if not route["plannable"]:
            continue
        for bits in (3, 4):
            for kind in ("dense", "hybrid"):
                for K, batch, widths in G.route_cases(route, bits):
                    ops = [G.make_operands(bits, K, N, kind) for N in widths]
                    cid = f"c{len(cases)}"
                    cases[cid] = (route, bits, kind, K, batch, widths)
                    sizes = " ".join(f"{c['N']},{0 if c['vals'] is None else c['vals'].size},{0 if c['full_rows'] is None else c['full_rows'].shape[1]}" for c in ops)
                    opts = " ".join(f"{k}={v}" for k, v in route["options"].items())
                    lines.append(f"{cid} {'null' if route['entry'] == 'ws-null' else 'ws'} {bits} {K} {batch} {len(ops)} {sizes} {opts}")
    # the shapes and batches of tests/test_gpu_nonfinite_routes.py (K = 544 / 1056, ragged N; every kind, spmv included; the batch-1
    # column-lane route under its two cuts as well): the same launcher and fields as the label's `expect` -- an op with CSR terms
    # alone plans as the hybrid one does.  Every label is reached at these shapes: none had to be moved to another.
    n_precision = len(cases)
    for route in R.NF_ROUTES:
        if not route["plannable"]:
            continue
        for bits in (3, 4):
            for kind in NC.KINDS:
                for K, batch, widths in R.route_launches(route, bits):
                    ops = [NC._base(bits, K, N, kind)[0] for N in widths]
                    cid = f"c{len(cases)}"
                    cases[cid] = (route, bits, kind, K, batch, widths)
                    sizes = " ".join(f"{c['N']},{0 if c['vals'] is None else c['vals'].size},{0 if c['full_rows'] is None else c['full_rows'].shape[1]}" for c in ops)
                    opts = " ".join(f"{k}={v}" for k, v in route["options"].items())
                    lines.append(f"{cid} {'null' if route['entry'] == 'ws-null' else 'ws'} {bits} {K} {batch} {len(ops)} {sizes} {opts}")
    assert {r["label"] for r in R.NF_ROUTES} >= {r["label"] for r in G.ALL_ROUTES} and len(cases) - n_precision > 300
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    seen, cur, trace = set(), None, []
    for ln in out.stdout.splitlines():
        if ln.startswith("begin "):
            cur, trace = ln.split()[1], []
            continue
        if not ln.startswith("end "):
            trace.append(ln)
            continue
        assert ln.split()[1] == cur and ln.split()[2] == "rc=0", ln
        route, bits, kind, K, batch, widths = cases[cur]
        what = f"route '{route['label']}' w{bits} {kind} K={K} batch={batch} widths={widths}:\n" + "\n".join(t[:400] for t in trace)
        seen.add(cur)
        exp = route["expect"]["dense" if kind == "dense" else "hybrid"]
        names = [t.split(" ", 1)[0] for t in trace]
        dense = [_fields(t) for t in trace if t.split(" ", 1)[0] in DENSE_LAUNCHERS]
        per_op = exp["launcher"] in ("launch_batched_mfma", "launch_batched_mfma_split", "launch_batched_mfma_split_all")
        assert len(dense) == (len(widths) if per_op else 1), what
        for d in dense:
            assert d["name"] == exp["launcher"], what
            assert int(d["n_seg"]) == (1 if per_op else len(widths)) and int(d["gm"]["batch"]) == max(batch, 1) and int(d["gm"]["K"]) == K, what
            for key, field in (("planes", "planes"), ("xT", "xT"), ("flags", "flags")):
                if key in exp:
                    assert (d[field] != "(nil)") == exp[key], (key, what)
            if "wide" in exp:
                assert int(d["wide"]) == exp["wide"], what
            if "row_blocks" in exp:  # (LaunchArgs.row_blocks 0: the launcher's own rule, csrc/sqllm_kernels.h: mfma_row_blocks)
                rb = int(d["row_blocks"]) or (1 if batch <= 16 else 2 if batch <= 32 else 4)
                assert rb == exp["row_blocks"][batch], what
        sparse_terms = kind != "dense"
        assert ("prepare_small" in names) == bool(exp.get("planes") and exp["launcher"] == "launch_small_split"), what
        assert ("transpose_small" in names) == bool(exp.get("xT") and not exp.get("planes") and exp["launcher"] == "launch_small_split"), what
        assert ("split_vec" in names) == bool(exp.get("planes") and exp.get("wide")), what
        if exp["launcher"] == "launch_batched_mfma_split_all" or not per_op:
            assert "launch_batched_sparse" not in names, what
        elif sparse_terms:  # a per-op matrix-core launch without the sparse workgroups in its grid: their own launch in front
            assert names.count("launch_batched_sparse") == len(widths), what
    assert seen == set(cases) and len(cases) > 400
