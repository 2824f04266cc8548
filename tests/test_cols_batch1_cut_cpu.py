"""The ONE-ROW cut of the column-lane kernel (csrc/sqllm_capi.hip: cut_ranges_one_row, best_aligned_cut) and the pair route of
cols_pays_batch1, on a part of 256 CUs without a GPU: plans come through sqllm_plan_query for single ops and through the recording
launchers (tests/native/launch_recorder.cpp + route_manifest.cpp) for groups.

What is computed HERE from a plan, with the kernel's own walk (csrc/sqllm_kernels.hip: dense_role_cols) re-stated in Python:
  coverage   every unit of every column tile belongs to exactly one piece of one workgroup;
  slots      a wave of a piece of n units has n_w = ceil((n - w) / 8) units and executes NB * D * ceil(ceil(n_w / D) / NB) unit
             slots (D = 4 units per chunk at 4 bits, 2 at 3 bits; NB = 2 chunks in flight); efficiency = units / slots.

Two settings of the cut are checked.  Option cols_slot_cut = 1 is the rule by slots alone (the best tile-aligned cut wherever it
executes no more slots than the plan of cut_ranges): it must give 4 x 128 units per tile for the 7B q/k/v group, eleven ranges (ten of
128 units, one of 96) for the 7B down_proj and 2 x 256 for the 7B gate/up pair, >= 95 % live slots on all three.  The DEFAULT adopts that
cut only where the plan of cut_ranges has ranges that cross tile boundaries: on the MI355X the 7B down_proj measured 3.5 % slower on
eleven ranges of 128 (704 workgroups) than on the twelve of 120 (768 = three per CU) it has, so it keeps them -- 93.5 % live slots --
and tests/test_capi_cpu.py goes on pinning its 768 workgroups; q/k/v and gate/up are the same under both settings."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import helpers as H

CUS, WAVES = 256, 8
SHAPES = {  # launch -> (K, [N of every op])
    "7b-qkv": (4096, [4096] * 3), "7b-gateup": (4096, [11008] * 2), "7b-down": (11008, [4096]),
    "13b-qkv": (5120, [5120] * 3), "13b-gateup": (5120, [13824] * 2), "13b-down": (13824, [5120]),
}
ONE_ROW = "cols_min_batch=1 cols_max_batch=1"                        # every one-row launch on the column-lane kernel
TWO_ROWS = "cols_min_batch=1 cols_max_batch=16 mfma_min_batch=1000"  # the same launch at 2 rows: the plan of cut_ranges, target and all


def _slots_of_piece(bits, n):
    d, nb = (4, 2) if bits == 4 else (2, 2)
    slots = 0
    for w in range(WAVES):
        n_w = -(-(n - w) // WAVES) if n > w else 0
        slots += nb * d * -(-(-(-n_w // d)) // nb)
    return slots


def _walk(gm):
    """(tile, u0, u1) of every piece of every dense workgroup, as dense_role_cols walks its range."""
    tiles, U, upw, ks, blocks = gm["col_tiles"], gm["units_total"], gm["units_per_wg"], gm["k_slices"], gm["dense_blocks"]
    stride = ks * upw if blocks == tiles * ks else U
    total = tiles * stride
    for bid in range(blocks):
        gpos, gend = bid * upw, min(bid * upw + upw, total)
        while gpos < gend:
            ct = gpos // stride
            u0 = gpos - ct * stride
            if u0 >= U:
                gpos = (ct + 1) * stride
                continue
            u1 = min(U, u0 + gend - gpos)
            gpos += u1 - u0
            if u1 == U:
                gpos = (ct + 1) * stride
            yield bid, ct, u0, u1


def _measure(bits, gms):
    """coverage check + (units, slots, workgroups, does any range cross a tile boundary) of a launch's ops"""
    units = slots = wgs = 0
    crossing = False
    for gm in gms:
        seen = np.zeros((gm["col_tiles"], gm["units_total"]), dtype=np.int32)
        pieces_of = {}
        for bid, ct, u0, u1 in _walk(gm):
            assert 0 <= ct < gm["col_tiles"] and 0 <= u0 < u1 <= gm["units_total"], gm
            seen[ct, u0:u1] += 1
            slots += _slots_of_piece(bits, u1 - u0)
            pieces_of[bid] = pieces_of.get(bid, 0) + 1
        assert (seen == 1).all(), f"units covered {seen.min()}..{seen.max()} times: {gm}"
        crossing = crossing or max(pieces_of.values()) > 1
        units += gm["col_tiles"] * gm["units_total"]
        wgs += gm["dense_block0"] + gm["dense_blocks"]
    return units, slots, wgs, crossing


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    """cases -> {id: (launcher, [geometry of every op])}: the host layer as plain C++ against the recording launchers"""
    from squeezellm_amd import build as B

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found: the launch recorder cannot be built")
    native = os.path.join(H.ROOT, "tests", "native")
    exe = str(tmp_path_factory.mktemp("cut") / "route_manifest")
    r = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-DSQLLM_RECORDER_NO_MAIN", f"-I{B.INCLUDE}", f"-I{B.CSRC}",
                        os.path.join(B.CSRC, "sqllm_capi.hip"), os.path.join(native, "launch_recorder.cpp"), os.path.join(native, "route_manifest.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def plan(cases):  # cases: {id: (bits, K, batch, [(N, nnz, topX)], "option=value ...")}
        lines = [f"{cid} ws {bits} {K} {batch} {len(ops)} " + " ".join(f"{n},{nnz},{topx}" for n, nnz, topx in ops) + " " + opts
                 for cid, (bits, K, batch, ops, opts) in cases.items()]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
        res, cur = {}, None
        for ln in out.stdout.splitlines():
            if ln.startswith("begin "):
                cur = ln.split()[1]
            elif ln.startswith("end "):
                rc = int(ln.split()[2].split("=")[1])
                if rc:  # a refused case: (error code, no geometry)
                    assert cur not in res, f"{cur}: launched and refused"
                    res[cur] = (rc, [])
            elif ln.startswith("launch_"):
                assert cur not in res, f"{cur}: more than one launch"
                gms = [{k: int(v) for k, v in (kv.split("=") for kv in g.split())} for g in re.findall(r"gm\{([^}]*)\}", ln)]
                res[cur] = (ln.split(" ", 1)[0], gms)
        assert set(res) == set(cases)
        return res

    return plan


def _cases(extra=""):
    cases = {}
    for name, (K, widths) in SHAPES.items():
        for bits in (3, 4):
            ops = [(n, 0, 0) for n in widths]
            cases[f"{name}-w{bits}-one"] = (bits, K, 0, ops, f"{ONE_ROW} {extra}")
            cases[f"{name}-w{bits}-two"] = (bits, K, 2, ops, TWO_ROWS)
    return cases


@pytest.mark.parametrize("slot_cut", [0, 1])
def test_one_row_plans(planner, slot_cut):
    """7B and 13B shapes x 3 and 4 bits x {q/k/v, gate/up, down_proj} at one row, under both settings of cols_slot_cut: every unit once, ranges of
    whole waves, at most four workgroups per CU, never more slots than the plan of cut_ranges for the same launch; and what each setting promises."""
    res = planner(_cases(f"cols_slot_cut={slot_cut}"))
    eff = {}
    for name in SHAPES:
        for bits in (3, 4):
            via, gms = res[f"{name}-w{bits}-one"]
            via2, gms2 = res[f"{name}-w{bits}-two"]
            assert via == via2 == "launch_batched_cols" and len(gms) == len(SHAPES[name][1])
            assert all(g["batch"] == 1 for g in gms) and all(g["batch"] == 2 for g in gms2)
            units, slots, wgs, crossing = _measure(bits, gms)
            units2, slots2, wgs2, crossing2 = _measure(bits, gms2)
            print(f"{name} w{bits} cols_slot_cut={slot_cut}: {gms[0]['k_slices']} x {gms[0]['units_per_wg']} units, {wgs} workgroups, "
                  f"{100 * units / slots:.1f} % live slots (cut_ranges: {gms2[0]['k_slices']} x {gms2[0]['units_per_wg']}, {wgs2}, {100 * units2 / slots2:.1f} %)")
            assert all(g["units_per_wg"] % WAVES == 0 for g in gms)
            assert wgs <= 4 * CUS
            assert units == units2 and slots <= slots2  # slot efficiency >= that of the cut_ranges plan
            same = [[g[k] for k in ("units_per_wg", "k_slices", "dense_blocks")] for g in gms] == [[g[k] for k in ("units_per_wg", "k_slices", "dense_blocks")] for g in gms2]
            if not same:  # a new cut is whole ranges per tile
                assert not crossing and all(g["dense_blocks"] == g["col_tiles"] * g["k_slices"] for g in gms)
            if not slot_cut:  # the default touches only plans whose ranges cross tile boundaries
                assert same or crossing2
            eff[name, bits] = units / slots

    def cut(name):  # ranges of a tile of the launch's first op, in units
        g = res[f"{name}-w4-one"][1][0]
        return [min(g["units_per_wg"], g["units_total"] - i * g["units_per_wg"]) for i in range(g["k_slices"])]

    assert cut("7b-qkv") == [128] * 4 and eff["7b-qkv", 4] >= 0.95
    assert cut("7b-gateup") == [256] * 2 and eff["7b-gateup", 4] >= 0.95
    if slot_cut:
        assert cut("7b-down") == [128] * 10 + [96] and eff["7b-down", 4] >= 0.95
    else:  # (measured: the twelve aligned ranges it has are faster -- module docstring)
        assert cut("7b-down") == [120] * 11 + [56] and 0.93 <= eff["7b-down", 4] < 0.95


def test_plan_query_single_ops_and_options():
    """down_proj through sqllm_plan_query; target_wgs and groups_per_wave go on overriding the cut, as they do in cut_ranges."""
    from squeezellm_amd import _lib

    _lib.set_option("cu_count", CUS)
    try:
        assert _lib.plan_query(4, 11008, 4096)["dense_blocks"] == 768 and _lib.plan_query(4, 11008, 4096)["groups_per_wave"] == 120
        _lib.set_option("cols_slot_cut", 1)
        p = _lib.plan_query(4, 11008, 4096)
        assert (p["dense_blocks"], p["k_slices"], p["groups_per_wave"]) == (704, 11, 128)
        p13 = _lib.plan_query(4, 13824, 5120)  # 1728 units = 27 quanta: nine ranges of 192 are whole chunk pairs already
        assert (p13["dense_blocks"], p13["k_slices"], p13["groups_per_wave"]) == (720, 9, 192)
        _lib.set_option("target_wgs", 512)
        p = _lib.plan_query(4, 11008, 4096)
        assert (p["dense_blocks"], p["k_slices"], p["groups_per_wave"]) == (512, 8, 176)
        _lib.set_option("target_wgs", 0)
        _lib.set_option("groups_per_wave", 20)
        p = _lib.plan_query(4, 11008, 4096)
        assert p["groups_per_wave"] == 160 and p["dense_blocks"] == -(-64 * 1376 // 160)
    finally:
        for n in ("cols_slot_cut", "target_wgs", "groups_per_wave", "cu_count"):
            _lib.set_option(n, 0)


def test_pair_route_and_unchanged_plans(planner):
    """cols_pays_batch1: the dense-only 4-bit pair of >= 16 MB takes the column-lane kernel where its plan is whole-tile ranges with >= 95 % live slots
    (7B: 2 x 256 units per tile; 13B: 1 x 640 -- of the cuts with equal slots the largest workgroup count up to three per CU, measured --; 65B: 1 x 1024); with sparse roles in the grid it keeps the fused kernel, and so does a pair under 16 MB.  The one-row cut is
    reached from one-row launches only: at 2 rows and more cols_slot_cut changes nothing."""
    cases = {
        "7b": (4, 4096, 0, [(11008, 0, 0)] * 2, ""), "7b-b1": (4, 4096, 1, [(11008, 0, 0)] * 2, ""), "13b": (4, 5120, 0, [(13824, 0, 0)] * 2, ""),
        "65b": (4, 8192, 0, [(22016, 0, 0)] * 2, ""),
        "7b-s45": (4, 4096, 0, [(11008, 202_899, 10)] * 2, ""), "small": (4, 2048, 0, [(4096, 0, 0)] * 2, ""),
        "7b-w3": (3, 4096, 0, [(11008, 0, 0)] * 2, ""),
    }
    for name, (K, widths) in SHAPES.items():
        for bits in (3, 4):
            for batch in (2, 3, 4):
                for sc in (0, 1):
                    cases[f"{name}-w{bits}-b{batch}-sc{sc}"] = (bits, K, batch, [(n, 0, 0) for n in widths], f"{TWO_ROWS} cols_slot_cut={sc}")
    res = planner(cases)
    for cid, upw, ks in (("7b", 256, 2), ("7b-b1", 256, 2), ("13b", 640, 1), ("65b", 1024, 1)):
        via, gms = res[cid]
        assert via == "launch_batched_cols" and [(g["units_per_wg"], g["k_slices"]) for g in gms] == [(upw, ks)] * 2, (cid, via, gms)
        units, slots, wgs, crossing = _measure(4, gms)
        assert not crossing and units == slots and wgs <= 4 * CUS
    assert res["7b-s45"][0] == "launch_fused" and res["small"][0] == "launch_fused"
    assert res["7b-w3"][0] == "launch_batched_cols"  # (as before: 2 x 64 units per tile, 100 %)
    for name in SHAPES:
        for bits in (3, 4):
            for batch in (2, 3, 4):
                assert res[f"{name}-w{bits}-b{batch}-sc0"] == res[f"{name}-w{bits}-b{batch}-sc1"]


def test_invalid_pair_is_refused_not_planned(planner):
    """The pair rule of cols_pays_batch1 plans the launch, and routing runs in front of validation: a dense 4-bit pair of >= 16 MB at one row that
    validation refuses (an op without columns, N not a multiple of 4, K = 0 or not a multiple of 32) must come back with SQLLM_E_SHAPE as it
    always did, not divide by its zero tile count; ops that differ in K or bits, with SQLLM_E_GROUP."""
    import ctypes

    from squeezellm_amd import _lib

    cases = {
        "n0": (4, 4096, 0, [(11008, 0, 0), (0, 0, 0)], ""), "n0-first": (4, 4096, 0, [(0, 0, 0), (11008, 0, 0)], ""),
        "n-odd": (4, 4096, 0, [(11008, 0, 0), (11006, 0, 0)], ""), "k0": (4, 0, 0, [(11008, 0, 0)] * 2, ""),
        "k-odd": (4, 4112, 0, [(11008, 0, 0)] * 2, ""), "n-neg": (4, 4096, 1, [(11008, 0, 0), (-64, 0, 0)], ""),
        "valid": (4, 4096, 0, [(11008, 0, 0)] * 2, ""),
    }
    res = planner(cases)
    for cid in cases:
        if cid == "valid":
            assert res[cid][0] == "launch_batched_cols"
        else:
            assert res[cid] == (-2, []), (cid, res[cid])  # SQLLM_E_SHAPE
    lib = _lib.load()
    ops = (_lib.SqllmOp * 2)()
    for K1, bits1 in ((8192, 4), (4096, 3)):
        for i, op in enumerate(ops):
            op.bits, op.batch, op.K, op.N = 4, 0, 4096, 11008
            op.vec, op.qweight, op.mul, op.lookup_table = 16, 32 * (i + 1), 16 * (i + 3), 16 * (i + 5)
        ops[1].K, ops[1].bits = K1, bits1
        assert lib.sqllm_launch_group(ops, 2, None) == -8  # SQLLM_E_GROUP, before anything touches a device


def test_small_group_on_three_cus_is_recut(planner):
    """What tests/test_gpu_cols_batch1_cut.py relies on for its "default-3cus" cut: on a pretended part of 3 CUs the plan of cut_ranges for the
    two-op group N = (136, 72) crosses tile boundaries at every K of that file, and the one-row cut replaces it by whole ranges per tile of another length."""
    cases = {}
    for bits, K in ((4, 512), (4, 1280), (4, 2816), (3, 1024), (3, 2560)):
        ops = [(136, 0, 0), (72, 0, 0)]
        cases[f"w{bits}-{K}-one"] = (bits, K, 0, ops, f"{ONE_ROW} cu_count=3")
        cases[f"w{bits}-{K}-two"] = (bits, K, 2, ops, f"{TWO_ROWS} cu_count=3")
    res = planner(cases)
    for cid in cases:
        if cid.endswith("-two"):
            continue
        gms, gms2 = res[cid][1], res[cid[:-3] + "two"][1]
        bits = int(cid[1])
        _, slots, _, crossing = _measure(bits, gms)
        _, slots2, _, crossing2 = _measure(bits, gms2)
        assert crossing2 and not crossing and slots <= slots2, (cid, gms, gms2)
        assert all(g["dense_blocks"] == g["col_tiles"] * g["k_slices"] for g in gms)
        assert [g["units_per_wg"] for g in gms] != [g["units_per_wg"] for g in gms2], (cid, gms, gms2)
