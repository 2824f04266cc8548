"""The four regions tests/test_gpu_attn_ranges.py enters, without a GPU: proof that the gate of tests/attn_decode_cases.py sees, on
that file's own inputs, what each region is there to catch -- and that it is FAIR there, i.e. that an fp32 implementation in the
kernels' structure (attn_decode_cases.model_parts: dot products lane by lane, partitions of P keys, then an ascending combine)
stays inside it.

  A. group ratios 1 .. 8: the five wrong oracles fail at every ratio, "rotate_in_group" (wrong only inside a group) at every
     ratio from 2 on -- over 16-bit values and over the dequantised bytes of an e4m3 cache.
  B. sharp softmax (attn_decode_cases.sharpen): model_parts <= 1.0 on every case; without the combine's rescale it fails every
     profile, without the max subtraction all but "ramp_down", with the maximum taken from partition 0 "ramp_up" and "spike"
     ("ramp_down" is legitimately passed by the last two: partition 0 holds the maximum and nothing overflows).  The expansions for
     2 and 16 new tokens: model_parts <= 1.0 on the draw each case uses, and > 1.0 on every draw attn_append_cases.SHARP_DRAWS
     passes over -- the 21 cases that were changed are exactly those that were unfair to the model.
  C. tables of 18 partitions and 64 rows: model_parts <= 1.0 although the gate's yardstick is the SEQUENTIAL fp32 model, whose
     error grows with the length; a combine that drops a row's last partition fails.
  D. the compact case behind the far offsets: the model inside, keys read from another block outside.
"""
import copy

import numpy as np
import pytest
import torch

from tests import attn_append_cases as A
from tests import attn_decode_cases as C
from tests import kv_fp8_cases as F

P = C.P
RATIOS = [(kind, D, hq, hk, dt) for kind in ("paged", "paged_single") for D in (64, 128) for hq, hk in C.ALL_HEADS for dt in C.DTYPES]
SHARP_SHAPES = ((64, 8, 2), (128, 4, 2), (64, 16, 2))
SHARP = [(kind, D, hq, hk, dt, prof) for kind in ("paged", "padded", "bhsd") for D, hq, hk in SHARP_SHAPES for dt in C.DTYPES
         for prof in C.PROFILES]
LONG = [(kind, D, hq, hk, dt) for kind in ("paged", "padded") for D, hq, hk in ((64, 8, 2), (128, 2, 2)) for dt in C.DTYPES]
FAILS = {"no_rescale": C.PROFILES, "no_max": ("ramp_up", "all_low", "all_high", "spike", "tie"), "first_max": ("ramp_up", "spike")}


def _model_excess(case, want, gate, variant=None):
    return C.excess(C.rounded(C.model_parts(case, variant), case.dtype), want, gate)


def test_the_ranges_are_the_ones_the_kernels_have():
    from squeezellm_amd import quant

    assert [hq // hk for hq, hk in C.ALL_HEADS] == list(range(1, 9)) and all(hk == 2 for _, hk in C.ALL_HEADS)
    assert C.LONG == 17 * P + 5 and (C.LONG + 15) // 16 * 16 > 17 * P  # 18 partitions in a table of blocks of 16
    assert C.MAX_ROWS == A.MAX_ROWS == 64 and quant.ATTN_PARTITION == P
    assert set(C.MUTANTS).isdisjoint(C.GROUP_MUTANTS)


# ---- A ----

@pytest.mark.parametrize("kind,D,hq,hk,dt", RATIOS)
def test_every_mutant_fails_at_every_group_ratio(kind, D, hq, hk, dt):
    """16-bit values and the dequantised bytes; "rotate_in_group" is the identity at ratio 1 and must fail from 2 on"""
    case, want, gate = C.reference(kind, 3, D, hq, hk, dt)
    fc, want8, gate8 = F.reference(kind, 3, D, hq, hk, dt)
    for c, w, g in ((case, want, gate), (fc.shadow, want8, gate8)):
        assert np.isfinite(w).all() and C.excess(C.rounded(w, c.dtype), w, g) <= 1.0
        assert _model_excess(c, w, g) <= 1.0
        for mutant in C.MUTANTS:
            assert C.excess(C.rounded(C.oracle(c, mutant)[0], c.dtype), w, g) > 1.0, mutant
        rotated = C.excess(C.rounded(C.oracle(c, "rotate_in_group")[0], c.dtype), w, g)
        assert (rotated > 1.0) if hq // hk >= 2 else (rotated <= 1.0), rotated


# ---- B ----

def test_sharpen_changes_coordinate_zero_alone():
    plain = C.build("padded", 3, 64, 8, 2, "fp16", 0, C.SHARP_LENS)
    sharp = C.sharpen(plain, "tie")
    assert torch.equal(sharp.v_buf.view(torch.int16), plain.v_buf.view(torch.int16)) and sharp.k_buf is not plain.k_buf
    assert torch.equal(torch.isnan(sharp.k_buf), torch.isnan(plain.k_buf)) and torch.equal(torch.isnan(sharp.q_buf), torch.isnan(plain.q_buf))
    dq = (sharp.q_buf.view(torch.int16) != plain.q_buf.view(torch.int16)).nonzero()
    assert set((dq[:, 1] % 64).tolist()) == {0} and len(dq) == 3 * 8
    changed = int((sharp.k_buf.view(torch.int16) != plain.k_buf.view(torch.int16)).sum())
    assert changed <= sum(C.SHARP_LENS) * 2 + 3 * 2 * 64  # coordinate 0 of every key and head, and the copied key of each row
    assert C.build("padded", 3, 64, 8, 2, "fp16", 0, C.SHARP_LENS) is plain and float(plain.q_buf[0, 0]) != 8.0  # (the shared case is left alone)


@pytest.mark.parametrize("kind,D,hq,hk,dt,prof", SHARP)
def test_sharp_softmax_the_gate_is_fair_and_sees_the_structure(kind, D, hq, hk, dt, prof):
    """the profile's conditions hold on the oracle's scores (asserted inside sharp_reference, for the shadow too); the correct
    partitioned fp32 model is inside the gate; the wrong variants are outside it where the profile is built to show them"""
    case, want, gate = C.sharp_reference(kind, D, hq, hk, dt, prof)
    fc, want8, gate8 = F.sharp_reference(kind, D, hq, hk, dt, prof)
    for c, w, g in ((case, want, gate), (fc.shadow, want8, gate8)):
        good = _model_excess(c, w, g)
        assert good <= 1.0, good
        for variant, profiles in FAILS.items():
            if prof in profiles:
                bad = _model_excess(c, w, g, variant)
                assert bad > 1.0, (variant, bad)


@pytest.mark.parametrize("kind,D,hq,hk,dt,prof", SHARP)
def test_sharp_expansions_are_finite_and_fair(kind, D, hq, hk, dt, prof):
    """what the append tests compare with: the expansion of a sharpened case for 2 and 16 new tokens per sequence, q sharpened the
    same way.  The draw of the new tokens' q that attn_append_cases.SHARP_DRAWS names (the first one for all but 21 cases) has the
    partitioned fp32 model inside the gate, and every draw in front of a listed one has it outside: no case was changed that did
    not have to be."""
    base16 = C.sharp_reference(kind, D, hq, hk, dt, prof)[0]
    base8 = F.sharp_reference(kind, D, hq, hk, dt, prof)[0].shadow
    for fp8, base in ((False, base16), (True, base8)):
        for T in (2, 16):
            used = A.SHARP_DRAWS.get((kind, D, hq, dt, prof, fp8, T), 0)
            for draw in range(used + 1):
                case = A.sharp_expand(base, T, fp8, draw)
                want, gate = C.reference_of(case)
                assert np.isfinite(want).all() and case.B == 3 * T
                fair = _model_excess(case, want, gate)
                assert (fair <= 1.0) if draw == used else (fair > 1.0), (fp8, T, draw, fair)
            assert np.array_equal(A.sharp_expand(base, T, fp8).q_buf.view(torch.int16).numpy(), case.q_buf.view(torch.int16).numpy())


def test_the_listed_draws_are_cases_of_the_sharp_tests():
    assert len(A.SHARP_DRAWS) == 21 and all(d >= 1 for d in A.SHARP_DRAWS.values())
    for kind, D, hq, dt, prof, fp8, T in A.SHARP_DRAWS:
        assert (kind, D, hq, 2, dt, prof) in SHARP and T in (2, 16) and dt == "fp16"


# ---- C ----

@pytest.mark.parametrize("kind,D,hq,hk,dt", LONG)
def test_long_tables_the_partitioned_model_is_inside_the_gate(kind, D, hq, hk, dt):
    case, want, gate = C.long_reference(kind, D, hq, hk, dt)
    fc, want8, gate8 = F.long_reference(kind, D, hq, hk, dt)
    assert case.table.shape[1] * case.block_size >= C.LONG and (case.table.shape[1] * case.block_size + P - 1) // P == 18
    for c, w, g in ((case, want, gate), (fc.shadow, want8, gate8)):
        assert np.isfinite(w).all() and (w[4] == 0).all()
        good = _model_excess(c, w, g)
        assert good <= 1.0, good
        for mutant in ("drop_last", "extra_key", "neighbour_group"):
            assert C.excess(C.rounded(C.oracle(c, mutant)[0], c.dtype), w, g) > 1.0, mutant
        # a combine that drops a row's last partition: one key of 4097 (row 3), and a whole partition of nine (row 1)
        for row, fewer in ((3, 1), (1, P)):
            wrong = copy.copy(c)
            wrong.lens = c.lens.copy()
            wrong.lens[row] -= fewer
            got = C.rounded(C.oracle(wrong)[0], c.dtype)
            assert C.excess(got[row:row + 1], w[row:row + 1], g[row:row + 1]) > 1.0, row


@pytest.mark.parametrize("dt", list(C.DTYPES))
def test_sixty_four_rows(dt):
    lens = C.batch64_lens()
    assert len(lens) == 64 and set(lens) == set(C.LENGTHS)
    case, want, gate = C.reference("paged", 64, 64, 8, 2, dt, lens)
    fc, want8, gate8 = F.reference("paged", 64, 64, 8, 2, dt, F.SCALES, lens)
    for c, w, g in ((case, want, gate), (fc.shadow, want8, gate8)):
        assert np.isfinite(w).all() and _model_excess(c, w, g) <= 1.0
        shifted = np.roll(C.rounded(w, c.dtype), 1, axis=0)  # every row the previous row's result
        assert C.excess(shifted, w, g) > 1.0


# ---- D ----

@pytest.mark.parametrize("dt", list(C.DTYPES))
def test_the_compact_case_behind_the_far_offsets(dt):
    """what tests/test_gpu_attn_ranges.py scatters to slots beyond 2^31 and 2^32: the model inside the gate, a wrong key outside it
    (a lost cast reads another slot or the poison), one query per sequence and two new tokens"""
    case, want, gate = C.reference("paged", 3, 64, 8, 2, dt, C.FAR_LENS)
    fc, want8, gate8 = F.reference("paged", 3, 64, 8, 2, dt, F.SCALES, C.FAR_LENS)
    for c, w, g in ((case, want, gate), (fc.shadow, want8, gate8)):
        assert np.isfinite(w).all() and _model_excess(c, w, g) <= 1.0
        x = A.expand(c, 2)
        wx, gx = C.reference_of(x)
        assert np.isfinite(wx).all() and _model_excess(x, wx, gx) <= 1.0
        wrong = copy.copy(c)
        wrong.table = c.table.copy()
        wrong.table[:, 0] = c.table[:, 1]  # the first block's keys read from the second block's slots
        assert all(C.excess(C.rounded(C.oracle(wrong)[0], c.dtype)[b:b + 1], w[b:b + 1], g[b:b + 1]) > 1.0 for b in range(3))
