"""The non-finite cases of tests/nonfinite_cases.py, proved on the CPU before they judge a kernel.  For EVERY case the GPU files can ask
for -- none is skipped or filtered; a seed that fails is changed in the generator --:
  (a) the term-wise, order-independent pattern model equals the pattern of helpers.oracle_ref (the fp64 oracle pinned to the reference):
      the expected NaN / +inf / -inf masks do not depend on how a kernel orders its sum;
  (b) the case discriminates: the outputs it names are +-inf and NOT NaN in the reference, and there is at least one per name -- a
      kernel that forms 0 x inf in a masked lane, or inf - inf of its own making, shows NaN there and fails;
  (c) every output that carries no poison is finite."""
import numpy as np
import pytest

from tests import nonfinite_cases as NC

CASES = NC.operator_cases()


def _check(what, ref_pattern, named, clean):
    nan, pos, neg = ref_pattern
    for name, rows, cols, sign, mode in named:
        rows, cols = np.asarray(rows), np.asarray(cols)
        assert rows.size and cols.size, (what, name)
        p, n = pos[np.ix_(rows, cols)], neg[np.ix_(rows, cols)]
        hit = p if sign > 0 else n if sign < 0 else p | n
        assert hit.all() if mode == "all" else hit.any(), (what, name, int(hit.sum()), hit.size)
    assert not (nan | pos | neg)[clean].any(), (what, "an output without poison is not finite")
    assert (nan | pos | neg)[~clean].any(), (what, "the poison reaches no output")


def test_case_list_is_complete():
    """both bit widths, every kind, every class the kind has, every shape, the one-row variants: a fixed count, so that a case cannot
    drop out unnoticed"""
    per_bits = {b: sum(1 for c in CASES if c[0] == b) for b in (3, 4)}
    assert per_bits[3] == per_bits[4] and len(CASES) == len(set(CASES))
    kinds_classes = sum(1 for k in NC.KINDS for c in NC.CLASSES if NC.applies(c, k))
    assert kinds_classes == 3 + 3 + 2 + 1 + 3
    shapes = 2 * 12 + 4 * 4 - 2  # SHAPES x batches + group widths x rows, (544, 132) at 1 and 13 rows in both
    v_extra = 3 * (NC.ONE_ROW_VARIANTS - 1) * (2 * 2 + 4 - 1)  # class V, three kinds: batches 0 and 1 of SHAPES, 1 row of the group widths
    assert per_bits[4] == kinds_classes * shapes + v_extra


@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("kind", NC.KINDS)
@pytest.mark.parametrize("cls", NC.CLASSES)
def test_every_case_is_order_independent_and_discriminating(bits, kind, cls):
    mine = [c for c in CASES if c[0] == bits and c[3] == kind and c[5] == cls]
    assert bool(mine) == NC.applies(cls, kind)
    for key in mine:
        c = NC.make(*key)
        ref = NC.pattern_of(NC.reference(*key))
        model = NC.pattern_model(c["case"], c["x"], c["mul"], kind)
        for name, m, r in zip(("NaN", "+inf", "-inf"), model, ref):
            assert np.array_equal(m, r), (key, name, int(m.sum()), int(r.sum()))  # (a)
        _check(key, ref, c["named"], c["clean"])  # (b), (c)
        if cls == "M":
            assert sum(int(m.sum()) for m in ref) == 3, key  # exactly the three poisoned outputs


def test_one_codebook_infinity_under_a_positive_vec_is_one_column():
    """544 x 132 at 13 rows, on this generator's hybrid operands (not the operands of any earlier hand check): +inf at vec[0, K - 1]
    makes every output of row 0 non-finite; and a codebook +inf under a strictly positive vec gives +inf in exactly that column of all
    13 rows, with no NaN and no -inf anywhere."""
    for bits in (3, 4):
        c = NC.make(bits, 544, 132, "hybrid", 13, "V")
        nan, pos, neg = NC.pattern_of(NC.reference(bits, 544, 132, "hybrid", 13, "V"))
        assert (nan | pos | neg)[0].all() and (pos | neg)[0].any()
        lut = np.array(c["case"]["lookup_table"])
        cc = dict(c["case"], lookup_table=lut)
        k_idx = NC.H.oracle.unpack_indices(cc["qweight"], bits)[543, 5]
        lut[5, k_idx] = np.inf
        x = np.abs(c["x"]) + np.float32(0.01)
        x = np.where(np.isfinite(x), x, np.float32(1))
        with np.errstate(all="ignore"):
            ref = NC.H.oracle_ref(cc, x, np.zeros((13, 132), np.float32), "hybrid")
        nan, pos, neg = NC.pattern_of(ref)
        assert pos[:, 5].all() and pos.sum() == 13 and not nan.any() and not neg.any()


@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("kind", ["dense", "hybrid"])
@pytest.mark.parametrize("cls", ["V", "C"])
@pytest.mark.parametrize("to16", [NC.to_fp16, NC.to_bf16], ids=["fp16", "bf16"])
def test_fused_linear_cases(bits, kind, cls, to16):
    """the same three statements for the fused linears' cases, for BOTH roundings of the activations the GPU files use (fp16-born and
    bf16-born vec, bias), and: every finite sum stays far inside the fp16 range"""
    for rows in NC.LINEAR_ROWS:
        c = NC.linear_case(bits, kind, rows, cls, to16)
        assert np.array_equal(to16(c["x16"]), c["x16"], equal_nan=True)  # (16-bit-born: rounding again changes nothing)
        with np.errstate(all="ignore"):
            ref = NC.H.oracle_ref(c["case"], c["x16"], np.broadcast_to(c["bias"], (rows, c["case"]["N"])), kind)
        rp = NC.pattern_of(ref)
        for m, r in zip((c["nan"], c["pos"], c["neg"]), rp):
            assert np.array_equal(m, r), (bits, kind, rows, cls)
        _check((bits, kind, rows, cls), rp, c["named"], c["clean"])
        assert (np.abs(ref[np.isfinite(ref)]) < 64).all()
