"""CPU tests of bench.py's command line and output dump: a plain run times one block of --steps steps and nothing
beside the headline, --full brings back the repeated blocks (and every other leg), and --dump-outputs writes float32
.npy files, cut to a fixed sample when the outputs exceed the size budget."""
import numpy as np
import torch

import bench


def parse(monkeypatch, *argv):
    monkeypatch.setattr("sys.argv", ["bench.py", *argv])
    return bench.parse_args()


def test_plain_run_is_one_block_and_full_restores_the_repeats(monkeypatch):
    a = parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.repeats, a.full, a.dump_outputs) == (7, 2, 1, False, None)
    b = parse(monkeypatch, "--full")
    assert b.full and b.repeats == 5
    assert parse(monkeypatch, "--full", "--repeats", "2").repeats == 2
    assert parse(monkeypatch, "--dump-outputs", "out").dump_outputs == "out"


def test_dump_outputs_writes_float32_npy(tmp_path):
    named = [("layers.0.q_proj", torch.arange(6, dtype=torch.float32)), ("layers.0.o_proj", torch.ones(2, 3, dtype=torch.float16))]
    assert bench.dump_outputs(str(tmp_path / "out"), named) == 2
    q = np.load(tmp_path / "out" / "layers.0.q_proj.npy")
    o = np.load(tmp_path / "out" / "layers.0.o_proj.npy")
    assert q.dtype == np.float32 and np.array_equal(q, np.arange(6))
    assert o.dtype == np.float32 and o.shape == (2, 3) and (o == 1).all()


def test_dump_outputs_samples_the_same_elements_beyond_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 400)
    y = torch.arange(1000, dtype=torch.float32)
    bench.dump_outputs(str(tmp_path / "a"), [("y", y)])
    bench.dump_outputs(str(tmp_path / "b"), [("y", y)])
    a, b = np.load(tmp_path / "a" / "y.npy"), np.load(tmp_path / "b" / "y.npy")
    assert a.dtype == np.float32 and a.nbytes <= 400 and a.size == 100
    assert np.array_equal(a, b) and (np.diff(a) > 0).all()  # a fixed sample, in element order
