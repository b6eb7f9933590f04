"""bench.py --dump-outputs: the writer of the last step's (U, s, V)."""
import importlib.util
import os
import types

import numpy as np
import torch


def _bench():
    spec = importlib.util.spec_from_file_location(
        "bench", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    bench = _bench()
    g = torch.Generator().manual_seed(3)
    U = torch.randn(5000, 20, generator=g).to(torch.bfloat16)
    s = torch.rand(20, generator=g, dtype=torch.float64)
    V = torch.randn(100, 20, generator=g)
    comm = types.SimpleNamespace(rank=0)
    # small enough: every row, in order; bf16 widens to float32, float64 stays
    bench.dump_outputs(str(tmp_path / "a"), U, s, V, comm)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(got) == ["U", "U_rows", "V", "s"]
    assert got["U"].dtype == np.float32 and got["s"].dtype == np.float64 and got["V"].dtype == np.float32
    assert np.array_equal(got["U"], U.float().numpy()) and np.array_equal(got["U_rows"], np.arange(5000.0))
    assert np.array_equal(got["s"], s.numpy()) and np.array_equal(got["V"], V.numpy())
    # over the cap: a sorted sample of distinct rows, the same on every call, inside the cap
    monkeypatch.setattr(bench, "DUMP_BYTES", 100_000)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), U, s, V, comm)
    rows = np.load(tmp_path / "b" / "U_rows.npy")
    assert 0 < len(rows) < 5000 and np.all(np.diff(rows) > 0) and rows[-1] < 5000
    assert np.array_equal(np.load(tmp_path / "b" / "U.npy"), U.float().numpy()[rows.astype(np.int64)])
    total = 0
    for f in os.listdir(tmp_path / "b"):
        x = np.load(tmp_path / "b" / f)
        assert np.array_equal(x, np.load(tmp_path / "c" / f))
        total += x.nbytes
    assert total <= 100_000
    # a rank other than 0 writes nothing
    bench.dump_outputs(str(tmp_path / "d"), U, s, V, types.SimpleNamespace(rank=1))
    assert not (tmp_path / "d").exists()
