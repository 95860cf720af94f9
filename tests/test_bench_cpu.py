"""bench.py pieces that run without a GPU: the optional sysfs sampler degrades to nothing when the hwmon files are absent, and
the synthetic problem builders are deterministic (the GPU tests and the oracle legs rely on identical inputs)."""
import os
import sys

import numpy as np
import torch

from conftest import ROOT

sys.path.insert(0, ROOT)


def test_device_sampler_without_hwmon_files_reports_nothing():
    import bench
    with bench.DeviceSampler("0000:ff:1f.7") as s:          # no such card: falls back to every card, here none with hwmon files
        s.read_once()
    assert s.summary() is None or isinstance(s.summary(), dict)
    s2 = bench.DeviceSampler(None, period=None)
    s2.read_once()
    assert s2.summary() is None or "cards_sampled" in s2.summary()


def test_synthetic_inputs_are_deterministic():
    import bench
    ue1, ud1 = bench.pems_like_graph(64, 71, seed=0)
    ue2, ud2 = bench.pems_like_graph(64, 71, seed=0)
    assert torch.equal(ue1, ue2) and torch.equal(ud1, ud2)
    assert ue1.shape == (142, 2)                               # both directions of 71 undirected edges
    y1 = bench.synth_y(64, 5, 12, seed=1, offset=3, device=torch.device("cpu"))
    y2 = bench.synth_y(64, 5, 12, seed=1, offset=3, device=torch.device("cpu"))
    assert y1.shape == (5, 12, 64, 1) and torch.equal(y1, y2)
    assert not torch.equal(y1, bench.synth_y(64, 5, 12, seed=1, offset=4, device=torch.device("cpu")))


def test_dump_outputs_writes_all_or_a_fixed_sample_of_windows(tmp_path, monkeypatch):
    import bench
    x = torch.arange(10 * 3 * 4, dtype=torch.float32).reshape(10, 3, 4, 1)
    info = bench.dump_outputs(str(tmp_path / "all"), x)
    np.testing.assert_array_equal(np.load(tmp_path / "all" / "x.npy"), x.numpy())
    assert info["x"]["shape"] == [10, 3, 4, 1] and info["x"]["dtype"] == "float32"
    row = 3 * 4 * 4
    monkeypatch.setattr(bench, "DUMP_BYTES", 4 * row + 5)              # room for 4 whole windows
    bench.dump_outputs(str(tmp_path / "a"), x)
    bench.dump_outputs(str(tmp_path / "b"), x)
    a, b = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "b" / "x.npy")
    assert a.shape == (4, 3, 4, 1) and a.dtype == np.float32
    np.testing.assert_array_equal(a, b)                                 # the same windows every time
    idx = (a[:, 0, 0, 0] // (3 * 4)).astype(int)                      # window i starts at element 12 i
    assert list(idx) == sorted(set(idx)) and all(0 <= i < 10 for i in idx)
    np.testing.assert_array_equal(a, x.numpy()[idx])
