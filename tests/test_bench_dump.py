"""bench.py --dump-outputs: dump_outputs writes each array exactly as float32 / float64, cuts an array over its share
of the budget to the same seeded rows every time, and keeps all files together under 64 MB. The command line offers
--full and --dump-outputs, and refuses options that only mean something with --full."""
import os
import subprocess
import sys

import numpy as np
import torch

import bench

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_dtypes_exact_values_and_rank_suffix(tmp_path):
    rng = np.random.default_rng(1)
    arrays = {
        "f32": rng.normal(size=(5, 3)).astype(np.float32),
        "f64": rng.normal(size=(4, 3, 3)),
        "i32": np.array([0, -1, 2**31 - 1], dtype=np.int32),
        "u32": np.array([[0, 2**32 - 1]], dtype=np.uint32),
        "u8": np.array([0, 1, 255], dtype=np.uint8),
        "flag": np.array([True, False]),
        "tensor": torch.arange(6, dtype=torch.int32).reshape(3, 2),
        "f16": torch.tensor([0.5, -2.0, 65504.0], dtype=torch.float16),
        "bf16": torch.tensor([0.5, -2.0, 3.0e38], dtype=torch.bfloat16),
    }
    bench.dump_outputs(str(tmp_path), arrays)
    want = {"f32": np.float32, "f64": np.float64, "i32": np.float64, "u32": np.float64, "u8": np.float32,
            "flag": np.float32, "tensor": np.float64, "f16": np.float32, "bf16": np.float32}
    for name, dt in want.items():
        got = np.load(tmp_path / f"{name}.npy")
        src = arrays[name].double().numpy() if isinstance(arrays[name], torch.Tensor) else arrays[name]
        assert got.dtype == dt and got.shape == src.shape
        assert np.array_equal(got.astype(np.float64), src.astype(np.float64))
    bench.dump_outputs(str(tmp_path), {"f32": arrays["f32"]}, rank=2)
    assert np.array_equal(np.load(tmp_path / "f32.rank2.npy"), arrays["f32"])


def test_dump_outputs_samples_large_arrays_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4000)  # two arrays: 2000 bytes each
    big = np.arange(1000 * 4, dtype=np.int32).reshape(1000, 4)  # 32 bytes per row as float64: 62 rows fit
    small = np.arange(10, dtype=np.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.shape == (62, 4) and np.array_equal(a, b)
    rows = (a[:, 0] // 4).astype(int)
    assert np.all(np.diff(rows) > 0) and np.array_equal(a, big[rows])  # whole rows of the source, in order
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 4000 + 2 * 128  # the budget plus the .npy headers
    bench.dump_outputs(str(tmp_path / "w"), {"big": big, "small": small}, rank=1, world=2)  # half the share each
    assert np.load(tmp_path / "w" / "big.rank1.npy").shape == (31, 4)


def test_dump_budget_is_under_64_mb():
    assert bench.DUMP_BUDGET_BYTES + 64 * 1024 < 64 * 1000 * 1000


def test_command_line_offers_full_and_dump_outputs():
    def run(*a):
        return subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *a], capture_output=True, text=True)

    usage = run("--help")
    assert usage.returncode == 0 and "--full" in usage.stdout and "--dump-outputs DIR" in usage.stdout
    for bad in (("--steps", "0"), ("--cpu-baseline-full",)):
        r = run(*bad)
        assert r.returncode == 2 and "usage:" in r.stderr
