"""bench.py's plain run and --dump-outputs: the plain run reports the timed steps only (the per-kernel / roofline / CPU-baseline
figures are behind --full), and --dump-outputs writes what the last timed step computed as float32 / float64 .npy files within
60 MiB, cut to a seeded sample of rows above that."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _clean_env():
    return {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}


def test_dump_outputs_dtypes_and_names(tmp_path):
    import bench
    arrays = {"a.half": torch.arange(6, dtype=torch.float16).reshape(3, 2), "b.f64": np.linspace(0, 1, 5),
              "c.u8": torch.ones(4, dtype=torch.uint8), "d.scalar": np.asarray(1.5, dtype=np.float64)}
    bench.dump_outputs(str(tmp_path / "out"), arrays)
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    assert sorted(got) == sorted(arrays)
    assert got["a.half"].dtype == np.float32 and got["a.half"].tolist() == [[0, 1], [2, 3], [4, 5]]
    assert got["b.f64"].dtype == np.float64 and np.array_equal(got["b.f64"], arrays["b.f64"])
    assert got["c.u8"].dtype == np.float32 and got["d.scalar"].dtype == np.float64


def test_dump_outputs_budget_keeps_a_seeded_row_sample(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 64 * 1024)
    big = np.arange(100_000, dtype=np.float32).reshape(10_000, 10)       # 400 KB
    other = np.arange(5_000, dtype=np.float64).reshape(2_500, 2)         # 40 KB
    tiny = np.ones(1, dtype=np.float32)
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "other": other, "tiny": tiny})
    sizes = 0
    for name in ("big", "other", "tiny"):
        x, y = np.load(tmp_path / "x" / f"{name}.npy"), np.load(tmp_path / "y" / f"{name}.npy")
        assert np.array_equal(x, y)                                      # same arguments, same rows
        sizes += x.nbytes
    assert sizes <= 64 * 1024
    b = np.load(tmp_path / "x" / "big.npy")
    assert b.shape[1] == 10 and 0 < b.shape[0] < 10_000
    rows = b[:, 0] / 10
    assert np.all(np.diff(rows) > 0) and np.array_equal(b, big[rows.astype(int)])   # whole rows, in order
    assert np.array_equal(np.load(tmp_path / "x" / "tiny.npy"), tiny)


def test_step_outputs_names_nets_buffer_and_objectives():
    import bench

    class Agent:
        act = torch.nn.Linear(3, 2)
        cri = torch.nn.Linear(3, 1)
        act_target = None

    class Buf:
        state = torch.zeros(4, 2, 3)
        reward = torch.zeros(3, 2)
        length = 3

    out = bench.step_outputs(Agent(), Buf(), (0.5, 2.0), prefix="ph.")
    assert sorted(out) == ["ph.act.bias", "ph.act.weight", "ph.buf.reward", "ph.buf.state", "ph.cri.bias", "ph.cri.weight",
                           "ph.update_objectives"]
    assert out["ph.update_objectives"].tolist() == [0.5, 2.0]


def test_steps_must_be_positive():
    p = subprocess.run([sys.executable, BENCH, "--steps", "0"], env=_clean_env(), capture_output=True, timeout=120)
    assert p.returncode == 2 and b"--steps must be at least 1" in p.stderr


@pytest.mark.gpu
def test_plain_run_reports_the_timed_steps_and_dumps_outputs(tmp_path):
    out_dir = tmp_path / "outputs"
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(out_dir)],
                       env=_clean_env(), capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    out = json.loads(lines[0])
    assert out["steps"] == 2 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "env-steps/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert abs(out["value"] - 819200 / (out["ms_per_step"] * 1e-3)) < 1e-3 * out["value"]
    assert not {"roofline", "roofline_env", "breakdown_ms", "cpu_baseline"} & set(out)    # --full only
    files = {f[:-4]: np.load(out_dir / f) for f in os.listdir(out_dir)}
    assert sum(os.path.getsize(out_dir / f) for f in os.listdir(out_dir)) <= 64 * 10 ** 6
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert files["buf.state"].shape == (51, 16384, 3) and files["buf.reward"].shape == (50, 16384)
    assert files["buf.done"][-1].all() and not files["buf.done"][:-1].all(axis=1).any()     # one 50-step episode per lane
    assert any(k.startswith("act.") for k in files) and any(k.startswith("cri.") for k in files)
    assert all(np.isfinite(a).all() for a in files.values())
    assert files["update_objectives"].shape == (2,)
