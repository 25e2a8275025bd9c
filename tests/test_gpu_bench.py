"""bench.py on the GPU at a small size, in this process: a plain run times the steps and nothing else,
--full adds its checks, and --dump-outputs writes the CRCs of the last timed step, the same for both
and equal to zlib over frames re-created on the host from the generator's definition."""
import json
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

FRAMES, L = 4099, 1518   # odd: no multiple of any tile; the whole output fits the dump cap


def _run(monkeypatch, capsys, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--frames-per-gpu", str(FRAMES), *argv])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    bench.main()
    lines = [x for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_and_full_runs_and_their_dumped_outputs(monkeypatch, capsys, tmp_path):
    plain = _run(monkeypatch, capsys, "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "p"))
    assert plain["steps"] == 3 and plain["warmup"] == 1 and plain["full"] is False
    assert plain["unit"] == "GiB/s" and plain["higher_is_better"] is True and plain["dtype"] == "u8"
    assert plain["ms_per_step"] > 0
    # both are rounded in the line: ms_per_step to 1e-4 ms of a step of at least 0.01 ms, value to 0.01
    assert plain["value"] == pytest.approx(FRAMES * L / (plain["ms_per_step"] * 1e-3) / bench.GIB, rel=1e-2, abs=0.01)
    assert plain["verified"] is None and plain["cpu_baseline"] is None and plain["configs"] is None
    assert "read_stream_gbs" not in plain["roofline"] and "profile_kernel_ms" not in plain["roofline"]

    full = _run(monkeypatch, capsys, "--steps", "2", "--warmup", "0", "--full", "--no-cpu",
                "--dump-outputs", str(tmp_path / "f"))
    assert full["steps"] == 2 and full["full"] is True and full["verified"] is True
    assert full["roofline"]["read_stream_gbs"] > 0 and full["roofline"]["dma_stream_gbs"] > 0

    a, b = np.load(tmp_path / "p" / "fcs.npy"), np.load(tmp_path / "f" / "fcs.npy")
    assert a.dtype == np.float64 and a.shape == (FRAMES,)
    assert np.array_equal(a, b)
    exp = [zlib.crc32(bench.splitmix_bytes(bench.SEED, i * L, L).tobytes()) for i in range(FRAMES)]
    assert np.array_equal(a, np.array(exp, dtype=np.float64))
