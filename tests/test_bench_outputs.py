"""bench.py's plain line and its --dump-outputs files: a plain run prints the headline fields only (everything else is behind
--full), and the files hold what the last timed step computed for a fixed seeded sample of the pairs, as float arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = 200_000
NAMES = ("pair_index", "offsets", "scores", "cigar_len", "status", "cigars", "score_max")


class _Batch:
    """The result arrays of a DeviceBatch, on the host."""

    def __init__(self, n, stride, seed=3):
        g = torch.Generator().manual_seed(seed)
        self.n, self.cigar_stride = n, stride
        self.offsets = torch.randint(0, 100, (n,), generator=g, dtype=torch.int32)
        self.scores = torch.randint(-1000, 30000, (n, 6), generator=g, dtype=torch.int32)
        self.cigars = torch.randint(1, 256, (n, stride), generator=g, dtype=torch.uint8)
        self.cigar_len = torch.randint(0, stride + 1, (n,), generator=g, dtype=torch.int32)
        self.status = torch.zeros(n, dtype=torch.int32)


def test_dump_outputs_sample_and_files(tmp_path):
    import bench

    a, b = bench.dump_sample(10_000_000), bench.dump_sample(10_000_000)
    assert len(a) == bench.DUMP_SAMPLE_PAIRS and (a == b).all() and (np.diff(a) > 0).all() and a[-1] < 10_000_000
    assert (bench.dump_sample(100) == np.arange(100)).all()

    bt = _Batch(50_000, 64)
    bench.dump_outputs(str(tmp_path / "d"), bt, bt.scores[:, 2], bt.n)
    got = {n: np.load(tmp_path / "d" / f"{n}.npy") for n in NAMES}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    idx = got["pair_index"].astype(np.int64)
    assert (idx == bench.dump_sample(bt.n)).all()
    assert (got["offsets"] == bt.offsets.numpy()[idx]).all() and (got["scores"] == bt.scores.numpy()[idx]).all()
    assert (got["score_max"] == bt.scores.numpy()[idx, 2]).all() and (got["status"] == 0).all()
    ln = bt.cigar_len.numpy()[idx]
    assert (got["cigar_len"] == ln).all()
    cg = bt.cigars.numpy()[idx]
    for k in range(0, len(idx), 97):   # the CIGAR bytes, zero past the CIGAR
        assert (got["cigars"][k, : ln[k]] == cg[k, : ln[k]]).all() and (got["cigars"][k, ln[k]:] == 0).all()

    # long CIGAR slots: fewer pairs, never more than 64 MB in all
    bt = _Batch(40_000, 2048)
    bench.dump_outputs(str(tmp_path / "long"), bt, None, bt.n)
    files = os.listdir(tmp_path / "long")
    assert "score_max.npy" not in files
    assert sum(os.path.getsize(tmp_path / "long" / f) for f in files) <= bench.DUMP_MAX_BYTES


def _plain(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--pairs", str(PAIRS), "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600, cwd=ROOT,
                       env={k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")})
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_line_and_outputs(tmp_path):
    import oracle_lib as ol
    from mgl_amd import device_batch

    d = _plain(tmp_path / "a")
    assert d["unit"] == "GCUPS" and d["higher_is_better"] is True and d["value"] > 0 and d["dtype"] in ("int16", "int32")
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["cigar_overflows"] == 0
    assert abs(d["value"] - PAIRS * 256 * 150 / (d["ms_per_step"] / 1e3) / 1e9) < 0.01 * d["value"]
    for key in ("roofline", "kernel_ms", "cpu_baseline", "two_steps_in_flight", "pcie_inclusive", "tl1000", "secondary"):
        assert key not in d, key                # --full only
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in NAMES}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    # the same arguments, the same inputs: a second run writes the same arrays
    _plain(tmp_path / "b")
    for n in NAMES:
        assert np.array_equal(got[n], np.load(tmp_path / "b" / f"{n}.npy")), n
    # ... and they are the CPU checker's answers for those pairs of the seeded workload
    idx = got["pair_index"].astype(np.int64)
    assert len(idx) == 16384 and (got["status"] == 0).all() and (got["score_max"] == got["scores"][:, 2]).all()
    b = device_batch.window_batch(42, PAIRS, torch.device("cuda", 0))
    sel = idx[::8]
    ts, qs = b.host_pairs(sel.tolist())
    off, sc, cg = ol.oracle_align_batch(ts, qs, (200, -150, 260, 11), ol.SOFTCLIP, nthreads=8)
    assert (got["offsets"][::8] == off).all() and (got["scores"][::8] == sc).all()
    ln = got["cigar_len"][::8].astype(np.int64)
    assert [bytes(got["cigars"][k * 8, : ln[k]].astype(np.uint8)).decode() for k in range(len(sel))] == cg
