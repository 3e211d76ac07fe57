"""bench.py's plain run on one GPU: the headline line only (nothing that
--full adds), --steps honoured, and --dump-outputs writing the last timed
step's output -- the forward NTT of the seeded input -- checked against the C
oracle at the sampled indices and over the whole vector (block sums)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG_N = 21  # 2^21 elements: more than the 2^20-element sample


def test_plain_run_is_headline_only_and_dumps_the_ntt(tmp_path):
    from multilinear_amd import device as D
    from oracle import coracle
    from oracle import field as F

    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
                        "--warmup", "1", "--spinup-s", "0", "--log-n", str(LOG_N), "--dump-outputs", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout + p.stderr[-2000:]
    d = json.loads(lines[0])
    assert d["full"] is False and d["steps"] == 3 and d["n_gpus"] == 1
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["higher_is_better"] is True
    assert abs(d["value"] - (1 << LOG_N) * 1e3 / d["ms_per_step"]) <= 1e-9 * d["value"]
    assert d["unit"] == "field-elems/s" and d["dtype"].startswith("u128 mod M")
    assert d["roofline"]["kernel"] in d["kernels"]  # timed live inside the three steps
    for k in ("intt_ms", "fri_commit_ms", "sumcheck_ms", "pcs_prove_ms", "strong_ntt", "config5_log_code",
              "cpu_baseline", "cpu_baseline_all_cores", "valu_profile", "reference_test_points"):
        assert k not in d, k
    # the dumped output against the oracle's NTT of the same seeded input
    x = D.from_device(D.random_device(1 << LOG_N, 1000, 0))
    want = coracle.ntt(x, LOG_N, F.pow_2_generator(LOG_N))
    files = {f: np.load(out / f) for f in sorted(os.listdir(out))}
    assert sorted(files) == ["ntt_out.npy", "ntt_out_block_sums.npy", "ntt_out_index.npy"]
    assert all(v.dtype == np.float64 for v in files.values())
    assert sum(v.nbytes for v in files.values()) <= 64 * 10**6
    idx = files["ntt_out_index.npy"].astype(np.int64)
    assert idx.shape == (1 << 20,)
    assert np.array_equal(files["ntt_out.npy"], want[idx].astype(np.float64))
    sums = want.astype(np.uint64).reshape(4096, -1, 4).sum(1)
    assert np.array_equal(files["ntt_out_block_sums.npy"], sums.astype(np.float64))
