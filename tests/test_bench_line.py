"""bench.py's plain line (the headline only) and --dump-outputs, on the GPU."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("cpu_baseline", "fp32_iq_path", "block_series", "end_to_end", "flex_chain", "ingest_8bit", "other_geometries",
             "north_star_shape", "group_path")


def _bench(out_dir, *extra):
    r = subprocess.run(["python3", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "2", "--settle-seconds", "0",
                        "--block-log2", "25", "--dump-outputs", str(out_dir)] + list(extra),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_line_and_dumped_outputs_match_a_verified_full_run(tmp_path):
    """A plain run times exactly --steps launches and carries the headline, none of --full's extras; its dump is the last timed
    launch's PCM (a fixed sample of columns: 64 channels x 2^25 / 96 outputs is over the size cap), the same on a --full run of the
    same arguments, whose self-check holds that launch bit-exact against the oracle."""
    plain = _bench(tmp_path / "plain")
    for k in HEADLINE:
        assert plain.get(k) is not None, k
    assert plain["steps"] == 6 and plain["roofline"]["launches"] == 6 and plain["ms_per_step"] > 0.0
    assert plain["verified"] is None and plain["roofline"]["board_sample"] is None
    assert not [k for k in FULL_ONLY if k in plain], plain.keys()
    pcm = np.load(tmp_path / "plain" / "pcm.npy")
    assert pcm.dtype == np.float32 and pcm.shape[0] == 64 and 0 < pcm.nbytes <= 64 << 20, pcm.shape
    assert np.array_equal(pcm, np.round(pcm)) and np.abs(pcm).max() <= 32768 and np.abs(pcm).max() > 0

    full = _bench(tmp_path / "full", "--full", "--no-cpu-baseline", "--no-fp32", "--no-series", "--no-chain")
    assert full["verified"] is True, full["verification"]
    assert np.array_equal(np.load(tmp_path / "full" / "pcm.npy"), pcm)
