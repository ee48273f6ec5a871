"""bench.py's plain run (no --full): the headline line alone, and --dump-outputs. The arrays it
writes are what the last timed step computed, so on the smallest configuration (c1: 4 peers,
1,024 events) they must equal the CPU oracle's results on the same seeded trace, value for value."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_line_and_dumped_outputs(tmp_path):
    import bench
    import hgref
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--config", "c1", "--dump-outputs", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["full"] is False and d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "consensus-ordered events/s" and d["higher_is_better"] is True and d["dtype"] == "int32"
    assert d["ms_per_step"] > 0
    # value = ordered events of the timed steps over their time
    per_step = d["config"]["ordered_events_per_step_per_gpu"]
    assert per_step > 0 and d["value"] == pytest.approx(per_step / (d["ms_per_step"] * 1e-3), rel=1e-9)
    # nothing of the --full legs in a plain line
    for k in ("roofline", "kernels_per_pass", "checks", "cpu_baseline", "hbm_resident", "packed_columns",
              "ingest_sha256", "ingest_p256_verify", "insert_verify", "chunked_sync", "sharded"):
        assert k not in d, k

    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert sorted(got) == sorted(d["outputs"]["arrays"])
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) == d["outputs"]["bytes"] <= 64 * 1000 * 1000
    tr, G = bench.make_trace("c1", 0)
    want = hgref.oracle_run(tr).results()
    assert np.array_equal(got["event_sample"], np.arange(tr.E))            # (below DUMP_SAMPLE: every event)
    assert np.array_equal(got["order_sample"], np.arange(len(want["order"])))
    assert len(want["order"]) == per_step
    for name, key in (("round", "round"), ("witness", "witness"), ("famous", "famous"), ("round_received", "rr"),
                      ("order", "order")):
        assert np.array_equal(got[name].astype(np.int64), np.asarray(want[key], np.int64)), name
    cts = (got["consensus_timestamp_hi32"].astype(np.int64) << 32) | got["consensus_timestamp_lo32"].astype(np.int64)
    assert np.array_equal(cts, want["cts"])
    assert got["per_graph"].tolist() == [[len(want["order"]), want["last_round"],
                                          -1 if want["lcr"] is None else want["lcr"], want["lcre"],
                                          want["consensus_tx"], len(want["blocks"])]]
    assert got["checksums"][:2].tolist() == [tr.E, len(want["order"])]
