"""bench.py's plain run and its options: a plain run times exactly --steps
launches in one loop and measures nothing beside the headline; --full brings
back the counted launches, the CPU baseline and the other configs (their
content is checked in tests/test_dist.py); --dump-outputs writes the last
timed launch's verdict words, which must equal the oracle's for the same
seeded batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
BENCH = os.path.join(os.path.dirname(HERE), "bench.py")


def test_plain_and_full_defaults():
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.runs == 1 and a.no_cpu and a.no_stats and a.others == "none"
    assert a.dump_outputs is None and not a.full
    f = bench.parse_args(["--steps", "7", "--full"])
    assert f.runs == 5 and not f.no_cpu and not f.no_stats and f.others is None
    assert bench.parse_args(["--full", "--runs", "2", "--no-cpu"]).runs == 2


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_verdicts(tmp_path):
    n = 3 * 4096 + 17        # several blocks, not a multiple of any tile
    cmd = [sys.executable, BENCH, "--gpus", "1", "--steps", "7", "--warmup", "2",
           "--batch", str(n), "--buffers", "3", "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(line) == 1, r.stdout[-2000:]
    d = json.loads(line[0])
    assert d["steps"] == 7 and d["warmup"] == 2 and d["runs"] == 1
    assert len(d["runs_ms_per_step"]) == 1 and d["ms_per_step"] == d["runs_ms_per_step"][0]
    assert d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "Mpps"
    assert d["higher_is_better"] is True and d["dtype"] == "u8"
    assert d["cpu_baseline"] is None
    assert "with_pktio_counters" not in d and "other_configs" not in d
    assert os.listdir(tmp_path / "out") == ["verdict.npy"]
    got = np.load(tmp_path / "out" / "verdict.npy")
    assert got.dtype == np.float64 and got.shape == (n,)

    import oracle
    from odp_amd import _lib as L
    from odp_amd import cls, gen
    opt = L.PKTIN_IPV4_CHKSUM | L.PKTIN_UDP_CHKSUM | L.PKTIN_TCP_CHKSUM
    cls.reset()
    p = cls.loop_pktio(pktin=opt)
    gen.build_c2_rules(cls, p)
    assert cls.pktio_start(p) == 0
    want = oracle.classify(cls.pktio_rules(p), gen.c2_frames(n), n, stride=64, opt=opt)["out"]
    cls.reset()
    np.testing.assert_array_equal(got, want.view(np.uint32).astype(np.float64))
