"""The exact code path bench.py times, checked word for word against the oracle.

bench.HMultWorkload is the bench's own workload object (not a copy of it): N=2^16, the C2 chain
(44 data limbs + the special prime), L = 44, 32 independent HMults per step issued as 4
mhe_hmult_batch calls of 8 entries (the relin key stream shared through the XCD-grouped entries of
k_ks_row_mac), the prepared key format (residues as doubles), the calls dealt round robin over 4 HIP streams.
One step runs as the bench runs it; every one of the 32 outputs must equal the oracle's HMult
(SEAL/evaluator.cpp:673-814 multiply, :2281-2525 relinearize, util/rns.cpp:737-808 rescale) on the
same inputs and the SEAL-layout key."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("key_format", ["prepared", "seal"])
def test_bench_timed_path_vs_oracle(key_format):
    import torch

    sys.path.insert(0, ROOT)
    import bench
    import oracle as O

    dev = torch.device("cuda", 0)
    w = bench.HMultWorkload(dev, rank=0, limbs=44, batch=32, group=8, streams=4, key_format=key_format,
                            keep_host=True)
    assert [c[1] for c in w.call_streams()] == [8, 8, 8, 8] and sorted({c[2] for c in w.call_streams()}) == [0, 1, 2, 3]
    if key_format == "prepared":
        assert w.eng.key_is_prepared(w.key)
    w.step()
    torch.cuda.synchronize(dev)
    got = w.host(w.out)
    oc = O.Context(bench.LOG_N, w.moduli)
    want, _ = oc.hmult_batch(np.ascontiguousarray(w.host(w.a)), np.ascontiguousarray(w.host(w.b)), w.key_host,
                             threads=min(16, os.cpu_count() or 1))
    bad = [i for i in range(w.B) if not np.array_equal(got[i], want[i])]
    assert not bad, f"HMult entries {bad} differ from the oracle"
    # a second step over the same buffers gives the same words (no state carried between steps)
    w.step()
    torch.cuda.synchronize(dev)
    assert np.array_equal(w.host(w.out), got)
    # and the bench's own rank-0 check passes on these outputs
    res = bench.check_timed_outputs(w, [0, 11, 19, 30], 4)
    assert res["entries"] == [0, 11, 19, 30] and len(res["calls_streams"]) == 4


def test_bench_plain_run_and_dump_outputs(tmp_path):
    """A plain `bench.py` run (no --full) at a small shape: --steps sets the timed steps, the line
    carries the headline keys with value = HMults per second of those steps and none of the --full
    legs, and --dump-outputs writes the last step's outputs: float64, the seeded sample
    (bench.dump_sample_index; 8 x 2 x 5 x 2^16 words is above DUMP_WORDS, so the sampling path runs),
    word for word what the same workload leaves in its output buffers when built again here."""
    import json
    import subprocess

    import torch

    sys.path.insert(0, ROOT)
    import bench

    limbs, batch, group, streams, steps = 6, 8, 4, 2, 2
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--limbs", str(limbs), "--batch", str(batch), "--hmult-group", str(group),
                        "--streams", str(streams), "--dump-outputs", str(tmp_path / "dump")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["warmup"] == 1 and line["unit"] == "HMult/s" and line["higher_is_better"]
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(batch / (line["ms_per_step"] * 1e-3), rel=1e-3)
    for key in ("timed_output_check", "roofline", "valu_roofline", "hmult_roofline", "resnet20", "cpu_baseline"):
        assert key not in line
    assert sorted(os.listdir(tmp_path / "dump")) == ["hmult_out.npy"]
    got = np.load(tmp_path / "dump" / "hmult_out.npy")
    assert got.dtype == np.float64 and got.shape == (bench.DUMP_WORDS,)

    dev = torch.device("cuda", 0)
    w = bench.HMultWorkload(dev, rank=0, limbs=limbs, batch=batch, group=group, streams=streams)
    w.step()
    torch.cuda.synchronize(dev)
    flat = w.host(w.out).reshape(-1)
    idx = bench.dump_sample_index(flat.size)
    assert idx is not None and idx.size == bench.DUMP_WORDS and 0 <= idx[0] and idx[-1] < flat.size
    want = flat[idx]
    assert int(want.max()) < 2**52  # so the float64 copy is exact
    assert np.array_equal(got, want.astype(np.float64))
    w.eng.close()
