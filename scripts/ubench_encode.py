"""Encode timing at N = 2^16 on the ResNet chain (51 + 16x46 + 14x51 + special 51), HIP events on the
engine's stream, 8 full-slot real vectors per leg:

  host    8 calls of the host entry mhe_ckks_encode (pinned ring, one vector per launch sequence)
  dev8    one 8-entry mhe_ckks_encode_dev on the same vectors, already resident
  dev1x8  8 one-entry mhe_ckks_encode_dev calls

After --warmup passes of all three, --rounds interleaved rounds of --reps timed passes per leg.  One
JSON line per (leg, round) with the mean time of a pass, then one summary line per leg (median and
spread of its rounds, per vector).  The three legs' words are compared once, before timing.
--only LEG runs that leg alone (--reps passes), for a kernel trace.

    python scripts/ubench_encode.py [--limbs 25] [--rounds 3] [--reps 20] [--l1]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fhe-gpt-2_amd"))

import torch  # noqa: E402

import mhe  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--limbs", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--l1", action="store_true", help="give encode_dev the l1 bounds (no device size check)")
    ap.add_argument("--only", default=None, choices=["host", "dev8", "dev1x8"])
    a = ap.parse_args()
    log_n, n, B = 16, 1 << 16, 8
    bits = [51] + [46] * 16 + [51] * 14 + [51]
    eng = mhe.Engine(log_n, mhe.coeff_modulus_create(n, bits), device=0)
    L, scale = a.limbs, 2.0 ** 46
    rng = np.random.default_rng(2026)
    host_v = [rng.uniform(-1, 1, n // 2) for _ in range(B)]
    dev_v = [torch.from_numpy(v).to(eng.torch_device) for v in host_v]
    l1 = [float(np.abs(v).sum()) * (1 + 1e-9) for v in host_v] if a.l1 else None
    out_h = eng.empty(B, L, n)
    out_8 = eng.empty(B, L, n)
    out_1 = eng.empty(B, L, n)
    status = torch.empty(B, dtype=torch.int32, device=eng.torch_device)

    def host():
        for b in range(B):
            eng.encode(host_v[b], scale, L, out=out_h[b])

    def dev8():
        eng.encode_dev(dev_v, scale, L, out=out_8, l1_bounds=l1, status=status)

    def dev1x8():
        for b in range(B):
            eng.encode_dev(dev_v[b], scale, L, out=out_1[b], l1_bounds=None if l1 is None else l1[b:b + 1],
                           status=status[b:b + 1])

    legs = {"host": host, "dev8": dev8, "dev1x8": dev1x8}
    if a.only:
        for _ in range(a.reps):
            legs[a.only]()
        eng.synchronize()
        return
    for _ in range(a.warmup):
        for f in legs.values():
            f()
    eng.synchronize()
    same = bool(torch.equal(out_h, out_8) and torch.equal(out_h, out_1) and int(status.abs().sum()) == 0)
    print(json.dumps({"check": "host == dev8 == dev1x8 words, status 0", "ok": same}), flush=True)
    if not same:
        sys.exit(1)
    times = {k: [] for k in legs}
    for r in range(a.rounds):
        for name, f in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                f()
            e1.record()
            e1.synchronize()
            us = e0.elapsed_time(e1) * 1000.0 / a.reps
            times[name].append(us)
            print(json.dumps({"leg": name, "round": r, "us_per_8_vectors": round(us, 2)}), flush=True)
    for name, t in times.items():
        print(json.dumps({"leg": name, "limbs": L, "l1_bounds": bool(a.l1), "median_us_per_vector": round(float(np.median(t)) / B, 2),
                          "min_us_per_vector": round(min(t) / B, 2), "max_us_per_vector": round(max(t) / B, 2),
                          "rounds": a.rounds, "reps": a.reps}), flush=True)


if __name__ == "__main__":
    main()
