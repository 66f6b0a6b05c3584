"""Times zk_verify_batch_all against zk_verify_batch on the same proofs in the same process: one JSON line per (circuit, N).

    python tools/time_verify_batch_all.py [--circuits chain,wide] [--chain-sizes ...] [--wide-sizes ...] [--reps 7] [--out FILE]

Circuits: the 2^10-gate chain (l = 2 public inputs) at N = 1, 16, 256, 4096, 65536, 2^18, 2^20 and a generated .zk program
with 257 `verify` wires at N = 1, 256, 4096, 65536.  A batch of N cycles through 32 distinct honest proofs.  After one warm-up
call of each, the two calls alternate `reps` times; per line: median, min and max of both call times, the ratio of the
medians, whether the [min, max] ranges are disjoint, and `verdict_match`: verify_batch_all == all(verify_batch) on that input.
Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this tool."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import zksnark_rs_amd as zk  # noqa: E402
from zksnark_rs_amd import SplitMix64  # noqa: E402
from time_verify_batch import chain_circuit, wide_circuit  # noqa: E402


def honest_proofs(ctx, crs, qap, weights, l, rng, count=32):
    x = np.ascontiguousarray(weights[1:1 + l])
    proofs = [np.frombuffer(ctx.prove(crs, qap, weights, rng.fr(), rng.fr()), dtype=np.uint8) for _ in range(count)]
    return np.repeat(x[None], count, axis=0), np.stack(proofs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--circuits", default="chain,wide")
    ap.add_argument("--chain-sizes", default="1,16,256,4096,65536,262144,1048576")
    ap.add_argument("--wide-sizes", default="1,256,4096,65536")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = zk.Context(0)
    rng = SplitMix64(7171)
    out = open(args.out, "w") if args.out else None
    plan = {"chain": (chain_circuit, args.chain_sizes), "wide": (wide_circuit, args.wide_sizes)}
    for key in args.circuits.split(","):
        make, sizes = plan[key]
        name, crs, qap, weights, l = make(ctx, rng)
        rows_d, proofs_d = honest_proofs(ctx, crs, qap, weights, l, rng)
        d = len(proofs_d)
        for n in [int(s) for s in sizes.split(",") if s]:
            idx = np.arange(n) % d
            rows, proofs = np.ascontiguousarray(rows_d[idx]), np.ascontiguousarray(proofs_d[idx])
            z = np.frombuffer(os.urandom(16 * n), dtype=np.uint64).reshape(n, 2).copy()
            z[(z == 0).all(axis=1), 0] = 1
            got_all = ctx.verify_batch_all(crs, rows, proofs, z)     # warm-up (and the verdicts compared below)
            got = ctx.verify_batch(crs, rows, proofs)
            t_all, t_one = [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                again_all = ctx.verify_batch_all(crs, rows, proofs, z)
                t_all.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                again = ctx.verify_batch(crs, rows, proofs)
                t_one.append((time.perf_counter() - t0) * 1e3)
                assert again_all == got_all and np.array_equal(again, got)
            med_all, med_one = float(np.median(t_all)), float(np.median(t_one))
            line = dict(tool="time_verify_batch_all", circuit=name, public_inputs=l, n=n, distinct_proofs=d, reps=args.reps,
                        all_ms_median=round(med_all, 3), all_ms_min=round(min(t_all), 3), all_ms_max=round(max(t_all), 3),
                        batch_ms_median=round(med_one, 3), batch_ms_min=round(min(t_one), 3), batch_ms_max=round(max(t_one), 3),
                        all_per_s=round(n / med_all * 1e3, 1), batch_per_s=round(n / med_one * 1e3, 1),
                        speedup=round(med_one / med_all, 3), ranges_disjoint=bool(max(t_all) < min(t_one) or max(t_one) < min(t_all)),
                        verdict=bool(got_all), verdict_match=bool(got_all == bool(got.all())))
            print(json.dumps(line), flush=True)
            if out:
                out.write(json.dumps(line) + "\n")
                out.flush()
    if out:
        out.close()


if __name__ == "__main__":
    main()
