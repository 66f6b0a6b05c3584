"""Times zk_verify_batch against zk_verify: one JSON line per (circuit, N).

    python tools/time_verify_batch.py [--sizes 1,16,256,4096,65536] [--reps 7] [--out FILE]

Circuits: the 2^10-gate chain (l = 2 public inputs) and a generated .zk program with 257 `verify` wires.  A batch of N cycles
through a few dozen distinct proofs, honest and tampered (wrong input, flipped byte, A and C swapped).  Per line: median and
spread (min, max) of the call time over `reps` warm calls, verifications/s at the median, zk_verify's ms per proof measured in
the same process, and `verdicts_match`: every verdict equals zk_verify's for the same distinct proof, and zk_verify run again on
a sample of 64 entries (all when N < 64) agrees.
Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this tool."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import zksnark_rs_amd as zk  # noqa: E402
from zksnark_rs_amd import ints_to_limbs, SplitMix64  # noqa: E402


def distinct_proofs(ctx, crs, qap, weights, l, rng, honest=16):
    """(rows (D, l, 4), proofs (D, 259)) of `honest` proofs plus as many tampered ones"""
    x = np.ascontiguousarray(weights[1:1 + l])
    rows, proofs = [], []
    for k in range(honest):
        p = ctx.prove(crs, qap, weights, rng.fr(), rng.fr())
        rows.append(x); proofs.append(p)
        bad_x = x.copy(); bad_x[k % l, 0] ^= np.uint64(1)
        flip = bytearray(p); flip[1 + (k * 37) % 250] ^= 1 << (k % 8)
        tampered = [(bad_x, p), (x, bytes(flip)), (x, p[194:] + p[65:194] + p[:65])][k % 3]
        rows.append(tampered[0]); proofs.append(tampered[1])
    return np.stack(rows), np.stack([np.frombuffer(p, dtype=np.uint8) for p in proofs])


def chain_circuit(ctx, rng):
    from zksnark_rs_amd.circuits import chain_rows, chain_weights
    log_n = 10
    m, l, u, v, w = chain_rows(log_n)
    weights = chain_weights(log_n, rng.fr(), [rng.fr() for _ in range(1 << log_n)])
    qap = ctx.qap_sparse(log_n, m, l, u, v, w)
    crs = ctx.setup(qap, ints_to_limbs([rng.fr() for _ in range(5)]))
    return "chain_2^10", crs, qap, weights, l


def wide_circuit(ctx, rng):
    from test_gpu_verify_batch import wide_program
    from zksnark_rs_amd.circuit import Circuit
    c = Circuit(wide_program(256))
    weights = c.weights([rng.fr() for _ in range(c.n_in)])
    qap = c.qap_sparse(ctx)
    crs = ctx.setup(qap, ints_to_limbs([rng.fr() for _ in range(5)]))
    return "wide_%d_inputs" % c.input, crs, qap, weights, c.input


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,16,256,4096,65536")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    ctx = zk.Context(0)
    rng = SplitMix64(7070)
    out = open(args.out, "w") if args.out else None
    for make in (chain_circuit, wide_circuit):
        name, crs, qap, weights, l = make(ctx, rng)
        rows_d, proofs_d = distinct_proofs(ctx, crs, qap, weights, l, rng)
        d = len(proofs_d)
        t0 = time.perf_counter()
        single = [ctx.verify(crs, rows_d[j], proofs_d[j].tobytes()) for j in range(d)]
        verify_ms = (time.perf_counter() - t0) * 1e3 / d
        for n in sizes:
            idx = np.arange(n) % d
            rows, proofs = np.ascontiguousarray(rows_d[idx]), np.ascontiguousarray(proofs_d[idx])
            got = ctx.verify_batch(crs, rows, proofs)      # warm-up (also the verdicts checked below)
            times = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                again = ctx.verify_batch(crs, rows, proofs)
                times.append((time.perf_counter() - t0) * 1e3)
                assert np.array_equal(again, got)
            sample = np.unique(np.linspace(0, n - 1, min(n, 64)).astype(int))
            match = bool(np.array_equal(got, np.array(single)[idx])) and \
                all(bool(got[j]) == ctx.verify(crs, rows[j], proofs[j].tobytes()) for j in sample[:64])
            med = float(np.median(times))
            line = dict(tool="time_verify_batch", circuit=name, public_inputs=l, n=n, distinct_proofs=d, reps=args.reps,
                        call_ms_median=round(med, 3), call_ms_min=round(min(times), 3), call_ms_max=round(max(times), 3),
                        verifications_per_s=round(n / med * 1e3, 1), zk_verify_ms_per_proof=round(verify_ms, 3),
                        zk_verify_per_s=round(1e3 / verify_ms, 2), speedup_vs_zk_verify=round(n / med * verify_ms, 1),
                        accepted=int(got.sum()), verdicts_compared=n, zk_verify_rechecked=int(len(sample)), verdicts_match=match)
            print(json.dumps(line), flush=True)
            if out:
                out.write(json.dumps(line) + "\n")
                out.flush()
    if out:
        out.close()


if __name__ == "__main__":
    main()
