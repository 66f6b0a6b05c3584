"""Times the compressed proof form on the GPU: one JSON line per (call, N).

    python tools/time_proof_codec.py [--sizes 4096,65536] [--reps 7] [--out profiles/proof_codec.jsonl]

One process, the 2^10-gate chain proofs of tools/time_verify_batch.py (honest and tampered, cycled to N).  Per N:
  zk_proof_decompress_batch and zk_proof_compress_batch: median and [min, max] of `reps` warm calls, proofs/s at the median;
      verdicts_match: bytes and verdict of every entry equal the single host form's for the same distinct string.
  zk_verify_batch_compressed ALTERNATED with zk_verify_batch on the same proofs (one call of each per repetition, so both see
      the same clocks): both medians, their ratio; verdicts_match: the two verdict vectors are equal.
A tampered proof that is no canonical encoding compresses to 128 zero bytes, which both paths refuse."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import zksnark_rs_amd as zk  # noqa: E402
from zksnark_rs_amd import SplitMix64  # noqa: E402
from time_verify_batch import chain_circuit, distinct_proofs  # noqa: E402


def host_single(fn, entries):
    out = []
    for e in entries:
        try:
            out.append((True, fn(e.tobytes())))
        except zk.ZkError:
            out.append((False, None))
    return out


def timed(call, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = call()
        times.append((time.perf_counter() - t0) * 1e3)
    return res, times


def stats(prefix, times):
    return {prefix + "_ms_median": round(float(np.median(times)), 3), prefix + "_ms_min": round(min(times), 3),
            prefix + "_ms_max": round(max(times), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,65536")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = zk.Context(0)
    rng = SplitMix64(7070)
    name, crs, qap, weights, l = chain_circuit(ctx, rng)
    rows_d, proofs_d = distinct_proofs(ctx, crs, qap, weights, l, rng)
    d = len(proofs_d)
    packed_single = host_single(zk.proof_compress, proofs_d)
    packed_d = np.stack([np.frombuffer(c if ok else bytes(128), dtype=np.uint8) for ok, c in packed_single])
    plain_single = host_single(zk.proof_decompress, packed_d)
    lines = []
    for n in [int(s) for s in args.sizes.split(",")]:
        idx = np.arange(n) % d
        rows, proofs, packed = np.ascontiguousarray(rows_d[idx]), np.ascontiguousarray(proofs_d[idx]), np.ascontiguousarray(packed_d[idx])
        common = dict(tool="time_proof_codec", circuit=name, n=n, distinct_proofs=d, reps=args.reps)
        for call_name, fn, src, single, fill in (("zk_proof_decompress_batch", ctx.proof_decompress_batch, packed, plain_single, 0xFF),
                                                 ("zk_proof_compress_batch", ctx.proof_compress_batch, proofs, packed_single, 0)):
            fn(src)   # warm-up
            (out, ok), times = timed(lambda: fn(src), args.reps)
            match = all(bool(ok[j]) == single[idx[j]][0] and out[j].tobytes() == (single[idx[j]][1] if ok[j] else bytes([fill]) * out.shape[1])
                        for j in range(n))
            med = float(np.median(times))
            lines.append(dict(common, call=call_name, **stats("call", times), proofs_per_s=round(n / med * 1e3, 1), accepted=int(ok.sum()),
                              verdicts_match=bool(match)))
        ctx.verify_batch_compressed(crs, rows, packed)   # warm-up of both
        ctx.verify_batch(crs, rows, proofs)
        t_c, t_p = [], []
        for _ in range(args.reps):
            got_c, t = timed(lambda: ctx.verify_batch_compressed(crs, rows, packed), 1)
            t_c += t
            got_p, t = timed(lambda: ctx.verify_batch(crs, rows, proofs), 1)
            t_p += t
        med_c, med_p = float(np.median(t_c)), float(np.median(t_p))
        lines.append(dict(common, call="zk_verify_batch_compressed vs zk_verify_batch", **stats("compressed", t_c), **stats("plain", t_p),
                          compressed_per_s=round(n / med_c * 1e3, 1), plain_per_s=round(n / med_p * 1e3, 1),
                          compressed_over_plain_time=round(med_c / med_p, 4), accepted=int(got_c.sum()),
                          verdicts_match=bool(np.array_equal(got_c, got_p))))
    out = open(args.out, "w") if args.out else None
    for line in lines:
        print(json.dumps(line), flush=True)
        if out:
            out.write(json.dumps(line) + "\n")
    if out:
        out.close()


if __name__ == "__main__":
    main()
