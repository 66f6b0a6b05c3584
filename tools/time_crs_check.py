"""Times zk_crs_check against the calls next to it: JSON lines into profiles/crs_check.jsonl.

    python tools/time_crs_check.py [--shapes unity:10,unity:16,unity:20,integers:16] [--reps 7] [--out profiles/crs_check.jsonl]
                                   [--step-timeout 420]

Shapes: the chain circuit over the roots of unity at 2^10, 2^16 and 2^20 gates and over the integers 1..n at 2^16.  One child process
per shape, each under its own `timeout`, chained: a step that fails, faults or runs out of time ends the run there.  Per shape, in
one process: zk_setup once, one warm zk_prove (median of 3 after the proof that builds the tables), then zk_crs_check with a drawn
challenge -- the first call (which builds W's rows by gate and, for the integer roots, the interpolation tree on the QAP handle) and
the median and [min, max] of `reps` warm calls; `check_over_prove` is the warm median as a multiple of one proof's time.  Every line
carries the commit hash.  Times are host wall-clock around synchronous calls."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def commit_hash():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        path = os.path.join(ROOT, ".build_commit")
        return open(path).read().strip() if os.path.exists(path) else "unknown"


def timed(fn, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return out, times


def stats(prefix, times):
    return {prefix + "_ms_median": round(float(np.median(times)), 3), prefix + "_ms_min": round(min(times), 3), prefix + "_ms_max": round(max(times), 3)}


def run_shape(kind, log_n, reps, emit):
    import zksnark_rs_amd as zk
    from zksnark_rs_amd import SplitMix64, ints_to_limbs
    from zksnark_rs_amd.circuits import chain_rows, chain_weights
    ctx = zk.Context(0)
    rng = SplitMix64(8181 + log_n)
    n = 1 << log_n
    if kind == "unity":
        m, l, u, v, w = chain_rows(log_n)
        qap = ctx.qap_sparse(log_n, m, l, u, v, w)
        weights = chain_weights(log_n, rng.fr(), [rng.fr() for _ in range(n)])
    else:
        from test_integer_roots import chain_rows_integers, chain_weights_integers
        m, l, u, v, w = chain_rows_integers(n)
        qap = ctx.qap_sparse_integers(n, m, l, u, v, w)
        weights = chain_weights_integers(n, rng.fr(), [rng.fr() for _ in range(n)])
    td = ints_to_limbs([rng.fr() for _ in range(5)])
    crs, t_setup = timed(lambda: ctx.setup(qap, td), 1)
    r, s = rng.fr(), rng.fr()
    first_proof, t_first_proof = timed(lambda: ctx.prove(crs, qap, weights, r, s), 1)
    proof, t_prove = timed(lambda: ctx.prove(crs, qap, weights, r, s), 3)
    res, t_first = timed(lambda: ctx.crs_check(crs, qap), 1)
    res2, t_warm = timed(lambda: ctx.crs_check(crs, qap), reps)
    after = ctx.prove(crs, qap, weights, r, s)
    med = float(np.median(t_warm))
    emit(dict(tool="time_crs_check", commit=commit_hash(), kind=kind, gates=n, wires=m, public_inputs=l, reps=reps,
              ok=bool(res.ok and res2.ok), failed=res2.failed, flags=res2.flags, proof_unchanged=bool(proof == after == first_proof),
              setup_ms=round(t_setup[0], 3), first_prove_ms=round(t_first_proof[0], 3), first_check_ms=round(t_first[0], 3),
              check_over_prove=round(med / float(np.median(t_prove)), 3), **stats("prove", t_prove), **stats("check", t_warm)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="unity:10,unity:16,unity:20,integers:16")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crs_check.jsonl"))
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds each shape's child process may take")
    ap.add_argument("--shape", default=None, help="run one shape (kind:log_n) in this process (what the steps do)")
    args = ap.parse_args()
    if args.shape:
        kind, log_n = args.shape.split(":")
        with open(args.out, "a") as out:
            def emit(line):
                text = json.dumps(line)
                print(text, flush=True)
                out.write(text + "\n")
                out.flush()
            run_shape(kind, int(log_n), args.reps, emit)
        return 0
    open(args.out, "w").close()
    for shape in args.shapes.split(","):   # chained: nothing more is started on the GPU after a step that did not end well
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--shape", shape,
               "--reps", str(args.reps), "--out", args.out]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print("time_crs_check: step %s ended with status %d; stopping" % (shape, rc), file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
