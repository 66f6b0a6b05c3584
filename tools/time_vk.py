"""Times the verifying-key calls against the CRS calls they mirror: JSON lines into profiles/vk.jsonl.

    python tools/time_vk.py [--sizes 1,4096,65536] [--reps 7] [--out profiles/vk.jsonl] [--step-timeout 420]

Circuits: the 2^10-gate chain (l = 2 public inputs) and the generated program with 257 `verify` wires.  One child process per
circuit, each under its own `timeout`, chained: a step that fails, faults or runs out of time ends the run there.  Per circuit:
  (a) kind "verify_batch": zk_vk_verify_batch alternated with zk_verify_batch on the same proofs, call by call, for every N --
      median and spread (min, max) of `reps` warm calls each, and `verdicts_match` (both calls and the distinct proofs' zk_verify)
  (b) kind "input_sums": zk_vk_input_sums with tables = 0 and tables = 1 on the same rows (`verdicts_match`: the words are equal)
  (c) kind "key": zk_vk_from_crs + byte form on the host; the bind (upload of the constants) and the table build (allocation +
      k_vk_table) each timed directly over `reps` fresh keys, through input-sum calls on a row with no inputs
  (d) kind "verify": zk_vk_verify against zk_verify, ms per proof (`verdicts_match`: the verdicts are equal)
Times are host wall-clock around synchronous calls, transfers included."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def timed(fn, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return out, times


def stats(prefix, times):
    return {prefix + "_ms_median": round(float(np.median(times)), 3), prefix + "_ms_min": round(min(times), 3), prefix + "_ms_max": round(max(times), 3)}


def run_circuit(which, sizes, reps, emit):
    import zksnark_rs_amd as zk
    from zksnark_rs_amd import SplitMix64
    from time_verify_batch import chain_circuit, wide_circuit, distinct_proofs
    ctx = zk.Context(0)
    rng = SplitMix64(7171)
    name, crs, qap, weights, l = (chain_circuit if which == "chain" else wide_circuit)(ctx, rng)
    rows_d, proofs_d = distinct_proofs(ctx, crs, qap, weights, l, rng)
    d = len(proofs_d)
    base = dict(tool="time_vk", circuit=name, public_inputs=l, reps=reps)

    # (c) the key: host side, then the first batch call of a fresh key (upload + tables) against the next one
    t0 = time.perf_counter()
    key = ctx.verifying_key(crs)
    from_crs_ms = (time.perf_counter() - t0) * 1e3
    blob = key.to_bytes()
    _, create = timed(lambda: zk.VerifyingKey.from_bytes(blob), 5)
    fresh = zk.VerifyingKey.from_bytes(blob)
    one_row, one_proof = rows_d[:1], proofs_d[:1]
    t0 = time.perf_counter()
    first = fresh.verify_batch(ctx, one_row, one_proof)
    first_ms = (time.perf_counter() - t0) * 1e3
    _, warm = timed(lambda: fresh.verify_batch(ctx, one_row, one_proof), reps)
    # bind (upload of the constants) and table build timed directly, over fresh keys: a row with NO inputs leaves the sum kernel
    # nothing to add, so a call is its fixed cost (measured warm, subtracted) plus the bind, or plus allocation and k_vk_table
    none = np.zeros((1, 0, 4), dtype=np.uint64)
    binds, builds = [], []
    for _ in range(reps):
        k2 = zk.VerifyingKey.from_bytes(blob)
        _, t_bind = timed(lambda: k2.input_sums(ctx, none, tables=False), 1)
        _, t_idle0 = timed(lambda: k2.input_sums(ctx, none, tables=False), 3)
        _, t_build = timed(lambda: k2.input_sums(ctx, none, tables=True), 1)
        _, t_idle1 = timed(lambda: k2.input_sums(ctx, none, tables=True), 3)
        binds.append(t_bind[0] - float(np.median(t_idle0)))
        builds.append(t_build[0] - float(np.median(t_idle1)))
        k2.close()
    emit(dict(base, kind="key", key_bytes=len(blob), table_bytes=l * 64 * 15 * 64, from_crs_ms=round(from_crs_ms, 3),
              first_call_ms=round(first_ms, 3),
              verdicts_match=bool(np.array_equal(first, ctx.verify_batch(crs, one_row, one_proof))),
              **stats("from_bytes", create), **stats("warm_call", warm), **stats("bind", binds), **stats("table_build", builds)))

    # (d) one proof on the host
    single_vk, t_vk = timed(lambda: [key.verify(rows_d[j], proofs_d[j].tobytes()) for j in range(d)], 1)
    single, t_crs = timed(lambda: [ctx.verify(crs, rows_d[j], proofs_d[j].tobytes()) for j in range(d)], 1)
    emit(dict(base, kind="verify", proofs=d, zk_vk_verify_ms_per_proof=round(t_vk[0] / d, 3), zk_verify_ms_per_proof=round(t_crs[0] / d, 3),
              accepted=int(sum(single)), verdicts_match=single_vk == single))

    for n in sizes:
        idx = np.arange(n) % d
        rows, proofs = np.ascontiguousarray(rows_d[idx]), np.ascontiguousarray(proofs_d[idx])
        # (a) alternated, call by call
        got_vk, got_crs = key.verify_batch(ctx, rows, proofs), ctx.verify_batch(crs, rows, proofs)      # warm-up
        t_vk, t_crs = [], []
        same = True
        for _ in range(reps):
            a, t = timed(lambda: key.verify_batch(ctx, rows, proofs), 1)
            t_vk += t
            b, t = timed(lambda: ctx.verify_batch(crs, rows, proofs), 1)
            t_crs += t
            same = same and np.array_equal(a, got_vk) and np.array_equal(b, got_crs)
        match = bool(same and np.array_equal(got_vk, got_crs) and np.array_equal(got_vk, np.array(single)[idx]))
        med_vk, med_crs = float(np.median(t_vk)), float(np.median(t_crs))
        emit(dict(base, kind="verify_batch", n=n, distinct_proofs=d, accepted=int(got_vk.sum()), verdicts_match=match,
                  vk_over_crs=round(med_vk / med_crs, 4), **stats("vk_call", t_vk), **stats("crs_call", t_crs)))
        # (b) the input sums alone
        s1, s0 = key.input_sums(ctx, rows, tables=True), key.input_sums(ctx, rows, tables=False)        # warm-up
        t_1, t_0 = [], []
        for _ in range(reps):
            _, t = timed(lambda: key.input_sums(ctx, rows, tables=True), 1)
            t_1 += t
            _, t = timed(lambda: key.input_sums(ctx, rows, tables=False), 1)
            t_0 += t
        emit(dict(base, kind="input_sums", n=n, window_bits=4, verdicts_match=bool(np.array_equal(s0, s1)),
                  tables_over_bits=round(float(np.median(t_1)) / float(np.median(t_0)), 4), **stats("tables", t_1), **stats("bits", t_0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,4096,65536")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vk.jsonl"))
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds each circuit's child process may take")
    ap.add_argument("--circuit", choices=("chain", "wide"), default=None, help="run one circuit in this process (what the steps do)")
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    if args.circuit:
        with open(args.out, "a") as out:
            def emit(line):
                text = json.dumps(line)
                print(text, flush=True)
                out.write(text + "\n")
                out.flush()
            run_circuit(args.circuit, sizes, args.reps, emit)
        return 0
    open(args.out, "w").close()
    for which in ("chain", "wide"):   # chained: nothing more is started on the GPU after a step that did not end well
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--circuit", which,
               "--sizes", args.sizes, "--reps", str(args.reps), "--out", args.out]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print("time_vk: step %s ended with status %d; stopping" % (which, rc), file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
