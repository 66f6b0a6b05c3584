"""Times zk_crs_contribute, its kernel and zk_crs_contribution_check against the calls next to them: JSON lines into
profiles/crs_contribute.jsonl.

    python tools/time_crs_contribute.py [--steps unity:10,unity:16,unity:20,kernel:20] [--reps 5] [--out profiles/crs_contribute.jsonl]
                                        [--step-timeout 420]

Steps, one child process each, each under its own `timeout`, chained: a step that fails, faults or runs out of time ends the run there.
  unity:K   the chain circuit over the roots of unity at 2^K gates.  Warm and alternated within the process: zk_setup on the QAP (what
            a party pays today for a CRS with a delta of its own) and zk_crs_contribute on that CRS (wall time, and the scale kernel's
            own time from the context's profile, name "g1_scale"); then zk_crs_contribution_check next to zk_crs_check on the new CRS.
  kernel:K  zk_g1_scale_batch against zk_g1_mul_batch (the scalar repeated: k_point_mul, the only way to do this before) on the same 2^K
            points, alternated: kernel time from the profile ("g1_scale" / "point_mul") and wall time for both, and their ratio.
Every line carries the commit hash.  Wall times are host clocks around synchronous calls; kernel times are HIP events on the stream."""
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
from time_crs_check import commit_hash, stats  # noqa: E402


def once(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def kernel_ms(ctx, name, fn):
    """(result, wall ms, the profile's total for `name` in ms) of one call"""
    ctx.profile_reset()
    out, wall = once(fn)
    return out, wall, ctx.profile().get(name, dict(total_ms=0.0))["total_ms"]


def run_unity(log_n, reps, emit):
    import zksnark_rs_amd as zk
    from zksnark_rs_amd import SplitMix64, ints_to_limbs
    from zksnark_rs_amd.circuits import chain_rows
    ctx = zk.Context(0)
    ctx.set_option("profile", 2)
    rng = SplitMix64(9191 + log_n)
    n = 1 << log_n
    m, l, u, v, w = chain_rows(log_n)
    qap = ctx.qap_sparse(log_n, m, l, u, v, w)
    td = ints_to_limbs([rng.fr() for _ in range(5)])
    crs, first_setup = once(lambda: ctx.setup(qap, td))
    (new, rec), first_contribute = once(lambda: ctx.crs_contribute(crs))
    t_setup, t_contribute, t_kernel = [], [], []
    for _ in range(reps):                       # alternated: both see the same clocks and the same neighbours
        _, t = once(lambda: ctx.setup(qap, td))
        t_setup.append(t)
        (new, rec), wall, k = kernel_ms(ctx, "g1_scale", lambda: ctx.crs_contribute(crs))
        t_contribute.append(wall)
        t_kernel.append(k)
    ok_first = ctx.crs_check(new, qap).ok      # builds what the first check builds on the QAP handle
    t_cc, t_check = [], []
    for _ in range(reps):
        res, t = once(lambda: ctx.crs_contribution_check(crs, new, rec))
        t_cc.append(t)
        full, t = once(lambda: ctx.crs_check(new, qap))
        t_check.append(t)
    points = (m - l - 1) + (n - 1)
    emit(dict(tool="time_crs_contribute", step="unity:%d" % log_n, commit=commit_hash(), gates=n, wires=m, public_inputs=l, reps=reps,
              points_scaled=points, ok=bool(res.ok and full.ok and ok_first and rec.verify()), first_setup_ms=round(first_setup, 3),
              first_contribute_ms=round(first_contribute, 3), kernel_us_per_point=round(1e3 * float(np.median(t_kernel)) / points, 4),
              contribute_over_setup=round(float(np.median(t_contribute)) / float(np.median(t_setup)), 3),
              contribution_check_over_crs_check=round(float(np.median(t_cc)) / float(np.median(t_check)), 3),
              **stats("setup", t_setup), **stats("contribute", t_contribute), **stats("scale_kernel", t_kernel),
              **stats("contribution_check", t_cc), **stats("crs_check", t_check)))


def run_kernel(log_n, reps, emit):
    import zksnark_rs_amd as zk
    from zksnark_rs_amd import SplitMix64, ints_to_limbs
    from zksnark_rs_amd.circuits import chain_rows
    ctx = zk.Context(0)
    ctx.set_option("profile", 2)
    rng = SplitMix64(9292 + log_n)
    n = 1 << log_n
    m, l, u, v, w = chain_rows(log_n)
    qap = ctx.qap_sparse(log_n, m, l, u, v, w)
    pts = ctx.crs_download(ctx.setup(qap, ints_to_limbs([rng.fr() for _ in range(5)])))["xi_g1"]      # n distinct points
    k = rng.fr()
    ks = np.tile(ints_to_limbs([k]), (n, 1))
    a = ctx.g1_scale_batch(pts[:1024], k)       # warm both code objects
    b = ctx.g1_mul_batch(pts[:1024], ks[:1024])
    w_scale, k_scale, w_mul, k_mul = [], [], [], []
    for _ in range(reps):
        a, wall, kern = kernel_ms(ctx, "g1_scale", lambda: ctx.g1_scale_batch(pts, k))
        w_scale.append(wall)
        k_scale.append(kern)
        b, wall, kern = kernel_ms(ctx, "point_mul", lambda: ctx.g1_mul_batch(pts, ks))
        w_mul.append(wall)
        k_mul.append(kern)
    emit(dict(tool="time_crs_contribute", step="kernel:%d" % log_n, commit=commit_hash(), points=n, reps=reps, equal=bool(np.array_equal(a, b)),
              scale_ns_per_point=round(1e6 * float(np.median(k_scale)) / n, 2), point_mul_ns_per_point=round(1e6 * float(np.median(k_mul)) / n, 2),
              point_mul_over_scale=round(float(np.median(k_mul)) / float(np.median(k_scale)), 3),
              **stats("scale_kernel", k_scale), **stats("point_mul_kernel", k_mul), **stats("scale_wall", w_scale), **stats("point_mul_wall", w_mul)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="unity:10,unity:16,unity:20,kernel:20")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crs_contribute.jsonl"))
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds each step's child process may take")
    ap.add_argument("--step", default=None, help="run one step in this process (what the steps do)")
    args = ap.parse_args()
    if args.step:
        what, log_n = args.step.split(":")
        with open(args.out, "a") as out:
            def emit(line):
                text = json.dumps(line)
                print(text, flush=True)
                out.write(text + "\n")
                out.flush()
            (run_kernel if what == "kernel" else run_unity)(int(log_n), args.reps, emit)
        return 0
    open(args.out, "w").close()
    for step in args.steps.split(","):   # chained: nothing more is started on the GPU after a step that did not end well
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step,
               "--reps", str(args.reps), "--out", args.out]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print("time_crs_contribute: step %s ended with status %d; stopping" % (step, rc), file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
