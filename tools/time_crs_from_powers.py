"""Times zk_crs_from_powers next to zk_setup on the same QAP and splits it into its three parts: JSON lines into
profiles/crs_from_powers.jsonl.

    python tools/time_crs_from_powers.py [--steps unity:10,unity:16,unity:20,integers:10,integers:16] [--reps 3]
                                         [--out profiles/crs_from_powers.jsonl] [--step-timeout 420]

Steps, one child process each, each under its own `timeout`, chained: a step that fails, faults or runs out of time ends the run there.
  unity:K      the chain circuit over the roots of unity at 2^K gates
  integers:K   the chain circuit over the roots 1..2^K (the .zk front end's form; its Lagrange-basis arrays are part of the call)
The transcript is built from a drawn (alpha, beta, x) with zk_g1_mul_batch / zk_g2_mul_batch (not timed), the derived CRS is compared
with zk_setup's for (alpha, beta, 1, 1, x) ("equal"), and both calls are timed warm and alternated.  The parts come from the
context's profile (HIP events on the call's stream): "powers_lagrange" (the three Lagrange arrays; for the integer roots also lag2 and
lagS_t1), "powers_wire_points" (classification, products, k_wire_points) and "powers_xi_t".  Wall times are host clocks around the
synchronous calls and include the upload and the checks of the transcript.  Every line carries the commit hash."""
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
from time_crs_check import commit_hash, stats  # noqa: E402

PARTS = ("powers_lagrange", "powers_wire_points", "powers_xi_t")


def once(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def run(form, log_n, reps, emit):
    import zksnark_rs_amd as zk
    from zksnark_rs_amd import SplitMix64, ints_to_limbs
    from zksnark_rs_amd.circuits import chain_rows
    import powers_cases as pc
    ctx = zk.Context(0)
    ctx.set_option("profile", 2)
    rng = SplitMix64(9393 + log_n)
    n = 1 << log_n
    if form == "unity":
        m, l, u, v, w = chain_rows(log_n)
        qap = ctx.qap_sparse(log_n, m, l, u, v, w)
    else:
        from test_integer_roots import chain_rows_integers
        m, l, u, v, w = chain_rows_integers(n)
        qap = ctx.qap_sparse_integers(n, m, l, u, v, w)
    alpha, beta, x = rng.fr(), rng.fr(), rng.fr()
    td = pc.trapdoor(alpha, beta, x)
    want, first_setup = once(lambda: ctx.setup(qap, td))
    arrs = ctx.crs_download(want)
    p = pc.transcript(ctx.g1_mul_batch, ctx.g2_mul_batch, arrs["xi_g1"][0].copy(), arrs["xi_g2"][0].copy(), alpha, beta, x, n)
    derive = lambda: ctx.crs_from_powers(qap, p["tau_g1"], p["tau_g2"], p["alpha_tau_g1"], p["beta_tau_g1"], p["beta_g2"])   # noqa: E731
    got, first_derive = once(derive)
    mine = ctx.crs_download(got)
    equal = all(np.array_equal(mine[k], arrs[k]) for k in arrs)
    del got, mine
    t_setup, t_derive, parts = [], [], {k: [] for k in PARTS}
    for _ in range(reps):                       # alternated: both see the same clocks and the same neighbours
        _, t = once(lambda: ctx.setup(qap, td))
        t_setup.append(t)
        ctx.profile_reset()
        got, t = once(derive)
        t_derive.append(t)
        prof = ctx.profile()
        for k in PARTS:
            parts[k].append(prof.get(k, dict(total_ms=0.0))["total_ms"])
        del got
    nnz = int(u[0][-1] + v[0][-1] + w[0][-1])
    line = dict(tool="time_crs_from_powers", step="%s:%d" % (form, log_n), commit=commit_hash(), gates=n, wires=m, public_inputs=l,
                row_entries=nnz, reps=reps, equal=bool(equal), first_setup_ms=round(first_setup, 3), first_from_powers_ms=round(first_derive, 3),
                from_powers_over_setup=round(float(np.median(t_derive)) / float(np.median(t_setup)), 3),
                wire_points_us_per_wire=round(1e3 * float(np.median(parts["powers_wire_points"])) / m, 4),
                **stats("setup", t_setup), **stats("from_powers", t_derive))
    for k in PARTS:
        line.update(stats(k[len("powers_"):], parts[k]))
    emit(line)
    return 0 if equal else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="unity:10,unity:16,unity:20,integers:10,integers:16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crs_from_powers.jsonl"))
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds each step's child process may take")
    ap.add_argument("--step", default=None, help="run one step in this process (what the steps do)")
    args = ap.parse_args()
    if args.step:
        form, log_n = args.step.split(":")
        with open(args.out, "a") as out:
            def emit(line):
                text = json.dumps(line)
                print(text, flush=True)
                out.write(text + "\n")
                out.flush()
            return run(form, int(log_n), args.reps, emit)
    open(args.out, "w").close()
    for step in args.steps.split(","):   # chained: nothing more is started on the GPU after a step that did not end well
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step,
               "--reps", str(args.reps), "--out", args.out]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print("time_crs_from_powers: step %s ended with status %d; stopping" % (step, rc), file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
