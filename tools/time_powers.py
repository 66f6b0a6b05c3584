"""Times zk_powers_contribute with both multiplication kernels, the kernels alone, and zk_powers_check next to zk_crs_check: JSON
lines into profiles/powers.jsonl.

    python tools/time_powers.py [--steps 10,16,20] [--reps 7] [--out profiles/powers.jsonl] [--step-timeout 420]

One child process per step (the transcript for n = 2^K gates: N1 = 2n - 1 powers in G1, N2 = n in the other arrays), each under its own
`timeout`, chained: a step that fails, faults or runs out of time ends the run there.  Within a step everything is warm and the two
forms of the option powers_mul_form are ALTERNATED, so both see the same clocks and the same neighbours on the machine:
  form 0   k_mul_each (regular signed windows, the same instruction stream in every lane): profile names mul_each_g1 / mul_each_g2
  form 1   k_mul_each_gb (gb_mul, a per-lane non-adjacent form -- what there was before): mul_each_gb_g1 / mul_each_gb_g2
Wall times are host clocks around the synchronous call; kernel times are HIP events on the call's stream (the context's profile),
summed over the launches of a group (G1: tau_g1, alpha_tau_g1, beta_tau_g1 = 4n - 1 points; G2: tau_g2 and beta_g2 = n + 1 points).
`spread` is (max - min) / median of form 1's kernel time over the repetitions: the run-to-run noise a ratio has to clear.
`new_over_old` below 1 means k_mul_each is faster.  The two forms' transcripts are compared byte for byte at every size that is timed.
Then zk_powers_check on the result next to zk_crs_check on the CRS zk_crs_from_powers derives from it (the chain circuit)."""
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


def spread(times):
    return round((max(times) - min(times)) / float(np.median(times)), 4)


def run_step(log_n, reps, emit):
    import zksnark_rs_amd as zk
    from zksnark_rs_amd import SplitMix64
    from zksnark_rs_amd.circuits import chain_rows
    ctx = zk.Context(0)
    ctx.set_option("profile", 2)
    rng = SplitMix64(9393 + log_n)
    n = 1 << log_n
    n1, n2 = 2 * n - 1, n
    secrets = (rng.fr(), rng.fr(), rng.fr())
    ctx.set_option("powers_mul_form", 0)
    head = ctx.powers_initial(n1, n2)
    (before, _), first = once(lambda: ctx.powers_contribute(head, (rng.fr(), rng.fr(), rng.fr())))   # distinct points; loads the code objects
    head.close()
    names = {0: ("mul_each_g1", "mul_each_g2"), 1: ("mul_each_gb_g1", "mul_each_gb_g2")}
    wall, k1, k2, result = {0: [], 1: []}, {0: [], 1: []}, {0: [], 1: []}, {}
    for form in (0, 1):                                # warm both forms at this size
        ctx.set_option("powers_mul_form", form)
        ctx.powers_contribute(before, secrets)[0].close()
    for _ in range(reps):
        for form in (0, 1):
            ctx.set_option("powers_mul_form", form)
            ctx.profile_reset()
            (after, rec), t = once(lambda: ctx.powers_contribute(before, secrets))
            prof = ctx.profile()
            wall[form].append(t)
            k1[form].append(prof.get(names[form][0], dict(total_ms=0.0))["total_ms"])
            k2[form].append(prof.get(names[form][1], dict(total_ms=0.0))["total_ms"])
            if form in result:
                after.close()
            else:
                result[form] = after
    a, b = ctx.powers_download(result[0]), ctx.powers_download(result[1])
    equal = all(a[k].tobytes() == b[k].tobytes() for k in a)
    del a, b
    result[1].close()
    med = lambda xs: float(np.median(xs))   # noqa: E731
    g1_points, g2_points = 4 * n - 1, n + 1
    line = dict(tool="time_powers", step="contribute:%d" % log_n, commit=commit_hash(), gates=n, n_tau_g1=n1, n_rest=n2, reps=reps,
                forms_equal=bool(equal), first_contribute_ms=round(first, 3),
                g1_new_over_old=round(med(k1[0]) / med(k1[1]), 4), g2_new_over_old=round(med(k2[0]) / med(k2[1]), 4),
                wall_new_over_old=round(med(wall[0]) / med(wall[1]), 4),
                g1_old_spread=spread(k1[1]), g2_old_spread=spread(k2[1]), wall_old_spread=spread(wall[1]),
                g1_new_ns_per_point=round(1e6 * med(k1[0]) / g1_points, 1), g1_old_ns_per_point=round(1e6 * med(k1[1]) / g1_points, 1),
                g2_new_ns_per_point=round(1e6 * med(k2[0]) / g2_points, 1), g2_old_ns_per_point=round(1e6 * med(k2[1]) / g2_points, 1),
                **stats("contribute_new", wall[0]), **stats("contribute_old", wall[1]), **stats("g1_kernel_new", k1[0]),
                **stats("g1_kernel_old", k1[1]), **stats("g2_kernel_new", k2[0]), **stats("g2_kernel_old", k2[1]))
    emit(line)
    # ---- the check of the transcript next to the check of a CRS derived from it ----
    ctx.set_option("powers_mul_form", 0)
    powers = result[0]
    m, l, u, v, w = chain_rows(log_n)
    qap = ctx.qap_sparse(log_n, m, l, u, v, w)
    crs, t_derive = once(lambda: ctx.crs_from_powers(qap, powers))
    ok_p, ok_c = ctx.powers_check(powers).ok, ctx.crs_check(crs, qap).ok       # warm; builds what the first crs_check builds on the QAP
    t_pc, t_cc = [], []
    for _ in range(reps):
        res_p, t = once(lambda: ctx.powers_check(powers))
        t_pc.append(t)
        res_c, t = once(lambda: ctx.crs_check(crs, qap))
        t_cc.append(t)
    emit(dict(tool="time_powers", step="check:%d" % log_n, commit=commit_hash(), gates=n, n_tau_g1=n1, n_rest=n2, reps=reps,
              ok=bool(ok_p and ok_c and res_p.ok and res_c.ok), from_powers_with_download_ms=round(t_derive, 3),
              powers_check_over_crs_check=round(med(t_pc) / med(t_cc), 3), **stats("powers_check", t_pc), **stats("crs_check", t_cc)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="10,16,20")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "powers.jsonl"))
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds each step's child process may take")
    ap.add_argument("--step", default=None, help="run one step in this process (what the steps do)")
    args = ap.parse_args()
    if args.step:
        with open(args.out, "a") as out:
            def emit(line):
                text = json.dumps(line)
                print(text, flush=True)
                out.write(text + "\n")
                out.flush()
            run_step(int(args.step), args.reps, emit)
        return 0
    open(args.out, "w").close()
    for step in args.steps.split(","):   # chained: nothing more is started on the GPU after a step that did not end well
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step,
               "--reps", str(args.reps), "--out", args.out]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print("time_powers: step %s ended with status %d; stopping" % (step, rc), file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
