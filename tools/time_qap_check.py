"""Times zk_qap_check_dev on resident witnesses, with the figures it is to be compared against taken in the same process: one JSON
line per shape.

    python tools/time_qap_check.py [--single 1024,65536,1048576] [--batches 16x65536,1024x4096] [--reps 20] [--prove-reps 3]
                                   [--out profiles/qap_check.jsonl]

Circuit: the chain (circuits.chain_rows / chain_zk; m = 2 n + 2), roots-of-unity form.  Every time is the median of `reps` timed calls
after 3 warm-up calls; a call is complete on return (the clock needs no further synchronisation).

    single  one witness resident in HBM: `first_check_ms` (the first check of the handle: builds W by gate), `check_ms`, and the summed
            qap_spmv time of one proof of the same circuit from Context.profile() (two launches, u and v) -- the bar is
            check_ms <= 2 x that sum
    batch   `count` witnesses from Witgen, checked in place: the rate for both lane mappings (option qap_check_by_instance), the
            generate-and-prove rate of the same shape (zk_witgen_run + zk_prove_batch_submit in batches of 64, two tickets in flight, as
            tools/time_witgen.py measures it) -- the bar is check rate >= 10 x that rate -- and the same batch with every instance
            corrupted at one gate against the satisfying batch, three repeats each (`*_spread`: min and max of the three medians)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zksnark_rs_amd as zk  # noqa: E402
from zksnark_rs_amd.circuit import Circuit, Witgen  # noqa: E402
from zksnark_rs_amd.circuits import chain_rows, chain_weights, chain_zk  # noqa: E402

WARM = 3
DISTINCT = 64
BATCH = zk._lib.MAX_BATCH


def timed(fn, reps):
    for _ in range(WARM):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def med(xs):
    return dict(median=round(float(np.median(xs)), 4), min=round(min(xs), 4), max=round(max(xs), 4))


def single(ctx, torch, n, reps, emit):
    log_n = n.bit_length() - 1
    m, l, u, v, w = chain_rows(log_n)
    rng = zk.SplitMix64(n)
    wts = chain_weights(log_n, rng.fr(), [rng.fr() for _ in range(n)])
    d = torch.from_numpy(np.ascontiguousarray(wts).view(np.int64)).cuda()
    torch.cuda.synchronize()
    qap = ctx.qap_sparse(log_n, m, l, u, v, w)
    t0 = time.perf_counter()
    res = ctx.qap_check_dev(qap, d.data_ptr(), m, 1)
    first_ms = (time.perf_counter() - t0) * 1e3
    ok = (int(res["bad_gates"][0]), int(res["flags"][0])) == (0, 0)
    ts = timed(lambda: ctx.qap_check_dev(qap, d.data_ptr(), m, 1), reps)
    # the kernel alone, and the prover's two qap_spmv launches of one proof, from the library's event timing
    ctx.set_option("profile", 2)
    ctx.profile_reset()
    for _ in range(reps):
        ctx.qap_check_dev(qap, d.data_ptr(), m, 1)
    kern = ctx.profile()["qap_check"]
    crs = ctx.setup(qap, [rng.fr() for _ in range(5)])
    r, s = rng.fr(), rng.fr()
    ctx.set_option("profile", 0)
    for _ in range(2):
        ctx.prove_dev(crs, qap, d.data_ptr(), m, r, s)       # the first proof builds the tables
    ctx.set_option("profile", 2)
    proofs = 5
    ctx.profile_reset()
    for _ in range(proofs):
        ctx.prove_dev(crs, qap, d.data_ptr(), m, r, s)
    sp = ctx.profile()["qap_spmv"]
    ctx.set_option("profile", 0)
    ctx.profile_reset()
    assert sp["launches"] == 2 * proofs, sp
    spmv_ms = sp["total_ms"] / proofs
    c = float(np.median(ts))
    emit(dict(tool="time_qap_check", mode="single", circuit="chain", gates=n, m=m, reps=reps, satisfied=ok, first_check_ms=round(first_ms, 3),
              check_ms=med(ts), check_kernels_ms=round(kern["total_ms"] / kern["launches"], 4), qap_spmv_ms_per_proof=round(spmv_ms, 4),
              check_over_spmv=round(c / spmv_ms, 2), bar="check_ms <= 2 x qap_spmv_ms_per_proof", bar_met=bool(c <= 2 * spmv_ms)))


def batch(ctx, torch, n, count, reps, prove_reps, emit):
    log_n = n.bit_length() - 1
    c = Circuit(chain_zk(n))
    rng = np.random.default_rng(n)
    ins = rng.integers(0, 1 << 63, size=(DISTINCT, c.n_in, 4), dtype=np.uint64)
    ins[:, :, 3] &= np.uint64((1 << 60) - 1)                # < 2^252 < r
    d_in = torch.from_numpy(ins.view(np.int64)).cuda()[torch.arange(count, device="cuda") % DISTINCT].contiguous()
    d_out = torch.empty((count, c.m, 4), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    wg = Witgen(ctx, c)
    m_, l_, u, v, w = chain_rows(log_n)
    assert m_ == c.m
    qap = ctx.qap_sparse(log_n, m_, l_, u, v, w)
    srng = zk.SplitMix64(n)
    crs = ctx.setup(qap, [srng.fr() for _ in range(5)])
    rs, ss = [srng.fr() for _ in range(BATCH)], [srng.fr() for _ in range(BATCH)]

    def gen_prove():
        t0 = time.perf_counter()
        wg.run(d_in.data_ptr(), count, d_out.data_ptr())
        pending = []
        for j0 in range(0, count, BATCH):
            k = min(BATCH, count - j0)
            ptrs = [d_out.data_ptr() + (j0 + j) * c.m * 32 for j in range(k)]
            pending.append((ctx.prove_batch_submit(crs, qap, ptrs, [c.m] * k, rs[:k], ss[:k]), k))
            if len(pending) == 2:
                ctx.prove_batch_wait(*pending.pop(0))
        for p in pending:
            ctx.prove_batch_wait(*p)
        return (time.perf_counter() - t0) * 1e3

    gen_prove()
    prove_ms = [gen_prove() for _ in range(prove_reps)]
    prove_rate = count / float(np.median(prove_ms)) * 1e3

    def check():
        return ctx.qap_check_dev(qap, d_out.data_ptr(), c.m, count)

    first = check()
    all_ok = not first["bad_gates"].any() and not first["flags"].any()
    rates = {}
    for by_instance in (0, 1):
        ctx.set_option("qap_check_by_instance", by_instance)
        rates[by_instance] = [count / float(np.median(timed(check, reps))) * 1e3 for _ in range(3)]
    ctx.set_option("qap_check_by_instance", 0)
    # every instance corrupted at one gate: a_3 = wire 8 replaced (gate 2 fails in every instance)
    d_out[:, 8, 0] += 1
    torch.cuda.synchronize()
    bad = check()
    all_bad = bool((bad["bad_gates"] == 1).all() and (bad["first_bad"] == 2).all())
    corrupted = [count / float(np.median(timed(check, reps))) * 1e3 for _ in range(3)]
    r0, r1 = float(np.median(rates[0])), float(np.median(rates[1]))
    spread = lambda xs: dict(median=round(float(np.median(xs)), 1), min=round(min(xs), 1), max=round(max(xs), 1))
    emit(dict(tool="time_qap_check", mode="batch", circuit="chain_zk", gates=n, m=c.m, count=count, reps=reps, all_satisfied=bool(all_ok),
              corrupted_all_found=all_bad, checks_per_s_gate_lanes=spread(rates[0]), checks_per_s_instance_lanes=spread(rates[1]),
              shipped_mapping="gate_lanes" if r0 >= r1 else "instance_lanes", gen_prove_ms=med(prove_ms), gen_prove_proofs_per_s=round(prove_rate, 1),
              check_over_gen_prove=round(r0 / prove_rate, 1), bar="checks_per_s >= 10 x gen_prove_proofs_per_s", bar_met=bool(r0 >= 10 * prove_rate),
              satisfying_checks_per_s_spread=spread(rates[0]), corrupted_checks_per_s_spread=spread(corrupted)))
    wg.close()
    del d_in, d_out
    torch.cuda.empty_cache()


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--single", default="1024,65536,1048576")
    ap.add_argument("--batches", default="16x65536,1024x4096")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--prove-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = zk.Context(0)
    out = open(args.out, "w") if args.out else None

    def emit(line):
        print(json.dumps(line), flush=True)
        if out:
            out.write(json.dumps(line) + "\n")
            out.flush()

    for n in [int(s) for s in args.single.split(",") if s]:
        assert n == 1 << (n.bit_length() - 1)
        single(ctx, torch, n, args.reps, emit)
    for shape in [s for s in args.batches.split(",") if s]:
        n, count = (int(x) for x in shape.split("x"))
        batch(ctx, torch, n, count, args.reps, args.prove_reps, emit)
    if out:
        out.close()


if __name__ == "__main__":
    main()
